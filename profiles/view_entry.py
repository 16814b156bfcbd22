"""Measurement for profiles/view_entry.md: k_ingest_view beside the ingest kernel of the plain entry on the same frames — 96 frames of
1080 x 1920, NV12 and uint8 NHWC — for the identity view, a 20 degree tilt and a 2 x zoom-out (s = 1), and the zoom-out with s = 2.
Kernel times are the library's own event spans (option "profile"), the median over REPS pyramid calls behind WARM warm-up calls; the
plain entry and the views alternate inside every repetition.  Prints one JSON line; `python profiles/view_entry.py [out.json]` also
writes it to a file."""
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np
import torch

import resized_entry_case as rc
import yuv_desc_ref as ydr
from acf_amd import synth
from acf_amd.detector import HipDetector

H, W, NF = 1080, 1920, 96
REPS, WARM = 10, 2
TILE = 64


def video_frames():
    return [rc.yuv_planes(900 + i, H, W, 1, 1) for i in range(4)]


def main():
    model = synth.make_model(seed=1, name="FACE80", isLuv=0)                     # rgb2luv in the ingest: H * W % 4 == 0, the vector body
    det = HipDetector(model, H, W, 3, max_batch=NF, max_hits=1 << 12)
    planes = video_frames()
    nv12 = np.stack([ydr.pack("nv12", *planes[i % 4]) for i in range(NF)])
    rgb = np.stack([rc.rgb_u8(900 + i, H, W) for i in range(4)])
    rgb = np.stack([rgb[i % 4] for i in range(NF)])                              # [NF][H][W][3]
    desc, fb = HipDetector.yuv_desc("nv12", H, W)
    xn, xr = torch.from_numpy(nv12).cuda(), torch.from_numpy(rgb).cuda()
    torch.cuda.synchronize()
    sources = {"nv12": (det.crop_source_yuv(xn, NF, desc, None, H, W, 0), lambda: det.pyramid_yuv(xn, NF, desc), "k_ingest_yuv420", "k_ingest_view_yuv"),
               "u8_nhwc": (det.crop_source_tensor(xr, layout="nhwc"), lambda: det.pyramid_tensor(xr, layout="nhwc"), "k_ingest_image", "k_ingest_view_image")}
    views = {"identity s1": (np.array([1, 0, 0, 0, 1, 0], np.float32), 1),
             "tilt 20 s1": (HipDetector.view_from_box((0, 0, W, H), 20 * np.pi / 180, H, W), 1),
             "zoom-out 2x s1": (HipDetector.view_from_box((-W / 2, -H / 2, 2 * W, 2 * H), 0.0, H, W), 1),
             "zoom-out 2x s2": (HipDetector.view_from_box((-W / 2, -H / 2, 2 * W, 2 * H), 0.0, H, W), 2)}
    det.set_option("profile", 1)
    res = {"frames": NF, "size": [H, W], "reps": REPS, "warm": WARM, "sources": {}}
    for sname, (src, plain, kplain, kview) in sources.items():
        dev_views = {k: torch.from_numpy(np.tile(m, (NF, 1))).cuda() for k, (m, s) in views.items()}
        torch.cuda.synchronize()
        ms = {"plain " + kplain: []}
        ms.update({k: [] for k in views})
        for rep in range(WARM + REPS):
            det.profile()
            plain()
            det.synchronize()
            t = det.profile()[kplain][0]
            if rep >= WARM:
                ms["plain " + kplain].append(t)
            for k, (m, s) in views.items():
                det.pyramid_view(src, dev_views[k], None, s)
                det.synchronize()
                t = det.profile()[kview][0]
                if rep >= WARM:
                    ms[k].append(t)
        out = {k: dict(ms_median=float(np.median(v)), ms_min=float(np.min(v)), ms_max=float(np.max(v))) for k, v in ms.items()}
        base = out["plain " + kplain]["ms_median"]
        for k in views:
            out[k]["ratio_to_plain"] = out[k]["ms_median"] / base
            m, s = views[k]
            forms = [HipDetector.view_form(m, s, tx, ty, H, W, H, W, 3, 1) for ty in range(-(-H // TILE)) for tx in range(-(-W // TILE))]
            out[k]["tiles_staged_gather"] = [forms.count(0), forms.count(1)]
        res["sources"][sname] = out
    # bytes by arithmetic: what the plain kernel and the identity view both read and write
    res["bytes"] = {"nv12_read": int(NF * fb), "u8_read": int(NF * H * W * 3), "planes_written": int(NF * H * W * 3 * 4)}
    if len(sys.argv) > 1:
        with open(sys.argv[1], "w") as fh:
            json.dump(res, fh, indent=1)
    print(json.dumps(res))
    det.close()


if __name__ == "__main__":
    main()
