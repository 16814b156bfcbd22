"""The oriented tensor / YUV entries against the path a caller had before them (profiles/oriented_entry.md): FACE80, 2048 trees,
colorSpace luv on RGB input, a 1080 x 1920 source, 96 frames a call, orientation codes 1 (upright 1920 x 1080) and 2.
On the same frames, alternating in one process, whole calls timed by the host clock around a synchronise (option "profile" off):
  channels_last uint8   composed: torch.rot90(x, k, (1, 2)).contiguous() + run_tensor(layout="nhwc")
                        oriented: run_tensor(x, layout="nhwc", orient=code)
  NV12                  composed: acf_hip_yuv_to_rgb8 + torch.rot90(...).contiguous() + run_u8(PIX_RGB)
                        oriented: run_yuv(nv12, ..., orient=code)
then, with option "profile" on (a kernel's time = the span between its marker and the next one on the stream), the ingest kernel of
each oriented call beside the un-oriented ingest kernel on the same layout at the upright size (k_ingest_image on the turned
channels_last tensor, k_ingest_yuv420 on an NV12 frame of the upright size).  Medians with the spread of the rounds, and whether both
sides left the same first pyramid level and the same detections.
  python profiles/oriented_entry.py [--frames 96] [--rounds 8]
"""
import argparse
import ctypes as C
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tests"))
import torch  # noqa: E402

import yuv420_ref as yr  # noqa: E402
from acf_amd import capi, synth  # noqa: E402
from acf_amd.detector import HipDetector  # noqa: E402

H, W, WARM = 1080, 1920, 2


def stats(v, key="median_ms"):
    v = np.array(v)
    return {key: float(np.median(v)), "min": float(v.min()), "max": float(v.max())}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=96)
    ap.add_argument("--rounds", type=int, default=8)
    ap.add_argument("--height", type=int, default=H)
    ap.add_argument("--width", type=int, default=W)
    args = ap.parse_args()
    n, h, w = args.frames, args.height, args.width
    assert torch.cuda.is_available(), "a measurement needs the GPU: there is no CPU path"
    model = synth.make_model(seed=1, nTrees=2048, name="FACE80", isLuv=0)
    # video-like frames: two synthetic ones through the forward BT.601 matrix, the batch filled with shifted copies
    nbase = 2
    Ys, Us, Vs = [], [], []
    for i in range(nbase):
        up = np.clip(np.rint(synth.make_frame(i + 1, h, w, "rgb").transpose(2, 1, 0) * 255.0), 0, 255).astype(np.uint8)
        Y, U, V = yr.planes(yr.from_rgb(up), h, w)
        Ys.append(Y), Us.append(U), Vs.append(V)
    Yb, Ub, Vb = (torch.from_numpy(np.stack(a)).cuda() for a in (Ys, Us, Vs))
    Y = torch.stack([torch.roll(Yb[i % nbase], shifts=(36 * (i // nbase), 52 * (i // nbase)), dims=(0, 1)) for i in range(n)])
    U = torch.stack([torch.roll(Ub[i % nbase], shifts=(18 * (i // nbase), 26 * (i // nbase)), dims=(0, 1)) for i in range(n)])
    V = torch.stack([torch.roll(Vb[i % nbase], shifts=(18 * (i // nbase), 26 * (i // nbase)), dims=(0, 1)) for i in range(n)])
    nv12 = torch.cat([Y.reshape(n, -1), torch.stack([U, V], dim=-1).reshape(n, -1)], dim=1).contiguous()
    dnv, fb = HipDetector.yuv_desc("nv12", h, w)
    assert fb == nv12.shape[1]
    conv = HipDetector()
    rgb = conv.yuv_to_rgb8(nv12, n, h, w, dnv)                                    # [n][h][w][3]: the channels_last source
    conv.close()
    scratch = torch.empty_like(rgb)                                               # the composed NV12 path's converted frames
    torch.cuda.synchronize()

    res = {"lib": os.path.basename(capi.LIB_PATH), "frames": n, "source": [h, w], "rounds": args.rounds, "codes": {}}
    for code in (1, 2):
        uh, uw = HipDetector.oriented_dims(h, w, code)
        k = {1: -1, 2: 2}[code]                                                   # torch.rot90's count for the code (clockwise = -1)
        det = HipDetector()
        det.set_model(model)
        det.plan(uh, uw, 3, n, 1 << 15)

        def composed_u8():
            turned = torch.rot90(rgb, k, (1, 2)).contiguous()
            torch.cuda.synchronize()                                              # (torch's stream, then the context's)
            det.run_tensor(turned, layout="nhwc")
            det.synchronize()

        def composed_nv12():
            det._chk(det.lib.acf_hip_yuv_to_rgb8(det.ctx, C.c_void_p(nv12.data_ptr()), n, h, w, C.byref(dnv), C.c_void_p(scratch.data_ptr())))
            det.synchronize()
            turned = torch.rot90(scratch, k, (1, 2)).contiguous()
            torch.cuda.synchronize()
            det.run_u8(turned, capi.PIX_RGB)
            det.synchronize()

        def oriented_u8():
            det.run_tensor(rgb, layout="nhwc", orient=code)
            det.synchronize()

        def oriented_nv12():
            det.run_yuv(nv12, n, dnv, code, h, w)
            det.synchronize()

        sides = {"u8 composed": composed_u8, "u8 oriented": oriented_u8, "nv12 composed": composed_nv12, "nv12 oriented": oriented_nv12}
        ms = {s: [] for s in sides}
        left = {}
        for r in range(WARM + args.rounds):
            for what, fn in sides.items():
                t0 = time.perf_counter()
                fn()
                dt = (time.perf_counter() - t0) * 1e3
                if r == 0:
                    left[what] = (det.read_level(n - 1, 0).tobytes(), det.detections(n - 1)[0].tobytes())
                if r >= WARM:
                    ms[what].append(dt)
        out = {"upright": [uh, uw], "call_ms": {s: stats(v) for s, v in ms.items()}}
        out["frames_per_s"] = {s: n * 1e3 / out["call_ms"][s]["median_ms"] for s in sides}
        out["same_first_level_and_detections"] = left["u8 composed"] == left["u8 oriented"] == left["nv12 composed"] == left["nv12 oriented"]
        out["detections_in_last_frame"] = len(left["u8 oriented"][1]) // capi.DET_DTYPE.itemsize
        out["oriented_not_slower"] = {p: out["call_ms"][p + " oriented"]["median_ms"] <= out["call_ms"][p + " composed"]["median_ms"] for p in ("u8", "nv12")}
        # the ingest kernels, option "profile": the oriented ones beside the un-oriented ones on the same layout at the upright size
        det.set_option("profile", 1)
        turned = torch.rot90(rgb, k, (1, 2)).contiguous()
        dup, fbu = HipDetector.yuv_desc("nv12", uh, uw)
        upnv = nv12.reshape(-1)[:n * fbu].reshape(n, fbu)                         # (the same bytes read as frames of the upright size: timing only)
        torch.cuda.synchronize()
        kern = {
            "k_ingest_image_oriented_" + ("cols" if code & 1 else "rows"): lambda: det.pyramid_tensor(rgb, layout="nhwc", orient=code),
            "k_ingest_image": lambda: det.pyramid_tensor(turned, layout="nhwc"),
            "k_ingest_yuv_oriented_" + ("cols" if code & 1 else "rows"): lambda: det.pyramid_yuv(nv12, n, dnv, code, h, w),
            "k_ingest_yuv420": lambda: det.pyramid_yuv(upnv, n, dup),
        }
        kms = {name: [] for name in kern}
        for r in range(WARM + args.rounds):
            for name, fn in kern.items():
                det.profile()
                fn()
                det.synchronize()
                p = det.profile()
                if r >= WARM:
                    kms[name].append(p[name][0] / p[name][1])
        out["ingest_kernel_ms_per_batch"] = {name: stats(v) for name, v in kms.items()}
        px = n * h * w
        out["ingest_GB_per_s"] = {name: (px * (3 if "image" in name else 1.5) + px * 12) / out["ingest_kernel_ms_per_batch"][name]["median_ms"] / 1e6 for name in kern}
        det.close()
        res["codes"][str(code)] = out
    print(json.dumps(res))


if __name__ == "__main__":
    main()
