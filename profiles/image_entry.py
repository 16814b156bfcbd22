"""The image entry for upright device tensors against the only routes the parent commit offers for the same tensor
(profiles/image_entry.md): FACE80, 2048 trees, colorSpace luv on RGB input, 1920 x 1080, 64 frames per call, one context.
  (a) float32 NCHW:  run_tensor(x)   against   run(x.transpose(-1, -2).contiguous())
  (b) uint8 NCHW:    run_tensor(x)   against   run_u8(x.permute(0, 2, 3, 1).contiguous(), PIX_RGB)
One process, torch and the detector on one stream; warm-up, then the two sides of a pair alternate; medians with the spread of
the repetitions.  Then, with option "profile", k_ingest_image's own time beside k_ingest_u8's on packed RGB bytes of the same
frames (and on the two NCHW layouts).
  python profiles/image_entry.py [--frames 64] [--reps 12]
"""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402

from acf_amd import capi, synth  # noqa: E402
from acf_amd.detector import HipDetector  # noqa: E402

H, W, WARM = 1080, 1920, 3


def stats(v):
    v = np.array(v) * 1e3
    return {"median_ms": float(np.median(v)), "min_ms": float(v.min()), "max_ms": float(v.max())}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=64)
    ap.add_argument("--reps", type=int, default=12)
    ap.add_argument("--height", type=int, default=H)
    ap.add_argument("--width", type=int, default=W)
    args = ap.parse_args()
    n, h, w = args.frames, args.height, args.width
    model = synth.make_model(seed=1, nTrees=2048, name="FACE80", isLuv=0)
    stream = torch.cuda.Stream()
    res = {"lib": os.path.basename(capi.LIB_PATH), "frames": n, "size": [h, w], "reps": args.reps}
    with torch.cuda.stream(stream):
        nbase = 8
        base = torch.from_numpy(np.stack([synth.make_frame(i + 1, h, w, "rgb") for i in range(nbase)])).cuda()      # [8][3][W][H]
        x = torch.empty((n, 3, h, w), dtype=torch.float32, device="cuda")                                            # upright NCHW
        for i in range(n):
            x[i] = torch.roll(base[i % nbase], shifts=(37 * (i // nbase), 53 * (i // nbase)), dims=(1, 2)).transpose(-1, -2)
        del base
        xu8 = torch.round(x * 255.0).to(torch.uint8)
        det = HipDetector(model, h, w, 3, max_batch=n, max_hits=1 << 15, stream=stream.cuda_stream)

        def timed(fn):
            t0 = time.perf_counter()
            fn()
            det.synchronize()
            return time.perf_counter() - t0

        def digest():
            return [det.detections(f)[0].tobytes() for f in (0, n // 2, n - 1)]

        pairs = {
            "a_f32_nchw": (lambda: det.run_tensor(x), lambda: det.run(x.transpose(-1, -2).contiguous())),
            "b_u8_nchw": (lambda: det.run_tensor(xu8), lambda: det.run_u8(xu8.permute(0, 2, 3, 1).contiguous(), capi.PIX_RGB)),
        }
        for name, (new, parent) in pairs.items():
            for _ in range(WARM):
                timed(new)
                timed(parent)
            timed(new)
            d_new = digest()
            timed(parent)
            same = d_new == digest()
            t_new, t_parent = [], []
            for _ in range(args.reps):
                t_new.append(timed(new))
                t_parent.append(timed(parent))
            s_new, s_par = stats(t_new), stats(t_parent)
            res[name] = {"run_tensor": s_new, "parent_route": s_par, "same_detections": bool(same),
                         "parent_spread_ms": s_par["max_ms"] - s_par["min_ms"],
                         "run_tensor_minus_parent_ms": s_new["median_ms"] - s_par["median_ms"],
                         "frames_per_s": {"run_tensor": n / s_new["median_ms"] * 1e3, "parent_route": n / s_par["median_ms"] * 1e3}}
        det.close()
        del det

        # the ingest kernels' own times (option "profile"): the same frames as packed RGB bytes through both entries, and the NCHW layouts
        prof = HipDetector(stream=stream.cuda_stream)
        prof.set_option("profile", 1)
        prof.set_model(model)
        prof.plan(h, w, 3, n, 1 << 15)
        packed = xu8.permute(0, 2, 3, 1).contiguous()
        calls = {
            "k_ingest_u8, packed RGB bytes": (lambda: prof.run_u8(packed, capi.PIX_RGB), "k_ingest_u8"),
            "k_ingest_image, packed RGB bytes (nhwc)": (lambda: prof.run_tensor(packed, layout="nhwc"), "k_ingest_image"),
            "k_ingest_image, uint8 NCHW": (lambda: prof.run_tensor(xu8), "k_ingest_image"),
            "k_ingest_image, float32 NCHW": (lambda: prof.run_tensor(x), "k_ingest_image"),
            "k_ingest_image, float32 NHWC": (lambda: prof.run_tensor(x.permute(0, 2, 3, 1).contiguous(), layout="nhwc"), "k_ingest_image"),
        }
        kernel_ms = {}
        for what, (fn, kernel) in calls.items():
            for _ in range(2):
                fn()
                prof.synchronize()
            prof.profile()
            for _ in range(5):
                fn()
                prof.synchronize()
            p = prof.profile()
            kernel_ms[what] = p[kernel][0] / p[kernel][1]
        res["kernel_ms_per_call"] = kernel_ms
        # bytes the kernels move per call: input elements + three f32 output planes
        px = n * h * w
        res["ingest_bytes_per_call"] = {"packed or planar uint8": px * (3 + 12), "float32": px * (12 + 12)}
        prof.close()
    print(json.dumps(res))


if __name__ == "__main__":
    main()
