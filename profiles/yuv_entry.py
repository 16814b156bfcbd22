"""The three-plane YUV entry's ingest kernel against what it replaces (profiles/yuv_entry.md): FACE80, 2048 trees, colorSpace luv on
RGB input, 1920 x 1080, 96 frames per call, one context, option "profile" (a kernel's time = the span between its marker and the
next one on the stream).  On the same frames, alternating in one process:
  fused     pyramid_yuv(I420, 4-aligned)   k_ingest_yuv_planar       pyramid_yuv(YUYV, 4-aligned)   k_ingest_yuv_packed422
  unfused   yuv_to_rgb8 + pyramid_u8(RGB)  k_yuv_to_rgb8 + k_ingest_u8   (for each of the two layouts)
  nv12      pyramid_u8(PIX_NV12)           k_ingest_yuv420           (the NV12 form of the same frames)
  generic   pyramid_yuv(I420) from a base one byte further: k_ingest_yuv_generic
Medians with the spread of the rounds, and whether the sides left the same first pyramid level.
  python profiles/yuv_entry.py [--frames 96] [--rounds 10]
"""
import argparse
import ctypes as C
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tests"))
import torch  # noqa: E402

import yuv420_ref as yr  # noqa: E402
from acf_amd import capi, synth  # noqa: E402
from acf_amd.detector import HipDetector  # noqa: E402

H, W, WARM = 1080, 1920, 2


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=96)
    ap.add_argument("--rounds", type=int, default=10)
    ap.add_argument("--height", type=int, default=H)
    ap.add_argument("--width", type=int, default=W)
    args = ap.parse_args()
    n, h, w = args.frames, args.height, args.width
    assert torch.cuda.is_available(), "a measurement needs the GPU: there is no CPU path"
    model = synth.make_model(seed=1, nTrees=2048, name="FACE80", isLuv=0)
    # video-like frames: a few synthetic ones through the forward BT.601 matrix, the batch filled with shifted copies
    nbase = 4
    Ys, Us, Vs = [], [], []
    for i in range(nbase):
        up = np.clip(np.rint(synth.make_frame(i + 1, h, w, "rgb").transpose(2, 1, 0) * 255.0), 0, 255).astype(np.uint8)
        Y, U, V = yr.planes(yr.from_rgb(up), h, w)
        Ys.append(Y), Us.append(U), Vs.append(V)
    Yb, Ub, Vb = (torch.from_numpy(np.stack(a)).cuda() for a in (Ys, Us, Vs))
    Y = torch.stack([torch.roll(Yb[i % nbase], shifts=(36 * (i // nbase), 52 * (i // nbase)), dims=(0, 1)) for i in range(n)])
    U = torch.stack([torch.roll(Ub[i % nbase], shifts=(18 * (i // nbase), 26 * (i // nbase)), dims=(0, 1)) for i in range(n)])
    V = torch.stack([torch.roll(Vb[i % nbase], shifts=(18 * (i // nbase), 26 * (i // nbase)), dims=(0, 1)) for i in range(n)])
    i420 = torch.cat([Y.reshape(n, -1), U.reshape(n, -1), V.reshape(n, -1)], dim=1).contiguous()
    nv12 = torch.cat([Y.reshape(n, -1), torch.stack([U, V], dim=-1).reshape(n, -1)], dim=1).contiguous()
    U2, V2 = U.repeat_interleave(2, dim=1), V.repeat_interleave(2, dim=1)        # 4:2:2: every chroma row twice
    yuyv = torch.stack([Y[:, :, 0::2], U2, Y[:, :, 1::2], V2], dim=-1).reshape(n, -1).contiguous()
    shifted = torch.empty(i420.numel() + 4, dtype=torch.uint8, device="cuda")
    shifted[1:1 + i420.numel()] = i420.reshape(-1)
    rgb = torch.empty((n, h, w, 3), dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    d420, fb420 = HipDetector.yuv_desc("i420", h, w)
    d422, fb422 = HipDetector.yuv_desc("yuyv", h, w)
    assert fb420 == i420.shape[1] and fb422 == yuyv.shape[1] and HipDetector.u8_frame_bytes(capi.PIX_NV12, h, w) == nv12.shape[1]

    det = HipDetector()
    det.set_option("profile", 1)
    det.set_model(model)
    det.plan(h, w, 3, n, 1 << 15)

    def to_rgb(src, desc):
        det._chk(det.lib.acf_hip_yuv_to_rgb8(det.ctx, C.c_void_p(src.data_ptr()), n, h, w, C.byref(desc), C.c_void_p(rgb.data_ptr())))

    def unfused(src, desc):
        to_rgb(src, desc)
        det.pyramid_u8(rgb, capi.PIX_RGB)

    sides = {
        "i420 fused": (lambda: det.pyramid_yuv(i420, n, d420), ["k_ingest_yuv_planar"]),
        "i420 unfused pair": (lambda: unfused(i420, d420), ["k_yuv_to_rgb8", "k_ingest_u8"]),
        "yuyv fused": (lambda: det.pyramid_yuv(yuyv, n, d422), ["k_ingest_yuv_packed422"]),
        "yuyv unfused pair": (lambda: unfused(yuyv, d422), ["k_yuv_to_rgb8", "k_ingest_u8"]),
        "nv12 (k_ingest_yuv420)": (lambda: det.pyramid_u8(nv12, capi.PIX_NV12), ["k_ingest_yuv420"]),
        "i420 generic (base + 1)": (lambda: det.pyramid_yuv(shifted.data_ptr() + 1, n, d420), ["k_ingest_yuv_generic"]),
    }
    level0 = {}
    ms = {k: {name: [] for name in kernels} for k, (_, kernels) in sides.items()}
    for r in range(WARM + args.rounds):
        for what, (fn, kernels) in sides.items():
            det.profile()
            fn()
            det.synchronize()
            p = det.profile()
            if r == 0:
                level0[what] = det.read_level(n - 1, 0).tobytes()
            if r >= WARM:
                for name in kernels:
                    ms[what][name].append(p[name][0] / p[name][1])
    det.close()

    def stats(v):
        v = np.array(v)
        return {"median_ms": float(np.median(v)), "min_ms": float(v.min()), "max_ms": float(v.max())}
    res = {"lib": os.path.basename(capi.LIB_PATH), "frames": n, "size": [h, w], "rounds": args.rounds, "kernel_ms_per_call": {}}
    for what, per in ms.items():
        res["kernel_ms_per_call"][what] = {name: stats(v) for name, v in per.items()}
        if len(per) > 1:
            res["kernel_ms_per_call"][what]["sum"] = stats(np.sum([per[name] for name in per], axis=0))
    res["same_first_level"] = {"i420 fused == unfused == generic": level0["i420 fused"] == level0["i420 unfused pair"] == level0["i420 generic (base + 1)"],
                               "i420 fused == nv12": level0["i420 fused"] == level0["nv12 (k_ingest_yuv420)"],
                               "yuyv fused == unfused": level0["yuyv fused"] == level0["yuyv unfused pair"]}
    px = n * h * w
    res["bytes_per_call"] = {"i420 / nv12 fused": px * 1.5 + px * 12, "yuyv fused": px * 2 + px * 12, "unfused pair, i420": px * 1.5 + px * 3 + px * 3 + px * 12,
                             "unfused pair, yuyv": px * 2 + px * 3 + px * 3 + px * 12}
    print(json.dumps(res))


if __name__ == "__main__":
    main()
