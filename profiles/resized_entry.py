"""The resized YUV / tensor entries' kernel against the chain it replaces (profiles/resized_entry.md): FACE80, 2048 trees, colorSpace
luv on RGB input, 3840 x 2160 I420 frames, 32 per call, option "profile" (a kernel's time = the span between its marker and the
next one on the stream), at scale 0.5 (to 1080p) and at resize_scale(80, 150).  On the same frames, alternating in one process:
  (a) fused    pyramid_yuv_resized(I420)                               k_ingest_resized_yuv
  (b) chain    yuv_to_rgb8 + pyramid_u8(RGB) under set_input_resize    k_yuv_to_rgb8 + k_resize_u8 + k_ingest_u8
  (c) nv12     pyramid_u8(PIX_NV12) under set_input_resize             k_yuv420_to_rgb8 + k_resize_u8 + k_ingest_u8
and for a uint8 NCHW tensor of the converted frames:
  fused        pyramid_tensor_resized                                  k_ingest_resized_image
  chain        torch permute(0, 2, 3, 1).contiguous() (torch events) + pyramid_u8(RGB) under set_input_resize: k_resize_u8 + k_ingest_u8
Medians with the spread of the rounds, and whether the sides left the same first pyramid level.
  python profiles/resized_entry.py [--frames 32] [--rounds 10]
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

H, W, WARM = 2160, 3840, 2


def stats(v):
    v = np.array(v)
    return {"median_ms": float(np.median(v)), "min_ms": float(v.min()), "max_ms": float(v.max())}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=32)
    ap.add_argument("--rounds", type=int, default=10)
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
    i420 = torch.cat([Y.reshape(n, -1), U.reshape(n, -1), V.reshape(n, -1)], dim=1).contiguous()
    nv12 = torch.cat([Y.reshape(n, -1), torch.stack([U, V], dim=-1).reshape(n, -1)], dim=1).contiguous()
    d420, fb420 = HipDetector.yuv_desc("i420", h, w)
    assert fb420 == i420.shape[1] and HipDetector.u8_frame_bytes(capi.PIX_NV12, h, w) == nv12.shape[1]
    conv = HipDetector()
    rgb = conv.yuv_to_rgb8(i420, n, h, w, d420)                                   # [n][h][w][3]: the chain's intermediate, and the tensor row's source
    conv.close()
    nchw = rgb.permute(0, 3, 1, 2).contiguous()
    torch.cuda.synchronize()

    res = {"lib": os.path.basename(capi.LIB_PATH), "frames": n, "size": [h, w], "rounds": args.rounds, "scales": {}}
    for tag, scale in (("0.5", 0.5), ("resize_scale(80, 150)", HipDetector.resize_scale(80, 150))):
        dr, dc = HipDetector.resize_dims(h, w, scale)
        fused, chain = HipDetector(), HipDetector()
        for det in (fused, chain):
            det.set_option("profile", 1)
            det.set_model(model)
            det.plan(dr, dc, 3, n, 1 << 15)
        chain.set_input_resize(h, w, scale)
        ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
        repack_ms = []

        def chain_b():
            chain._chk(chain.lib.acf_hip_yuv_to_rgb8(chain.ctx, C.c_void_p(i420.data_ptr()), n, h, w, C.byref(d420), C.c_void_p(rgb.data_ptr())))
            chain.pyramid_u8(rgb, capi.PIX_RGB)

        def chain_tensor():
            ev[0].record()
            packed = nchw.permute(0, 2, 3, 1).contiguous()
            ev[1].record()
            torch.cuda.synchronize()                                               # (torch's stream, then the context's)
            repack_ms.append(ev[0].elapsed_time(ev[1]))
            chain.pyramid_u8(packed, capi.PIX_RGB)
            chain.synchronize()

        sides = {
            "(a) i420 fused": (fused, lambda: fused.pyramid_yuv_resized(i420, n, d420, h, w, scale), ["k_ingest_resized_yuv"]),
            "(b) i420 chain": (chain, chain_b, ["k_yuv_to_rgb8", "k_resize_u8", "k_ingest_u8"]),
            "(c) nv12 chain": (chain, lambda: chain.pyramid_u8(nv12, capi.PIX_NV12), ["k_yuv420_to_rgb8", "k_resize_u8", "k_ingest_u8"]),
            "nchw fused": (fused, lambda: fused.pyramid_tensor_resized(nchw, scale), ["k_ingest_resized_image"]),
            "nchw repack + chain": (chain, chain_tensor, ["k_resize_u8", "k_ingest_u8"]),
        }
        level0 = {}
        ms = {k: {name: [] for name in kernels} for k, (_, _, kernels) in sides.items()}
        for r in range(WARM + args.rounds):
            for what, (det, fn, kernels) in sides.items():
                det.profile()
                fn()
                det.synchronize()
                p = det.profile()
                if r == 0:
                    level0[what] = det.read_level(n - 1, 0).tobytes()
                if r >= WARM:
                    for name in kernels:
                        ms[what][name].append(p[name][0] / p[name][1])
        fused.close()
        chain.close()
        out = {"reduced": [dr, dc], "kernel_ms_per_call": {}}
        for what, per in ms.items():
            out["kernel_ms_per_call"][what] = {name: stats(v) for name, v in per.items()}
            if len(per) > 1:
                out["kernel_ms_per_call"][what]["sum"] = stats(np.sum([per[name] for name in per], axis=0))
        out["kernel_ms_per_call"]["nchw repack + chain"]["torch repack"] = stats(repack_ms[WARM:])
        out["kernel_ms_per_call"]["nchw repack + chain"]["sum with repack"] = stats(
            np.sum([ms["nchw repack + chain"][k] for k in ("k_resize_u8", "k_ingest_u8")], axis=0) + np.array(repack_ms[WARM:]))
        out["same_first_level"] = {"(a) == (b) == (c)": level0["(a) i420 fused"] == level0["(b) i420 chain"] == level0["(c) nv12 chain"],
                                   "nchw fused == chain == (a)": level0["nchw fused"] == level0["nchw repack + chain"] == level0["(a) i420 fused"]}
        a = out["kernel_ms_per_call"]["(a) i420 fused"]["k_ingest_resized_yuv"]
        b = out["kernel_ms_per_call"]["(b) i420 chain"]["sum"]
        out["fused median below the chain's whole range"] = a["median_ms"] < b["min_ms"]
        src, red = n * h * w, n * dr * dc
        out["bytes_per_call"] = {"(a) fused": src * 1.5 + red * 12, "(b) chain": src * 1.5 + src * 3 + src * 3 + red * 3 + red * 3 + red * 12,
                                 "nchw fused": src * 3 + red * 12}
        out["GB_per_s"] = {"(a) fused": out["bytes_per_call"]["(a) fused"] / a["median_ms"] / 1e6,
                           "(b) chain": out["bytes_per_call"]["(b) chain"] / b["median_ms"] / 1e6}
        res["scales"][tag] = out
    print(json.dumps(res))


if __name__ == "__main__":
    main()
