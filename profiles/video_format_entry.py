"""The video entries' ingest kernels against what the parent commit offers for the same frames (profiles/video_format_entry.md):
FACE80, 2048 trees, colorSpace luv on RGB input, 1920 x 1080, 96 frames per call, option "profile" (a kernel's time = the span between
its marker and the next one on the stream), two warm-up rounds then --rounds, the sides alternating inside a round, the first pyramid
level compared before times count.  On the same pictures, in one process:
  p010 fused            pyramid_video(P010, BT.2020 limited)                    k_ingest_yuv16_pairs
  p010 narrowed (a)     torch: words >> 8 -> 8-bit NV12, then pyramid_yuv       torch ms (events) + k_ingest_yuv420       (lossy)
  p010 float rgb (b)    torch: words -> packed float32 RGB, then pyramid_tensor torch ms (events) + k_ingest_image        (lossless)
  planar16 / generic16  yuv420p10le 4-aligned / from a base 2 bytes further     k_ingest_yuv16_planar / k_ingest_yuv16_generic
  nv12 default / bt709  pyramid_yuv(NV12) / pyramid_video(NV12, BT.709)         k_ingest_yuv420 both (constants inline / as an argument)
  parent: i420, nv12    --parent-lib: the parent commit's library on the same frames, alternating with this one's
                                                                                k_ingest_yuv_planar, k_ingest_yuv420
Medians with the spread of the rounds.
  python profiles/video_format_entry.py [--frames 96] [--rounds 10] [--parent-lib path/to/parent/libacf_hip.so]
"""
import argparse
import ctypes as C
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402

from acf_amd import capi, synth  # noqa: E402
from acf_amd.detector import HipDetector  # noqa: E402

H, W, WARM = 1080, 1920, 2


def detector_on(path):
    """A HipDetector bound to another build of the library (the entries both builds have)."""
    main, lib = capi.load(), C.CDLL(path)
    for name in capi.DECLARED_SYMBOLS:
        if hasattr(lib, name):
            getattr(lib, name).argtypes, getattr(lib, name).restype = getattr(main, name).argtypes, getattr(main, name).restype
    orig = capi.load
    capi.load = lambda: lib
    try:
        return HipDetector()
    finally:
        capi.load = orig


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=96)
    ap.add_argument("--rounds", type=int, default=10)
    ap.add_argument("--height", type=int, default=H)
    ap.add_argument("--width", type=int, default=W)
    ap.add_argument("--parent-lib", default="")
    args = ap.parse_args()
    n, h, w = args.frames, args.height, args.width
    assert torch.cuda.is_available(), "a measurement needs the GPU: there is no CPU path"
    model = synth.make_model(seed=1, nTrees=2048, name="FACE80", isLuv=0)
    # video-like 10-bit pictures: a few synthetic frames, the batch filled with shifted copies; 8-bit ones are their top 8 bits
    nbase = 4
    Ys, Us, Vs = [], [], []
    for i in range(nbase):
        p = synth.make_frame(i + 1, h, w, "rgb").transpose(0, 2, 1)
        Ys.append(np.rint(4 * (16 + 219 * p[0])).astype(np.int16))
        Us.append(np.rint(4 * (128 + 90 * (p[1] - 0.5))).astype(np.int16)[::2, ::2])
        Vs.append(np.rint(4 * (128 + 90 * (p[2] - 0.5))).astype(np.int16)[::2, ::2])
    Yb, Ub, Vb = (torch.from_numpy(np.stack(a)).cuda() for a in (Ys, Us, Vs))
    Y = torch.stack([torch.roll(Yb[i % nbase], shifts=(36 * (i // nbase), 52 * (i // nbase)), dims=(0, 1)) for i in range(n)])
    U = torch.stack([torch.roll(Ub[i % nbase], shifts=(18 * (i // nbase), 26 * (i // nbase)), dims=(0, 1)) for i in range(n)])
    V = torch.stack([torch.roll(Vb[i % nbase], shifts=(18 * (i // nbase), 26 * (i // nbase)), dims=(0, 1)) for i in range(n)])
    p010 = torch.cat([(Y << 6).reshape(n, -1), (torch.stack([U, V], dim=-1) << 6).reshape(n, -1)], dim=1).contiguous()       # int16 words
    planar = torch.cat([Y.reshape(n, -1), U.reshape(n, -1), V.reshape(n, -1)], dim=1).contiguous()                            # yuv420p10le
    shifted = torch.empty(planar.numel() + 2, dtype=torch.int16, device="cuda")
    shifted[1:1 + planar.numel()] = planar.reshape(-1)
    Y8, U8, V8 = ((t >> 2).to(torch.uint8) for t in (Y, U, V))
    i420 = torch.cat([Y8.reshape(n, -1), U8.reshape(n, -1), V8.reshape(n, -1)], dim=1).contiguous()
    nv12 = torch.cat([Y8.reshape(n, -1), torch.stack([U8, V8], dim=-1).reshape(n, -1)], dim=1).contiguous()
    narrowed = torch.empty_like(nv12)
    rgbf = torch.empty((n, h, w, 3), dtype=torch.float32, device="cuda")
    torch.cuda.synchronize()
    f10 = HipDetector.video_format(10, 6, "bt2020")
    f10p = HipDetector.video_format(10, 0, "bt2020")
    f709 = HipDetector.video_format(8, 0, "bt709")
    d010, fb010 = HipDetector.video_desc("nv12", h, w, f10)
    dpl, fbpl = HipDetector.video_desc("i420", h, w, f10p)
    d420, fb420 = HipDetector.yuv_desc("i420", h, w)
    dnv, fbnv = HipDetector.yuv_desc("nv12", h, w)
    assert fb010 == 2 * p010.shape[1] and fbpl == 2 * planar.shape[1] and fb420 == i420.shape[1] and fbnv == nv12.shape[1]

    def make(det):
        det.set_option("profile", 1)
        det.set_model(model)
        det.plan(h, w, 3, n, 1 << 15)
        return det
    det = make(HipDetector())
    parent = make(detector_on(args.parent_lib)) if args.parent_lib else None
    # a second context of each build: how far two contexts of ONE build lie apart (their planes are other allocations) is the yardstick
    # for the distance between the builds
    det2 = make(HipDetector()) if parent is not None else None
    parent2 = make(detector_on(args.parent_lib)) if parent is not None else None
    yoff, cmid, omax, cy, cvr, cvg, cug, cub = (float(v) for v in HipDetector.yuv_coeffs(f10))

    def narrow():                                                       # (a) the user's own pass: 10-bit P010 words -> 8-bit NV12
        narrowed.copy_(p010.view(torch.uint8).view(n, -1, 2)[:, :, 1])   # the high byte of every word

    def to_float():                                                     # (b) the user's own pass: P010 -> packed float32 RGB in [0, 1]
        words = ((p010.view(n, -1).to(torch.int32) & 0xFFFF) >> 6).float()
        y = (words[:, :h * w].view(n, h, w) - yoff).clamp_(min=0) * (cy / 1048576.0)
        c = words[:, h * w:].view(n, h // 2, w // 2, 2) - cmid
        u = c[..., 0].repeat_interleave(2, 1).repeat_interleave(2, 2)
        v = c[..., 1].repeat_interleave(2, 1).repeat_interleave(2, 2)
        rgbf[..., 0] = ((y + (cvr / 1048576.0) * v) / omax).clamp_(0, 1)
        rgbf[..., 1] = ((y + (cvg / 1048576.0) * v + (cug / 1048576.0) * u) / omax).clamp_(0, 1)
        rgbf[..., 2] = ((y + (cub / 1048576.0) * u) / omax).clamp_(0, 1)

    def timed_torch(fn):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        a.record()
        fn()
        b.record()
        torch.cuda.synchronize()
        return a.elapsed_time(b)

    torch_ms = {}

    def route_a():
        torch_ms["a"] = timed_torch(narrow)
        det.pyramid_yuv(narrowed, n, dnv)

    def route_b():
        torch_ms["b"] = timed_torch(to_float)
        det.pyramid_tensor(rgbf, layout="nhwc")

    sides = {
        "p010 fused": (det, lambda: det.pyramid_video(p010, n, d010, f10), ["k_ingest_yuv16_pairs"], None),
        "p010 narrowed to nv12 (a)": (det, route_a, ["k_ingest_yuv420"], "a"),
        "p010 to float rgb (b)": (det, route_b, ["k_ingest_image"], "b"),
        "planar16": (det, lambda: det.pyramid_video(planar, n, dpl, f10p), ["k_ingest_yuv16_planar"], None),
        "generic16 (base + 2)": (det, lambda: det.pyramid_video(shifted.data_ptr() + 2, n, dpl, f10p), ["k_ingest_yuv16_generic"], None),
        "nv12 default": (det, lambda: det.pyramid_yuv(nv12, n, dnv), ["k_ingest_yuv420"], None),
        "nv12 bt709": (det, lambda: det.pyramid_video(nv12, n, dnv, f709), ["k_ingest_yuv420"], None),
        "i420 default": (det, lambda: det.pyramid_yuv(i420, n, d420), ["k_ingest_yuv_planar"], None),
    }
    if parent is not None:
        sides["parent: nv12 default"] = (parent, lambda: parent.pyramid_yuv(nv12, n, dnv), ["k_ingest_yuv420"], None)
        sides["parent: i420 default"] = (parent, lambda: parent.pyramid_yuv(i420, n, d420), ["k_ingest_yuv_planar"], None)
        sides["second context: nv12 default"] = (det2, lambda: det2.pyramid_yuv(nv12, n, dnv), ["k_ingest_yuv420"], None)
        sides["second context: i420 default"] = (det2, lambda: det2.pyramid_yuv(i420, n, d420), ["k_ingest_yuv_planar"], None)
        sides["parent, second context: nv12 default"] = (parent2, lambda: parent2.pyramid_yuv(nv12, n, dnv), ["k_ingest_yuv420"], None)
        sides["parent, second context: i420 default"] = (parent2, lambda: parent2.pyramid_yuv(i420, n, d420), ["k_ingest_yuv_planar"], None)
    level0 = {}
    ms = {k: {name: [] for name in kernels + (["torch"] if tk else [])} for k, (_, _, kernels, tk) in sides.items()}
    for r in range(WARM + args.rounds):
        for what, (d, fn, kernels, tk) in sides.items():
            d.profile()
            fn()
            d.synchronize()
            p = d.profile()
            if r == 0:
                level0[what] = d.read_level(n - 1, 0).tobytes()
            if r >= WARM:
                for name in kernels:
                    ms[what][name].append(p[name][0] / p[name][1])
                if tk:
                    ms[what]["torch"].append(torch_ms[tk])
    for d in (det, parent, det2, parent2):
        if d is not None:
            d.close()

    def stats(v):
        v = np.array(v)
        return {"median_ms": float(np.median(v)), "min_ms": float(v.min()), "max_ms": float(v.max())}
    res = {"lib": os.path.basename(capi.LIB_PATH), "parent_lib": os.path.basename(args.parent_lib), "frames": n, "size": [h, w], "rounds": args.rounds,
           "kernel_ms_per_call": {}}
    for what, per in ms.items():
        res["kernel_ms_per_call"][what] = {name: stats(v) for name, v in per.items()}
        if len(per) > 1:
            res["kernel_ms_per_call"][what]["sum"] = stats(np.sum([per[name] for name in per], axis=0))
    res["same_first_level"] = {"p010 fused == planar16 == generic16": level0["p010 fused"] == level0["planar16"] == level0["generic16 (base + 2)"],
                               "nv12 default == i420 default": level0["nv12 default"] == level0["i420 default"],
                               "nv12 bt709 != nv12 default (another matrix)": level0["nv12 bt709"] != level0["nv12 default"]}
    if parent is not None:
        res["same_first_level"]["parent == this build, nv12 and i420"] = (level0["parent: nv12 default"] == level0["nv12 default"] and
                                                                            level0["parent: i420 default"] == level0["i420 default"])
    px = n * h * w
    res["bytes_per_call"] = {"p010 / planar16 fused": px * 3 + px * 12, "nv12 / i420": px * 1.5 + px * 12}
    print(json.dumps(res))


if __name__ == "__main__":
    main()
