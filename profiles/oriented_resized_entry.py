"""The oriented resized YUV entry's kernel against the chain a caller had to run before it (profiles/oriented_resized_entry.md):
FACE80, 2048 trees, colorSpace luv on RGB input, 3840 x 2160 I420 frames AS STORED, 32 per call, option "profile" (a kernel's time =
the span between its marker and the next one on the stream), scales 0.5 and resize_scale(80, 150), orientation codes 1 (a quarter
turn) and 4 (mirror).  On the same frames, alternating in one process:
  (a) fused    pyramid_yuv_resized(I420, orient=code)                      k_ingest_oriented_resized_yuv (or _generic: see below)
  (b) chain    yuv_to_rgb8, torch rot90 / flip(...).contiguous() of the packed image (torch events), pyramid_u8(RGB) under
               set_input_resize at the upright size                        k_yuv_to_rgb8 + torch + k_resize_u8 + k_ingest_u8
  (c) upright  pyramid_yuv_resized(I420) on the same bytes taken as upright frames: today's k_ingest_resized_yuv (no bar: another image)
Two warm-up rounds, then `rounds` rounds; medians with the spread of the rounds; the first pyramid level of (a) and (b) compared byte
for byte before any time counts.  The form of (a) is the library's choice; run the program again under
ACF_HIP_FORCE_FALLBACK=oriented_resized_generic (read once per process) for the generic form.
  python profiles/oriented_resized_entry.py [--frames 32] [--rounds 10]
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
    d420, fb420 = HipDetector.yuv_desc("i420", h, w)
    assert fb420 == i420.shape[1]
    rgb = torch.empty((n, h, w, 3), dtype=torch.uint8, device="cuda")             # the chain's first intermediate
    tiny = torch.empty((2, 2, 3), dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()

    res = {"lib": os.path.basename(capi.LIB_PATH), "forced": os.environ.get("ACF_HIP_FORCE_FALLBACK", ""), "frames": n, "stored": [h, w],
           "rounds": args.rounds, "runs": {}}
    for tag, scale in (("0.5", 0.5), ("resize_scale(80, 150)", HipDetector.resize_scale(80, 150))):
        for code in (1, 4):
            uh, uw = HipDetector.oriented_dims(h, w, code)
            dr, dc = HipDetector.oriented_resized_dims(h, w, code, scale)
            ur, uc = HipDetector.resize_dims(h, w, scale)
            fused, chain, upright = HipDetector(), HipDetector(), HipDetector()
            for det, (pr, pc) in ((fused, (dr, dc)), (chain, (dr, dc)), (upright, (ur, uc))):
                det.set_option("profile", 1)
                det.set_model(model)
                det.plan(pr, pc, 3, n, 1 << 15)
            chain.set_input_resize(uh, uw, scale)
            ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
            turn_ms, conv_ms = [], []
            rot, mirror = code & 3, code >> 2

            def chain_b():
                # the conversion in a profile window of its own, closed by the marker of a second, 2 x 2 conversion right behind it: a
                # span ends at the NEXT marker on the stream, which must not be the one behind the host's wait and torch's turn
                chain._chk(chain.lib.acf_hip_yuv_to_rgb8(chain.ctx, C.c_void_p(i420.data_ptr()), n, h, w, C.byref(d420), C.c_void_p(rgb.data_ptr())))
                chain._chk(chain.lib.acf_hip_yuv_to_rgb8(chain.ctx, C.c_void_p(i420.data_ptr()), 1, 2, 2, C.byref(d420), C.c_void_p(tiny.data_ptr())))
                chain.synchronize()                                                # (the context's stream, then torch's)
                p = chain.profile()
                assert p["k_yuv_to_rgb8"][1] == 1
                conv_ms.append(p["k_yuv_to_rgb8"][0])
                ev[0].record()
                t = rgb.flip(2) if mirror else rgb
                t = torch.rot90(t, k=-rot, dims=(1, 2)).contiguous()
                ev[1].record()
                torch.cuda.synchronize()
                turn_ms.append(ev[0].elapsed_time(ev[1]))
                assert tuple(t.shape) == (n, uh, uw, 3)
                chain.pyramid_u8(t, capi.PIX_RGB)
                chain.synchronize()

            sides = {
                "(a) fused": (fused, lambda: fused.pyramid_yuv_resized(i420, n, d420, h, w, scale, code), None),
                "(b) chain": (chain, chain_b, ["k_resize_u8", "k_ingest_u8"]),
                "(c) upright resized": (upright, lambda: upright.pyramid_yuv_resized(i420, n, d420, h, w, scale), ["k_ingest_resized_yuv"]),
            }
            level0 = {}
            ms = {k: {} for k in sides}
            for r in range(WARM + args.rounds):
                for what, (det, fn, kernels) in sides.items():
                    det.profile()
                    fn()
                    det.synchronize()
                    p = det.profile()
                    if kernels is None:
                        kernels = [k for k in p if k.startswith("k_ingest_oriented_resized")]
                        assert len(kernels) == 1, sorted(p)
                    if r == 0:
                        level0[what] = det.read_level(n - 1, 0).tobytes()
                        if what == "(b) chain":
                            assert level0["(a) fused"] == level0["(b) chain"], "the fused entry and the chain leave different first levels"
                    if r >= WARM:
                        for name in kernels:
                            ms[what].setdefault(name, []).append(p[name][0] / p[name][1])
            for det in (fused, chain, upright):
                det.close()
            out = {"upright": [uh, uw], "reduced": [dr, dc], "kernel_ms_per_call": {}}
            for what, per in ms.items():
                out["kernel_ms_per_call"][what] = {name: stats(v) for name, v in per.items()}
            kern = np.sum([ms["(b) chain"][k] for k in ("k_resize_u8", "k_ingest_u8")], axis=0) + np.array(conv_ms[WARM:])
            out["kernel_ms_per_call"]["(b) chain"]["k_yuv_to_rgb8"] = stats(conv_ms[WARM:])
            out["kernel_ms_per_call"]["(b) chain"]["torch rot90 / flip"] = stats(turn_ms[WARM:])
            out["kernel_ms_per_call"]["(b) chain"]["sum"] = stats(kern + np.array(turn_ms[WARM:]))
            out["same_first_level (a) == (b)"] = level0["(a) fused"] == level0["(b) chain"]
            (fname, a), = out["kernel_ms_per_call"]["(a) fused"].items()
            b = out["kernel_ms_per_call"]["(b) chain"]["sum"]
            out["fused median below the chain's whole range"] = a["median_ms"] < b["min_ms"]
            src, red = n * h * w, n * dr * dc
            out["GB_per_s (a)"] = (src * 1.5 + red * 12) / a["median_ms"] / 1e6
            res["runs"]["%s, code %d" % (tag, code)] = out
    print(json.dumps(res))


if __name__ == "__main__":
    main()
