"""Every kind of input on ONE context, in turn, forwards and then backwards: each call must leave exactly what a fresh context leaves
for that call alone — the pyramid and the raw detections of both frames, bit for bit.  This is independence from history (the
resized entries' tap tables, the planar staging buffer, the NV12 conversion buffer and its growth, the input resize's switch, the
destination the ingest chooses), not correctness: the per-entry suites hold every entry against the reference.

Once with a model whose colour conversion the ingest does itself (LUV), once with one it stages planar for (HSV)."""
import numpy as np
import pytest

import resized_entry_case as rc
import yuv_desc_ref as ydr
from acf_amd import capi, synth

pytestmark = pytest.mark.gpu

PH, PW = 96, 128                  # the plan
SH, SW, SCALE = 192, 256, 0.5     # the unreduced frames of the resized kinds
NF = 2


def dev(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def steps():
    """[(name, call(det))]: the device buffers are made once and shared by the fresh contexts and the sequence."""
    import torch
    from acf_amd.detector import HipDetector
    assert HipDetector.resize_dims(SH, SW, SCALE) == (PH, PW)
    f32 = dev(np.stack([synth.make_frame(11 + f, PH, PW, "rgb") for f in range(NF)]))
    rgb = dev(np.stack([rc.rgb_u8(21 + f, PH, PW) for f in range(NF)]))
    nv12 = dev(np.concatenate([ydr.pack("nv12", *rc.yuv_planes(31 + f, PH, PW, 1, 1)) for f in range(NF)]))
    f16 = dev(np.stack([rc.rgb_u8(41 + f, PH, PW) for f in range(NF)])).permute(0, 3, 1, 2).contiguous().to(torch.float16) / 255
    i420 = dev(np.concatenate([ydr.pack("i420", *rc.yuv_planes(51 + f, PH, PW, 1, 1)) for f in range(NF)]))
    nv12b = dev(np.concatenate([ydr.pack("nv12", *rc.yuv_planes(61 + f, PH, PW, 1, 1)) for f in range(NF)]))
    i420S = dev(np.concatenate([ydr.pack("i420", *rc.yuv_planes(71 + f, SH, SW, 1, 1)) for f in range(NF)]))
    nchwS = dev(np.stack([rc.rgb_u8(81 + f, SH, SW) for f in range(NF)]).transpose(0, 3, 1, 2))
    rgbS = dev(np.stack([rc.rgb_u8(91 + f, SH, SW) for f in range(NF)]))
    d_i420, _ = HipDetector.yuv_desc("i420", PH, PW)
    d_nv12, _ = HipDetector.yuv_desc("nv12", PH, PW)
    d_i420S, _ = HipDetector.yuv_desc("i420", SH, SW)

    def resized_u8(det):
        det.set_input_resize(SH, SW, SCALE)
        try:
            det.run_u8(rgbS, capi.PIX_RGB, 0, n=NF)
        finally:
            det.set_input_resize(0, 0, 1.0)
    return [
        ("run_f32", lambda det: det.run(f32, NF)),
        ("run_u8_rgb", lambda det: det.run_u8(rgb, capi.PIX_RGB, 0, n=NF)),
        ("run_u8_nv12", lambda det: det.run_u8(nv12, capi.PIX_NV12, 0, n=NF)),
        ("run_tensor_f16", lambda det: det.run_tensor(f16)),
        ("run_yuv_i420", lambda det: det.run_yuv(i420, NF, d_i420)),
        ("run_yuv_nv12_description", lambda det: det.run_yuv(nv12b, NF, d_nv12)),
        ("run_yuv_resized_i420", lambda det: det.run_yuv_resized(i420S, NF, d_i420S, SH, SW, SCALE)),
        ("run_tensor_resized", lambda det: det.run_tensor_resized(nchwS, SCALE)),
        ("input_resize_run_u8", resized_u8),
    ]


def snapshot(det):
    return [(det.read_pyramid(f).view(np.uint32).copy(), det.raw_detections(f).tobytes()) for f in range(NF)]


@pytest.mark.parametrize("space", ["luv", "hsv"])
def test_each_kind_leaves_what_a_fresh_context_leaves(space):
    from acf_amd.detector import HipDetector
    over = dict(isLuv=0) if space == "luv" else dict(isLuv=0, colorSpace=capi.CS_HSV)   # luv: the ingest converts; hsv: it stages planar
    model = synth.make_model(seed=3, name="TINY", nTrees=16, **over)

    def fresh():
        return HipDetector(model, PH, PW, 3, max_batch=NF, max_hits=1 << 15)
    seq = steps()
    want = {}
    for name, call in seq:
        det = fresh()
        call(det)
        want[name] = snapshot(det)
        det.close()
    assert sum(len(d) for snap in want.values() for _, d in snap) > 0
    assert len({snap[0][0].tobytes() for snap in want.values()}) == len(seq), "every step has frames of its own"
    det = fresh()
    for name, call in seq + seq[::-1]:
        call(det)
        for f, ((gp, gd), (wp, wd)) in enumerate(zip(snapshot(det), want[name])):
            assert np.array_equal(gp, wp), (space, name, f, "pyramid")
            assert gd == wd, (space, name, f, "detections")
    det.close()


def test_the_specific_and_the_general_entry_of_a_call_are_one():
    """Every general combination through its most specific entry and through the most general one, on one context per plan size: the
    raw detections of both frames bit for bit, and the same kernel names in the profile.  (Called by their C names: a row says which
    entry it enters.)"""
    import ctypes as C

    from acf_amd.detector import HipDetector, PinnedBuffer
    model = synth.make_model(seed=3, name="TINY", nTrees=16, isLuv=0, cascThr=-10.0)   # (no window is rejected: every score is compared)
    i420 =np.concatenate([ydr.pack("i420", *rc.yuv_planes(51 + f, PH, PW, 1, 1)) for f in range(NF)])
    i420S = dev(np.concatenate([ydr.pack("i420", *rc.yuv_planes(71 + f, SH, SW, 1, 1)) for f in range(NF)]))
    rgb = dev(np.stack([rc.rgb_u8(21 + f, PH, PW) for f in range(NF)]))
    rgbS = dev(np.stack([rc.rgb_u8(91 + f, SH, SW) for f in range(NF)]))
    x = dev(i420)
    d, fb = HipDetector.yuv_desc("i420", PH, PW)
    dS, _ = HipDetector.yuv_desc("i420", SH, SW)
    img = capi.ImageDesc(capi.T_U8, 3, PH * PW * 3, 1, PW * 3, 3)
    imgS = capi.ImageDesc(capi.T_U8, 3, SH * SW * 3, 1, SW * 3, 3)
    P = lambda t: C.c_void_p(t.data_ptr())
    upright = HipDetector(model, PH, PW, 3, max_batch=NF, max_hits=1 << 15)
    turned = HipDetector(model, PW, PH, 3, max_batch=NF, max_hits=1 << 15)     # the plan of the quarter turns
    assert HipDetector.oriented_resized_dims(SH, SW, 1, SCALE) == (PW, PH)
    for det in (upright, turned):
        det.set_option("profile", 1)

    def call(det, fn, *args):
        det.profile()
        det._chk(getattr(det.lib, "acf_hip_" + fn)(det.ctx, *args))
        return [det.raw_detections(f).tobytes() for f in range(NF)], sorted(det.profile())

    # (context, [the calls that are one call])
    groups = [
        (upright, [("run_yuv", P(x), NF, C.byref(d)), ("run_video", P(x), NF, C.byref(d), None, 0, 0, 0, 0.0),
                   ("run_yuv_oriented", P(x), NF, C.byref(d), PH, PW, 0), ("run_video", P(x), NF, C.byref(d), None, PH, PW, 0, 0.0)]),
        (upright, [("run_yuv_resized", P(i420S), NF, C.byref(dS), SH, SW, SCALE), ("run_yuv_oriented_resized", P(i420S), NF, C.byref(dS), SH, SW, 0, SCALE),
                   ("run_video", P(i420S), NF, C.byref(dS), None, SH, SW, 0, SCALE)]),
        (upright, [("run_yuv_oriented", P(x), NF, C.byref(d), PH, PW, 2), ("run_video", P(x), NF, C.byref(d), None, PH, PW, 2, 0.0)]),
        (upright, [("run_yuv_oriented_resized", P(i420S), NF, C.byref(dS), SH, SW, 6, SCALE), ("run_video", P(i420S), NF, C.byref(dS), None, SH, SW, 6, SCALE)]),
        (turned, [("run_yuv_oriented", P(x), NF, C.byref(d), PH, PW, 1), ("run_video", P(x), NF, C.byref(d), None, PH, PW, 1, 0.0)]),
        (turned, [("run_yuv_oriented_resized", P(i420S), NF, C.byref(dS), SH, SW, 1, SCALE), ("run_video", P(i420S), NF, C.byref(dS), None, SH, SW, 1, SCALE)]),
        (upright, [("run_image", P(rgb), NF, C.byref(img)), ("run_image_oriented", P(rgb), NF, C.byref(img), PH, PW, 0)]),
        (upright, [("run_image_resized", P(rgbS), NF, C.byref(imgS), SH, SW, SCALE), ("run_image_oriented_resized", P(rgbS), NF, C.byref(imgS), SH, SW, 0, SCALE)]),
    ]
    seen = set()
    for det, calls in groups:
        want = call(det, *calls[0])
        assert sum(len(b) for b in want[0]) > 0 and any(n.startswith("k_ingest_") for n in want[1]), calls[0][0]
        seen.add(tuple(want[0]))
        for other in calls[1:]:
            assert call(det, *other) == want, (calls[0][0], other[0])
    assert len(seen) == len(groups), "every group has frames or a geometry of its own"
    # the streams: stream_open_yuv against stream_open_video with the default format, then with no format at all
    cap, got = 256, []
    pin = PinnedBuffer(NF * fb)
    pin.array[:i420.size] = i420
    default = capi.YuvFormat(8, 0, capi.YUV_MATRIX_BT601, 0)
    for fn, args in (("stream_open_yuv", (C.byref(d), fb, cap, 2)), ("stream_open_video", (C.byref(d), C.byref(default), fb, 0, 0, 0, 0.0, cap, 2)),
                     ("stream_open_video", (C.byref(d), None, fb, 0, 0, 0, 0.0, cap, 2))):
        upright._chk(getattr(upright.lib, "acf_hip_" + fn)(upright.ctx, *args))
        upright._stream_cap = cap
        upright.profile()
        rec = upright.stream_collect(upright.stream_submit(pin.ptr.value, NF))
        got.append((rec.tobytes(), sorted(upright.profile())))
        upright.stream_close()
    assert int(np.frombuffer(got[0][0], np.int32).reshape(NF, -1)[:, 0].sum()) > 0
    assert got[1] == got[0] and got[2] == got[0]
    pin.close()
    upright.close()
    turned.close()
