"""The resized tensor and YUV entries on the GPU (include/acf_hip.h: acf_hip_pyramid_yuv_resized / run_yuv_resized /
pyramid_image_resized / run_image_resized / stream_open_yuv_resized; kernel k_ingest_resized).

Two references, both equalities of bytes or of uint32 views:
  the oracle chain    numpy gather / convert (tests/yuv_desc_ref.py) -> oracle.resize_u8 -> acfo_ingest_u8 -> chnsPyramid -> acfDetect
                      (tests/resized_entry_case.py: expected), the boxes back by oracle.unscale_rect
  the device chain    the existing entries composed: yuv_to_rgb8 (or a torch repack to packed bytes) into a second context with
                      set_input_resize + run_u8
tests/test_resized_entries.py holds the precondition that every case detects something.
"""
import ctypes as C
import os
import sys

import numpy as np
import pytest

import resized_entry_case as rc
from acf_amd import capi, synth

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

OLD_KERNELS = ("k_yuv_to_rgb8", "k_yuv420_to_rgb8", "k_resize_u8", "k_ingest_u8", "k_ingest_image")   # and every k_ingest_yuv*


def bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def dev(buf):
    import torch
    return torch.from_numpy(np.ascontiguousarray(buf)).cuda()


def snapshot(det, nF):
    """Per frame (levels, detections bytes, hits bytes) of the last run."""
    out = []
    for f in range(nF):
        d, h = det.detections(f)
        out.append(([bits(det.read_level(f, i)) for i in range(len(det.levels))], d.tobytes(), h.tobytes()))
    return out


def same(got, want, tag):
    assert len(got) == len(want), tag
    for f, ((gl, gd, gh), (wl, wd, wh)) in enumerate(zip(got, want)):
        assert len(gl) == len(wl), (tag, f)
        for i, (a, b) in enumerate(zip(gl, wl)):
            assert np.array_equal(a, b), (tag, f, "level", i)
        assert gd == wd and gh == wh, (tag, f)


def detector(case, arith=0, oracle=None, **kw):
    from acf_amd.detector import HipDetector
    name, H, W, dr, dc, scale, form, inp, model, d_in = case
    det = HipDetector(synth.make_model(**model), dr, dc, d_in, max_batch=rc.NF, max_hits=1 << 17, **kw)
    if arith:
        det.set_x86_tables(*oracle.x86_fixture())
        det.set_option("arith", 1)
    return det


def run_entry(det, case, x, pyramid_only=False):
    """The case's frames (x: the device copy of built(case).buf) through the resized entry, by the Python method a caller would use."""
    name, H, W, dr, dc, scale, form, inp, model, d_in = case
    b = rc.built(case)
    if inp == "three_planes":
        y, u, v = (x[at:at + int(np.prod(shape))].view(shape) for at, shape in b.planes)
        base, n, d = det.yuv_planes_desc(y, u, v, 1, 1)
        assert n == rc.NF and bytes(d) == bytes(b.desc), "run_yuv_planes describes the arena as the case does"
        if not pyramid_only:
            return det.run_yuv_planes(y, u, v, 1, 1, scale=scale)
    if b.kind == "yuv":
        fn = det.pyramid_yuv_resized if pyramid_only else det.run_yuv_resized
        return fn(x.data_ptr() + b.base, rc.NF, b.desc, H, W, scale)
    if inp in ("nchw", "gray"):
        fn = det.pyramid_tensor_resized if pyramid_only else det.run_tensor_resized
        return fn(x.view(b.shape), scale)
    if inp == "rgba":
        fn = det.pyramid_tensor_resized if pyramid_only else det.run_tensor_resized
        return fn(x.view(rc.NF, H, W, 4)[..., :3], scale, layout="nhwc")
    fn = det.pyramid_image_resized if pyramid_only else det.run_image_resized      # bgr: a negative channel stride, no torch view
    return fn(x.data_ptr() + b.base, rc.NF, b.desc, H, W, scale)


def packed_on_device(det, case, x):
    """What the chain of existing entries starts from, made on the device: yuv_to_rgb8, or a torch repack of the tensor."""
    name, H, W, dr, dc, scale, form, inp, model, d_in = case
    b = rc.built(case)
    if b.kind == "yuv":
        return det.yuv_to_rgb8(x.data_ptr() + b.base, rc.NF, H, W, b.desc)
    if inp == "nchw":
        return x.view(b.shape).permute(0, 2, 3, 1).contiguous()
    if inp == "gray":
        return x.view(rc.NF, H, W, 1)
    if inp == "bgr":
        return x.view(rc.NF, H, W, 3).flip(-1).contiguous()
    return x.view(rc.NF, H, W, 4)[..., :3].contiguous()


def chain_expect(case, x, src, arith=0, oracle=None):
    """snapshot of set_input_resize + run_u8 on a second context, on the packed bytes."""
    name, H, W, dr, dc, scale, form, inp, model, d_in = case
    b = rc.built(case)
    ref = detector(case, arith, oracle)
    ref.set_input_resize(H, W, scale)
    packed = packed_on_device(src, case, x)
    assert np.array_equal(packed.cpu().numpy(), b.packed), "the device's packed bytes are the restatement's"
    ref.run_u8(packed, b.pix, 0, n=rc.NF)
    want = snapshot(ref, rc.NF)
    ref.close()
    return want


# ---------------------------------------------------------------- 1. the oracle chain; 3. what ran

@pytest.mark.parametrize("case", rc.CASES, ids=rc.IDS)
def test_resized_entry_equals_the_oracle_chain(oracle, case):
    from acf_amd.detector import HipDetector
    name, H, W, dr, dc, scale, form, inp, model, d_in = case
    b = rc.built(case)
    plan, want = rc.expected(oracle, case)
    det = detector(case)
    x = dev(b.buf)
    det.set_option("profile", 1)
    det.profile()
    run_entry(det, case, x)
    names = set(det.profile())
    det.set_option("profile", 0)
    mine = "k_ingest_resized_yuv" if b.kind == "yuv" else "k_ingest_resized_image"
    assert mine in names, names
    assert not [n for n in names if n in OLD_KERNELS or n.startswith("k_ingest_yuv") or (n.startswith("k_ingest_resized") and n != mine)], names
    if model.get("colorSpace") == capi.CS_HSV:
        assert "k_colour" in names, names                                                  # planar to d_stage, then k_rgb2hsv
    total = 0
    for f, (pyr, wdet, whits) in enumerate(want):
        assert np.array_equal(bits(det.read_pyramid(f)), bits(pyr)), (name, f)            # every level, bit for bit
        got, hits = det.detections(f)
        assert got.tobytes() == wdet.tobytes() and hits.tobytes() == whits.tobytes(), (name, f, len(got), len(wdet))
        back = HipDetector.unscale_boxes(got, scale)
        for g, w_ in zip(back, wdet):
            assert [int(g["x"]), int(g["y"]), int(g["w"]), int(g["h"])] == oracle.unscale_rect(scale, [w_["x"], w_["y"], w_["w"], w_["h"]])
        total += len(wdet)
    assert total > 0
    det.close()


# ---------------------------------------------------------------- 2. the device chain of existing entries

@pytest.mark.parametrize("case", rc.CASES, ids=rc.IDS)
def test_resized_entry_equals_the_chain_of_existing_entries(case):
    b = rc.built(case)
    det = detector(case)
    x = dev(b.buf)
    want = chain_expect(case, x, det)
    run_entry(det, case, x)
    same(snapshot(det, rc.NF), want, case[0])
    assert sum(len(w[1]) for w in want) > 0
    # the pyramid entry alone leaves the same levels
    run_entry(det, case, x, pyramid_only=True)
    det.synchronize()
    for f in range(rc.NF):
        for i in range(len(det.levels)):
            assert np.array_equal(bits(det.read_level(f, i)), want[f][0][i]), (case[0], f, i)
    det.close()


@pytest.mark.parametrize("name", ["yuyv_padded_half", "nchw_area_frac"])
def test_reference_arithmetic_equals_the_chain(oracle, name):
    """Option "arith" = 1 (rgb2luv_sse's reciprocal as one x86 CPU gives it): against the device chain, and against the oracle."""
    case = rc.CASES[rc.IDS.index(name)]
    b = rc.built(case)
    det = detector(case, 1, oracle)
    x = dev(b.buf)
    want = chain_expect(case, x, det, 1, oracle)
    run_entry(det, case, x)
    got = snapshot(det, rc.NF)
    same(got, want, name)
    plan, exp = rc.expected(oracle, case, arith=1)
    _, plain = rc.expected(oracle, case)
    assert any(not np.array_equal(bits(a[0]), bits(p[0])) for a, p in zip(exp, plain)), "the tables change no bit: the case checks nothing"
    for f, (pyr, wdet, whits) in enumerate(exp):
        assert np.array_equal(bits(det.read_pyramid(f)), bits(pyr)), (name, f)
        assert got[f][1] == wdet.tobytes() and got[f][2] == whits.tobytes(), (name, f)
    det.close()


# ---------------------------------------------------------------- 4. the table cache

def test_tap_tables_are_kept_by_key_and_dropped_by_a_plan():
    from acf_amd.detector import HipDetector, HipError
    case = rc.CASES[rc.IDS.index("yuyv_padded_half")]
    name, H, W, dr, dc, scale, form, inp, model, d_in = case
    b = rc.built(case)
    det = detector(case)
    xa = dev(b.buf)
    # a second key with the same reduced size: 360 x 480 I420 frames at 1 / 3
    H2, W2, s2 = 360, 480, 1.0 / 3.0
    assert HipDetector.resize_dims(H2, W2, s2) == (dr, dc)
    d2, fb2 = HipDetector.yuv_desc("i420", H2, W2)
    import yuv_desc_ref as ydr
    xb = dev(np.concatenate([ydr.pack("i420", *rc.yuv_planes(90 + f, H2, W2, 1, 1)) for f in range(rc.NF)]))

    def run_a():
        det.run_yuv_resized(xa, rc.NF, b.desc, H, W, scale)
        return snapshot(det, rc.NF)

    def run_b():
        det.run_yuv_resized(xb, rc.NF, d2, H2, W2, s2)
        return snapshot(det, rc.NF)
    a0 = run_a()
    same(run_a(), a0, "the same key again")
    b0 = run_b()
    assert any(not np.array_equal(p, q) for p, q in zip(a0[0][0], b0[0][0]))
    for _ in range(2):
        same(run_a(), a0, "key A after key B")
        same(run_b(), b0, "key B after key A")
    # a plan drops them: the same plan again gives the same bits from rebuilt tables; a plan of another size refuses the old key
    det.plan(dr, dc, d_in, rc.NF, 1 << 17)
    same(run_b(), b0, "after acf_hip_plan")
    det.plan(dr + 4, dc, d_in, rc.NF, 1 << 17)
    with pytest.raises(HipError) as e:
        run_b()
    assert e.value.code == capi.E_INVALID
    det.close()


# ---------------------------------------------------------------- 5. streaming

def test_stream_of_unreduced_i420_frames_matches_blocking_calls():
    """Four I420 batches (one short) from pinned memory at depth 2 give the records of run_yuv_resized + export of each batch."""
    import torch
    import yuv_desc_ref as ydr
    from acf_amd.detector import HipDetector, PinnedBuffer
    case = rc.CASES[rc.IDS.index("i420_area_frac")]
    name, H, W, dr, dc, scale, form, inp, model, d_in = case
    cap, nB, depth = 512, 3, 2
    det = HipDetector(synth.make_model(**model), dr, dc, 3, max_batch=nB, max_hits=1 << 16)
    d, fb = HipDetector.yuv_desc("i420", H, W)
    batches = [np.stack([ydr.pack("i420", *rc.yuv_planes(100 + 10 * k + i, H, W, 1, 1)) for i in range(nB if k != 2 else 1)]) for k in range(4)]
    want = []
    for x in batches:
        xd = dev(x)                                                       # (alive until the synchronise: the call is asynchronous)
        det.run_yuv_resized(xd, x.shape[0], d, H, W, scale)
        dst = torch.zeros((x.shape[0], 1 + 6 * cap), dtype=torch.int32, device="cuda")
        torch.cuda.synchronize()                                          # (torch fills dst on its own stream: before the export writes it)
        det.export_detections(dst, cap)
        det.synchronize()
        want.append(dst.cpu().numpy())
    assert sum(int(x[:, 0].sum()) for x in want) > 0
    pins = [PinnedBuffer(nB * fb) for _ in range(depth)]
    det.stream_open_yuv_resized(d, fb, H, W, scale, cap, depth)
    got, inflight = [], []
    for k, x in enumerate(batches):
        if len(inflight) == depth:
            got.append(det.stream_collect(inflight.pop(0)))
        pin = pins[k % depth]
        pin.array[:x.size] = x.ravel()
        inflight.append(det.stream_submit(pin.ptr.value, x.shape[0]))
    while inflight:
        got.append(det.stream_collect(inflight.pop(0)))
    for k in range(4):
        assert got[k].shape == want[k].shape, k
        for f in range(want[k].shape[0]):
            n = want[k][f, 0]
            assert got[k][f, 0] == n
            assert np.array_equal(got[k][f, :1 + 6 * n], want[k][f, :1 + 6 * n]), (k, f)
    det.stream_close()
    det.close()
    for p in pins:
        p.close()


# ---------------------------------------------------------------- 6. what is refused

def test_resized_entries_argument_checks():
    import torch
    from acf_amd.detector import HipDetector, HipError
    model = synth.make_model(seed=3, name="TINY", nTrees=16)
    H, W, scale = 192, 256, 0.5
    h, w = HipDetector.resize_dims(H, W, scale)
    x = torch.zeros(4 * H * W * 4, dtype=torch.uint8).cuda()              # room for every call below, were it not refused
    good, fb = HipDetector.yuv_desc("i420", H, W)
    img = capi.ImageDesc(capi.T_U8, 3, 3 * H * W, H * W, W, 1)
    ptr = x.data_ptr()

    def refused(fn, code=capi.E_INVALID):
        with pytest.raises(HipError) as e:
            fn()
        assert e.value.code == code, e.value

    def variant(**kw):
        d = capi.YuvDesc.from_buffer_copy(good)
        for k, v in kw.items():
            plane, _, field = k.partition("_")
            if plane in ("y", "u", "v"):
                setattr(getattr(d, plane), field, v)
            else:
                setattr(d, k, v)
        return d

    def image(**kw):
        d = capi.ImageDesc.from_buffer_copy(img)
        for k, v in kw.items():
            setattr(d, k, v)
        return d
    det = HipDetector(model, h, w, 3, max_batch=2)
    lib = det.lib
    det.run_yuv_resized(x, 2, good, H, W, scale)                         # accepted as they are
    det.run_image_resized(ptr, 2, img, H, W, scale)
    det.stream_open_yuv_resized(good, fb, H, W, scale, 64, 2)
    det.stream_close()
    # what the un-resized entries refuse
    sc = C.c_double(scale)
    assert lib.acf_hip_run_yuv_resized(det.ctx, None, 1, C.byref(good), H, W, sc) == capi.E_INVALID
    assert lib.acf_hip_run_yuv_resized(det.ctx, C.c_void_p(ptr), 1, None, H, W, sc) == capi.E_INVALID
    assert lib.acf_hip_pyramid_yuv_resized(None, C.c_void_p(ptr), 1, C.byref(good), H, W, sc) == capi.E_INVALID
    assert lib.acf_hip_run_image_resized(det.ctx, None, 1, C.byref(img), H, W, sc) == capi.E_INVALID
    assert lib.acf_hip_run_image_resized(det.ctx, C.c_void_p(ptr), 1, None, H, W, sc) == capi.E_INVALID
    assert lib.acf_hip_pyramid_image_resized(None, C.c_void_p(ptr), 1, C.byref(img), H, W, sc) == capi.E_INVALID
    assert lib.acf_hip_stream_open_yuv_resized(det.ctx, None, fb, H, W, sc, 64, 2) == capi.E_INVALID
    for n in (0, 3):                                                      # max_batch is 2
        refused(lambda: det.run_yuv_resized(x, n, good, H, W, scale))
        refused(lambda: det.run_image_resized(ptr, n, img, H, W, scale))
    for bad in (variant(sub_x=2), variant(sub_y=-1), variant(y_stride_px=0), variant(u_stride_row=0), variant(v_stride_n=-4), variant(u_stride_px=-1)):
        refused(lambda: det.run_yuv_resized(x, 1, bad, H, W, scale))
        refused(lambda: det.pyramid_yuv_resized(x, 1, bad, H, W, scale))
        refused(lambda: det.stream_open_yuv_resized(bad, fb, H, W, scale, 64, 2))
    for bad in (image(dtype=7), image(dtype=-1), image(channels=2), image(channels=1), image(stride_x=0), image(stride_y=-3), image(stride_n=-1)):
        refused(lambda: det.run_image_resized(ptr, 1, bad, H, W, scale))
        refused(lambda: det.pyramid_image_resized(ptr, 1, bad, H, W, scale))
    # the source size, the scale, a plan of other dimensions
    for rows, cols, s in ((0, W, scale), (H, 0, scale), (-H, W, scale), (H, W, 0.0), (H, W, -0.5), (H, W, float("nan")), (H, W, float("inf")),
                          (H + 2, W, scale), (H, W, 0.75), (H, W, 1.0)):
        refused(lambda: det.run_yuv_resized(x, 1, good, rows, cols, s))
        refused(lambda: det.pyramid_yuv_resized(x, 1, good, rows, cols, s))
        refused(lambda: det.run_image_resized(ptr, 1, img, rows, cols, s))
        refused(lambda: det.pyramid_image_resized(ptr, 1, img, rows, cols, s))
        refused(lambda: det.stream_open_yuv_resized(good, fb, rows, cols, s, 64, 2))
    # float images: cv::resize's CV_32F arithmetic is not restated
    for dt in (capi.T_F16, capi.T_BF16, capi.T_F32):
        refused(lambda: det.run_image_resized(ptr, 1, image(dtype=dt), H, W, scale), capi.E_UNSUPPORTED)
        refused(lambda: det.pyramid_image_resized(ptr, 1, image(dtype=dt), H, W, scale), capi.E_UNSUPPORTED)
    refused(lambda: det.run_tensor_resized(torch.zeros((1, 3, H, W), dtype=torch.float32, device="cuda"), scale), capi.E_UNSUPPORTED)
    # the stream: planes outside [0, frame_bytes) at the SOURCE size, stride_n other than frame_bytes, depth, cap
    _, fbs = HipDetector.yuv_desc("i420", h, w)                          # room for a frame of the plan's size, not of the source's
    refused(lambda: det.stream_open_yuv_resized(good, fb - 1, H, W, scale, 64, 2))
    refused(lambda: det.stream_open_yuv_resized(variant(v_offset=-8), fb, H, W, scale, 64, 2))
    refused(lambda: det.stream_open_yuv_resized(variant(y_stride_n=fb + 4), fb, H, W, scale, 64, 2))
    refused(lambda: det.stream_open_yuv_resized(good, fb, H, W, scale, 64, 1))
    refused(lambda: det.stream_open_yuv_resized(good, fb, H, W, scale, 0, 2))
    goods, _ = HipDetector.yuv_desc("i420", H, W)
    for p in (goods.y, goods.u, goods.v):
        p.stride_n = fbs
    refused(lambda: det.stream_open_yuv_resized(goods, fbs, H, W, scale, 64, 2))
    # an active input resize: refused by the resized entries, and still by the un-resized ones
    det.set_input_resize(H, W, scale)
    refused(lambda: det.run_yuv_resized(x, 1, good, H, W, scale))
    refused(lambda: det.run_image_resized(ptr, 1, img, H, W, scale))
    refused(lambda: det.stream_open_yuv_resized(good, fb, H, W, scale, 64, 2))
    plain, _ = HipDetector.yuv_desc("i420", h, w)
    refused(lambda: det.run_yuv(x, 1, plain))
    refused(lambda: det.run_image(ptr, 1, capi.ImageDesc(capi.T_U8, 3, 3 * h * w, h * w, w, 1)))
    det.set_input_resize(0, 0, 1.0)
    det.run_yuv_resized(x, 1, good, H, W, scale)
    det.run_yuv(x, 1, plain)
    # plans of one and of five input planes
    g = HipDetector(synth.make_model(seed=3, name="FACE64", nTrees=16), h, w, 1, max_batch=1)
    refused(lambda: g.run_yuv_resized(x, 1, good, H, W, scale))
    refused(lambda: g.stream_open_yuv_resized(good, fb, H, W, scale, 64, 2))
    refused(lambda: g.run_image_resized(ptr, 1, img, H, W, scale))       # three channels into a plan of one
    g.run_image_resized(ptr, 1, image(channels=1, stride_c=0, stride_n=H * W), H, W, scale)
    g.close()
    five = HipDetector(model, h, w, 5, max_batch=1)
    refused(lambda: five.run_yuv_resized(x, 1, good, H, W, scale))
    refused(lambda: five.run_image_resized(ptr, 1, img, H, W, scale))
    five.close()
    # no plan; sub-batch contexts
    bare = HipDetector(model)
    refused(lambda: bare.run_yuv_resized(x, 1, good, H, W, scale), capi.E_NOPLAN)
    refused(lambda: bare.run_image_resized(ptr, 1, img, H, W, scale), capi.E_NOPLAN)
    refused(lambda: bare.stream_open_yuv_resized(good, fb, H, W, scale, 64, 2), capi.E_NOPLAN)
    bare.close()
    multi = HipDetector(model, h, w, 3, max_batch=4, streams=2)
    refused(lambda: multi.run_yuv_resized(x, 2, good, H, W, scale), capi.E_UNSUPPORTED)
    refused(lambda: multi.run_image_resized(ptr, 2, img, H, W, scale), capi.E_UNSUPPORTED)
    refused(lambda: multi.stream_open_yuv_resized(good, fb, H, W, scale, 64, 2), capi.E_UNSUPPORTED)
    multi.close()
    det.close()


# ---------------------------------------------------------------- 7. the C++ host

@pytest.mark.parametrize("mode", [[], ["--stream", "2"]], ids=["batch", "stream"])
def test_cli_yuv_min_width_matches_the_python_path(tmp_path, mode):
    """acf::HipDetector::detectYuv and streamOpenYuv / streamSubmit / streamCollect under setMinObjectWidth, through the CLI."""
    import subprocess
    import yuv_desc_ref as ydr
    from acf_amd.detector import HipDetector
    from acf_amd.modelio import write_model
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    from test_host_cpp import parse, run
    host = os.path.join(ROOT, "acf_amd", "host")
    subprocess.check_call(["make", "-s", "-C", host])
    H, W, cnt, min_width = 240, 320, 5, 150
    model = synth.make_model(**rc.FACE80)
    write_model(str(tmp_path / "m.acfm"), model)
    d, fb = HipDetector.yuv_desc("i420", H, W)
    buf = np.concatenate([ydr.pack("i420", *rc.yuv_planes(60 + i, H, W, 1, 1)) for i in range(cnt)])
    (tmp_path / "f.yuv").write_bytes(buf.tobytes())
    p = run(os.path.join(host, "acf_hip_detect"), ["--model", str(tmp_path / "m.acfm"), "--frames", str(tmp_path / "f.yuv"), "--yuv", "i420",
                                                   "--rows", str(H), "--cols", str(W), "--count", str(cnt), "--min-width", str(min_width),
                                                   "--luv"] + mode)           # (FACE80 takes its planes as they are)
    got = parse(p.stdout)
    scale = HipDetector.resize_scale(model["modelDs_w"], min_width)
    dr, dc = HipDetector.resize_dims(H, W, scale)
    det = HipDetector(model, dr, dc, 3, max_batch=cnt, max_hits=1 << 16)
    x = dev(buf)
    det.run_yuv_resized(x, cnt, d, H, W, scale)
    total = 0
    for f in range(cnt):
        dd, _ = det.detections(f)
        dd = HipDetector.unscale_boxes(dd, scale)
        py = [(int(r["x"]), int(r["y"]), int(r["w"]), int(r["h"]), int(np.float32(r["score"]).view(np.uint32))) for r in dd]
        assert got[f] == py, f
        total += len(py)
    assert total > 0
    det.close()
