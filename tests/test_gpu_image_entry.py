"""The image entry for upright device tensors on the device (include/acf_hip.h: acf_hip_pyramid_image / acf_hip_run_image;
HipDetector.pyramid_tensor / run_tensor): strided uint8 / float16 / bfloat16 / float32 images through k_ingest_image, every level
and every detection bit for bit against the oracle on the planes the entry is defined to read (tests/image_entry_case.py; that
each case detects something is checked on the CPU by tests/test_image_entry.py).
"""
import ctypes as C

import numpy as np
import pytest

import image_entry_case as iec
from acf_amd import capi, synth

pytestmark = pytest.mark.gpu


def bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def _run_case(det, b):
    """run_tensor on the case's view — or, where torch cannot express it (a negative stride), the raw entry on the pointer."""
    c = b["case"]
    if min(c["strides"]) < 0:
        t = iec.to_device(b["buf"], c["dtype"])
        det.run_image(t.data_ptr() + c["base"] * t.element_size(), iec.N_FRAMES, b["desc"])
    else:
        view, t = iec.tensor_view(b)
        assert view.stride() == tuple(c["strides"]) and view.storage_offset() == c["base"]
        det.run_tensor(view)
    det.synchronize()
    return t


def _check_against(det, plan, res, name):
    total = 0
    for f, (pyr, want, _) in enumerate(res):
        for i in range(plan.nScales):
            assert np.array_equal(bits(det.read_level(f, i)), bits(plan.level_view(pyr, i))), (name, f, "level", i)
        got, _ = det.detections(f)
        assert len(got) == len(want), (name, f)
        for k in ("x", "y", "w", "h", "scale"):
            assert np.array_equal(got[k], want[k]), (name, f, k)
        assert np.array_equal(bits(got["score"]), bits(want["score"])), (name, f)
        total += len(want)
    assert total > 0, "no detections: the cascade comparison would be vacuous"


@pytest.mark.parametrize("name", iec.CASE_IDS)
def test_run_tensor_bit_exact(oracle, name):
    from acf_amd.detector import HipDetector
    b = iec.build(name)
    c = b["case"]
    plan, res = iec.oracle_results(name)
    det = HipDetector(b["model"], c["H"], c["W"], c["d_in"], max_batch=iec.N_FRAMES, max_hits=1 << 16)
    keep = _run_case(det, b)
    _check_against(det, plan, res, name)
    del keep
    det.close()


def test_packed_u8_nhwc_equals_run_u8(oracle):
    """Packed RGB bytes [n, H, W, 3] through run_tensor(layout="nhwc") and through run_u8(PIX_RGB): the same levels and detections
    (rows of 175 * 3 bytes: every alignment of a row's first byte inside its dword)."""
    import torch
    from acf_amd.detector import HipDetector
    H, W, n = 131, 175, 3
    model = synth.make_model(seed=3, name="INRIA", nTrees=64, nOctUp=0, cascThr=-2.5)
    stored = np.stack([iec.round_to(synth.make_frame(60 + f, H, W, "rgb"), capi.T_U8)[0].transpose(2, 1, 0) for f in range(n)])   # [n][H][W][3]
    x = torch.from_numpy(np.ascontiguousarray(stored)).cuda()
    a = HipDetector(model, H, W, 3, max_batch=n, max_hits=1 << 16)
    b = HipDetector(model, H, W, 3, max_batch=n, max_hits=1 << 16)
    a.run_tensor(x, layout="nhwc")
    b.run_u8(x, capi.PIX_RGB)
    total = 0
    for f in range(n):
        for i in range(len(a.levels)):
            assert np.array_equal(bits(a.read_level(f, i)), bits(b.read_level(f, i))), (f, i)
        (da, ha), (db, hb) = a.detections(f), b.detections(f)
        assert da.tobytes() == db.tobytes() and ha.tobytes() == hb.tobytes(), f
        total += len(da)
    assert total > 0
    a.close()
    b.close()


def test_reference_arithmetic_tier(oracle):
    """nchw_f32_luv_vec with option "arith" = 1 and the committed tables, against the oracle's table tier."""
    from acf_amd.detector import HipDetector
    name = "nchw_f32_luv_vec"
    b = iec.build(name)
    c = b["case"]
    plan, res = iec.oracle_results(name, True)
    det = HipDetector(b["model"], c["H"], c["W"], c["d_in"], max_batch=iec.N_FRAMES, max_hits=1 << 16)
    det.set_x86_tables(*oracle.x86_fixture())
    det.set_option("arith", 1)
    keep = _run_case(det, b)
    _check_against(det, plan, res, name + " arith")
    _, exact = iec.oracle_results(name)
    assert not np.array_equal(bits(res[0][0]), bits(exact[0][0]))     # (the tier is not a no-op)
    del keep
    det.close()


def test_every_load_form_gives_the_same_planes(oracle):
    """The values of nhwc_f32_luv_scalar (131 x 175: partial tiles on both axes, a row tail of three elements) laid out for the planar
    vector form (NCHW, rows padded to 176), the packed form (NHWC; with a skipped fourth element) and the element-wise form — forced
    by strides that match neither (stride_x = 2; the NCHW layout from an odd base): every form gives the oracle's pyramid, so
    identical planes."""
    import torch
    from acf_amd.detector import HipDetector
    name = "nhwc_f32_luv_scalar"
    b = iec.build(name)
    c = b["case"]
    H, W, n = c["H"], c["W"], iec.N_FRAMES
    plan, res = iec.oracle_results(name)
    up = np.ascontiguousarray(b["planes"].transpose(0, 1, 3, 2))                            # [n][3][H][W]
    det = HipDetector(b["model"], H, W, 3, max_batch=n)
    Wp = 176
    forms = [
        ("row vectors", (3 * H * Wp, H * Wp, Wp, 1), 0),
        ("packed", (H * W * 3, 1, W * 3, 3), 0),
        ("packed, fourth element skipped", (H * W * 4, 1, W * 4, 4), 0),
        ("element-wise, stride_x 2", (3 * H * W * 2, H * W * 2, W * 2, 2), 0),
        ("element-wise, odd base", (3 * H * Wp, H * Wp, Wp, 1), 1),
    ]
    for what, strides, base in forms:
        t = torch.from_numpy(iec.lay_out(up, capi.T_F32, strides, base)).cuda()
        det.pyramid_tensor(torch.as_strided(t, (n, 3, H, W), strides, base))
        for f in range(n):
            for i in range(plan.nScales):
                assert np.array_equal(bits(det.read_level(f, i)), bits(plan.level_view(res[f][0], i))), (what, f, i)
    det.close()


@pytest.mark.parametrize("dtype", [capi.T_F16, capi.T_BF16, capi.T_U8], ids=["f16", "bf16", "u8"])
def test_narrow_types_through_the_vector_forms(oracle, dtype):
    """The 2-byte and 1-byte element types through the load forms the case table does not take them through: row vectors (contiguous
    NCHW with rows padded to 176: the 8-byte / 4-byte loads, a row tail of three elements) and packed pixels with the channels
    backwards (stride_c = -1 from the pointer at R; stride_x = 3 and 4, rows of 175 * 3 elements: every alignment of a row inside its
    dword).  131 x 175, the values of nhwc_f32_luv_scalar rounded to the type; every level against the oracle on those values."""
    from acf_amd.detector import HipDetector
    b = iec.build("nhwc_f32_luv_scalar")
    c = b["case"]
    H, W, n = c["H"], c["W"], 2
    stored, values = iec.round_to(b["planes"][:n], dtype)                                   # [n][3][W][H]
    up = np.ascontiguousarray(stored.transpose(0, 1, 3, 2))                                  # [n][3][H][W]
    plan = oracle.Plan(b["model"], H, W, 3)
    want = [oracle.chns_pyramid(plan, np.ascontiguousarray(values[f]))[0] for f in range(n)]
    det = HipDetector(b["model"], H, W, 3, max_batch=n)
    Wp = 176
    forms = [
        ("row vectors", (3 * H * Wp, H * Wp, Wp, 1), 0),
        ("packed, channels backwards", (H * W * 3, -1, W * 3, 3), 2),
        ("packed, channels backwards, fourth element skipped", (H * W * 4, -1, W * 4, 4), 2),
    ]
    for what, strides, base in forms:
        t = iec.to_device(iec.lay_out(up, dtype, strides, base), dtype)
        det.pyramid_image(t.data_ptr() + base * t.element_size(), n, capi.ImageDesc(dtype, 3, *strides))
        for f in range(n):
            for i in range(plan.nScales):
                assert np.array_equal(bits(det.read_level(f, i)), bits(plan.level_view(want[f], i))), (what, f, i)
        del t
    det.close()


def test_tap_image_after_pyramid_tensor_returns_the_planes():
    from acf_amd.detector import HipDetector
    b = iec.build("f16_roi_passthrough")
    c = b["case"]
    det = HipDetector(b["model"], c["H"], c["W"], 3, max_batch=iec.N_FRAMES, taps=True)
    view, keep = iec.tensor_view(b)
    det.pyramid_tensor(view)
    for f in range(iec.N_FRAMES):
        got = det.read_tap(f, capi.TAP_IMAGE, 0, (3, c["W"], c["H"]))
        assert np.isfinite(got).all()                       # nothing of the NaN around the view
        assert np.array_equal(bits(got), bits(b["planes"][f])), f
    del keep
    det.close()


def test_stride_n_zero_repeats_one_frame_and_stride_c_zero_one_plane(oracle):
    import torch
    from acf_amd.detector import HipDetector
    H, W = 96, 128
    model = synth.make_model(seed=3, **iec._TINY)
    frame = synth.make_frame(75, H, W, "luv")
    det = HipDetector(model, H, W, 3, max_batch=2, taps=True)
    t = torch.from_numpy(np.ascontiguousarray(frame.transpose(0, 2, 1))).cuda()             # [3][H][W]
    det.pyramid_tensor(t[None].expand(2, 3, H, W))                                           # stride_n = 0
    for f in range(2):
        assert np.array_equal(bits(det.read_tap(f, capi.TAP_IMAGE, 0, (3, W, H))), bits(frame)), f
    det.pyramid_tensor(t[1:2][None].expand(2, 3, H, W))                                      # stride_n = stride_c = 0
    for f in range(2):
        assert np.array_equal(bits(det.read_tap(f, capi.TAP_IMAGE, 0, (3, W, H))), bits(np.repeat(frame[1:2], 3, axis=0))), f
    det.close()


def test_argument_checks():
    import torch
    from acf_amd.detector import HipDetector, HipError
    model = synth.make_model(seed=3, name="TINY", nTrees=16)
    H, W = 96, 128
    det = HipDetector(model, H, W, 3, max_batch=2)
    x = torch.zeros((2, 3, H, W), dtype=torch.float32).cuda()
    ok = capi.ImageDesc(capi.T_F32, 3, 3 * H * W, H * W, W, 1)

    def code(ptr, n, desc):
        return det.lib.acf_hip_run_image(det.ctx, C.c_void_p(ptr), n, None if desc is None else C.byref(desc))

    def desc(**kw):
        d = capi.ImageDesc(capi.T_F32, 3, 3 * H * W, H * W, W, 1)
        for k, v in kw.items():
            setattr(d, k, v)
        return d

    assert code(x.data_ptr(), 2, ok) == capi.OK
    for what, rc in (("null frames", code(0, 2, ok)), ("null description", code(x.data_ptr(), 2, None)),
                     ("no frames", code(x.data_ptr(), 0, ok)), ("more than max_batch", code(x.data_ptr(), 3, ok)),
                     ("dtype", code(x.data_ptr(), 2, desc(dtype=4))), ("channels", code(x.data_ptr(), 2, desc(channels=1))),
                     ("stride_x", code(x.data_ptr(), 2, desc(stride_x=0))), ("stride_y", code(x.data_ptr(), 2, desc(stride_y=-W))),
                     ("stride_n", code(x.data_ptr(), 2, desc(stride_n=-1)))):
        assert rc == capi.E_INVALID, what
        assert det.lib.acf_hip_last_error(det.ctx), what
    assert det.lib.acf_hip_pyramid_image(None, C.c_void_p(x.data_ptr()), 2, C.byref(ok)) == capi.E_INVALID
    # the Python layer: sizes, dtype, layout
    for bad in (torch.zeros((2, 3, H, W + 1)), torch.zeros((2, 1, H, W)), torch.zeros((2, 3, H, W), dtype=torch.float64),
                torch.zeros((3, H, W))):
        with pytest.raises(HipError):
            det.run_tensor(bad.cuda())
    with pytest.raises(HipError):
        det.run_tensor(x, layout="nwhc")
    det.run_tensor(x.permute(0, 2, 3, 1).contiguous(), layout="nhwc")
    det.close()
    # no plan; a five-plane plan; an active input resize; sub-batch contexts
    bare = HipDetector(model)
    assert bare.lib.acf_hip_run_image(bare.ctx, C.c_void_p(x.data_ptr()), 2, C.byref(ok)) == capi.E_NOPLAN
    bare.close()
    five = HipDetector(synth.make_model(seed=3, name="TINY", nTrees=16), H, W, 5, max_batch=2)
    assert five.lib.acf_hip_run_image(five.ctx, C.c_void_p(x.data_ptr()), 2, C.byref(ok)) == capi.E_INVALID
    five.close()
    scale = HipDetector.resize_scale(16, 32)
    rh, rw = HipDetector.resize_dims(2 * H, 2 * W, scale)
    rz = HipDetector(model, rh, rw, 3, max_batch=2)
    rz.set_input_resize(2 * H, 2 * W, scale)
    d = capi.ImageDesc(capi.T_F32, 3, 3 * rh * rw, rh * rw, rw, 1)
    y = torch.zeros((2, 3, rh, rw), dtype=torch.float32).cuda()
    assert rz.lib.acf_hip_run_image(rz.ctx, C.c_void_p(y.data_ptr()), 2, C.byref(d)) == capi.E_INVALID
    rz.set_input_resize(0, 0, 1.0)
    assert rz.lib.acf_hip_run_image(rz.ctx, C.c_void_p(y.data_ptr()), 2, C.byref(d)) == capi.OK
    rz.close()
    kids = HipDetector(model, H, W, 3, max_batch=4, streams=2)            # (sub-batch contexts exist from 2 frames a context)
    assert kids.lib.acf_hip_run_image(kids.ctx, C.c_void_p(x.data_ptr()), 2, C.byref(ok)) == capi.E_UNSUPPORTED
    kids.close()


def test_profile_names_the_kernel_and_a_captured_graph_stays_valid(oracle):
    import torch
    from acf_amd.detector import HipDetector
    H, W = 96, 128
    model = synth.make_model(seed=3, **iec._TINY)
    frames = np.stack([synth.make_frame(80 + f, H, W, "luv") for f in range(2)])
    planar = torch.from_numpy(frames).cuda()
    upright = planar.transpose(-1, -2).contiguous()                        # [n, 3, H, W]
    det = HipDetector(model, H, W, 3, max_batch=2, max_hits=1 << 15)
    det.set_option("graph", 1)
    for _ in range(3):
        det.run(planar)                                                     # plain, captured, replayed
    want = [det.detections(f)[0] for f in range(2)]
    assert sum(len(w) for w in want) > 0
    det.run_tensor(upright[:1])                                             # runs plainly, one frame
    assert det.detections(0)[0].tobytes() == want[0].tobytes()
    det.run(planar)                                                         # the graph of acf_hip_run again
    for f in range(2):
        assert det.detections(f)[0].tobytes() == want[f].tobytes(), f
    det.set_option("graph", 0)
    det.set_option("profile", 1)
    det.run_tensor(upright)
    det.synchronize()
    assert "k_ingest_image" in det.profile()
    det.close()


# ---- the C++ host side, through tests/test_host_cpp.py's harness
def _cli_frames(tmp_path, n=3):
    from acf_amd.modelio import write_model
    H, W = 96, 128
    model = synth.make_model(seed=3, name="TINY", nTrees=96)
    frames = [synth.make_frame(40 + i, H, W, "luv") for i in range(n)]
    write_model(str(tmp_path / "m.acfm"), model)
    (tmp_path / "f.raw").write_bytes(np.stack(frames).tobytes())
    return ["--model", str(tmp_path / "m.acfm"), "--frames", str(tmp_path / "f.raw"), "--rows", str(W), "--cols", str(H),
            "--channels", "3", "--count", str(n), "--luv"]


@pytest.mark.parametrize("mode", [["--via-images"], ["--via-images", "--nms", "--max-count", "5"], ["--interleaved"], ["--interleaved", "--transposed"]])
def test_host_cpp_image_entries_equal_detect_batch(tmp_path, mode):
    """acf::HipDetector::detectImages (the transposed planes described as upright images by their strides) and
    operator()(const float* rgbInterleaved, ...) (upright, and transposed after setIsTranspose(true)) print what detectBatch prints
    for the same frames."""
    import subprocess
    import test_host_cpp as th
    subprocess.check_call(["make", "-s", "-C", th.HOST])
    common = _cli_frames(tmp_path)
    nms = [m for m in mode if m not in ("--via-images", "--interleaved", "--transposed")]
    want = th.parse(th.run(th.CLI, common + ["--batch"] + nms).stdout)
    got = th.parse(th.run(th.CLI, common + mode).stdout)
    assert sum(len(w) for w in want) > 0
    assert got == want
