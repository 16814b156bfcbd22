"""Crops of the stored frame without a GPU (include/acf_hip.h: "crops of the stored frame"): the declarations, the host-only entries
acf_hip_crop_box / crop_bytes / crop_form against the numpy restatement (tests/cut_crops_ref.py), and the properties of that
restatement which the GPU test (tests/test_gpu_cut_crops.py) then relies on."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import cut_crops_ref as ccr
import orient_ref as orf
from acf_amd import capi
from acf_amd.detector import HipDetector, HipError

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F = np.float32
ENTRIES = ["acf_hip_cut_crops", "acf_hip_cut_detections", "acf_hip_crop_box", "acf_hip_crop_bytes", "acf_hip_crop_form"]


def test_header_declares_the_entries_and_the_abi_stays_9():
    text = open(os.path.join(ROOT, "include", "acf_hip.h")).read()
    assert re.search(r"#define ACF_HIP_ABI_VERSION 9\b", text)
    for name in ENTRIES:
        assert re.search(r"ACF_HIP_API int %s\(" % name, text), name
        assert name in capi.DECLARED_SYMBOLS
    for name in ("acf_hip_crop_source", "acf_hip_crop_spec"):
        assert re.search(r"typedef struct %s\b" % name, text), name
    lib = capi.load()
    assert lib.acf_hip_abi_version() == 9
    for name in ENTRIES:
        assert getattr(lib, name).argtypes is not None
    # the structs as the header lays them out (LP64): 8 + 4 (+ 4) + 3 * 8 + 3 * 4 (+ 4); eight 4-byte members
    assert C.sizeof(capi.CropSource) == 56 and capi.CropSource.image.offset == 16 and capi.CropSource.src_rows.offset == 40
    assert C.sizeof(capi.CropSpec) == 32 and capi.CropSpec.grow.offset == 24


def test_crop_bytes():
    for (oh, ow, s) in ccr.SPECS:
        for dt, es in ccr.T_BYTES.items():
            for ch in (1, 3):
                for layout in (0, 1):
                    assert HipDetector.crop_bytes(ccr.spec_of(oh, ow, s, dt, layout), ch) == oh * ow * ch * es
    assert HipDetector.crop_bytes(ccr.spec_of(512, 512, 4, capi.T_F32), 3) == 512 * 512 * 3 * 4
    for bad in (ccr.spec_of(0, 5, 1), ccr.spec_of(5, 513, 1), ccr.spec_of(5, 5, 0), ccr.spec_of(5, 5, 5), ccr.spec_of(5, 5, 1, 4), ccr.spec_of(5, 5, 1, layout=2)):
        with pytest.raises(HipError) as e:
            HipDetector.crop_bytes(bad, 3)
        assert e.value.code == capi.E_INVALID
    with pytest.raises(HipError):
        HipDetector.crop_bytes(ccr.spec_of(5, 5, 1), 2)
    res = ccr.spec_of(5, 5, 1)
    res.reserved = 1
    with pytest.raises(HipError):
        HipDetector.crop_bytes(res, 3)
    assert capi.load().acf_hip_crop_bytes(None, 3, C.byref(C.c_int64())) == capi.E_INVALID
    assert capi.load().acf_hip_crop_bytes(C.byref(ccr.spec_of(5, 5, 1)), 3, None) == capi.E_INVALID


def test_crop_box_matches_the_f32_restatement():
    dets = [(0, 0, 1, 1), (13, 7, 41, 52), (-9, 4, 80, 80), (-31, -17, 64, 96), (1919, 1079, 333, 251), (5, 6, 7, 0), (100000, -100000, 12345, 54321)]
    n = 0
    for scale in (0, 1, 0.5, 80.0 / 300.0, float(HipDetector.resize_scale(80, 300))):
        for grow in (1.0, 1.3):
            for d in dets:
                got = HipDetector.crop_box(d, scale, grow)
                want = ccr.crop_box(d, scale, grow)
                assert got.dtype == F and np.array_equal(got.view(np.uint32), want.view(np.uint32)), (scale, grow, d, got, want)
                n += 1
    assert n == 5 * 2 * len(dets)
    # scale None is 0 is 1: the box itself; grow keeps the centre
    assert np.array_equal(HipDetector.crop_box((3, 4, 10, 20)), np.array([3, 4, 10, 20], dtype=F))
    g = HipDetector.crop_box((3, 4, 10, 20), None, 2.0)
    assert np.array_equal(g, np.array([-2, -6, 20, 40], dtype=F))
    assert capi.load().acf_hip_crop_box(None, 1.0, 1.0, capi.fptr(np.zeros(4, F))) == capi.E_INVALID


def _sources():
    # (Hu, Wu) of the GPU cases' stored sizes in both turns; channels; staged code bytes
    return [(hu, wu, ch, sb) for (hs, ws) in ((37, 53), (48, 64)) for (hu, wu) in ((hs, ws), (ws, hs)) for ch, sb in ((3, 1), (1, 1), (3, 2), (3, 4))]


def test_crop_form_is_deterministic_and_the_gpu_cases_take_both_forms():
    seen = {0: 0, 1: 0}
    with_boundary = 0
    for hu, wu, ch, sb in _sources():
        for (oh, ow, s) in ccr.SPECS:
            spec = ccr.spec_of(oh, ow, s)
            boxes, frames, what = ccr.boxes_for(hu, wu, 2, spec, ch, sb)
            forms = [ccr.form(spec, b, hu, wu, ch, sb) for b in boxes]
            assert forms == [ccr.form(spec, b, hu, wu, ch, sb) for b in boxes]
            assert set(forms) <= {0, 1}
            for b, f, w in zip(boxes, forms, what):
                if not ccr.box_ok(b):
                    assert f == 1, w                      # nothing is sampled: not staged
                seen[f] += 1
            if "boundary: the widest staged box" in what:
                i = what.index("boundary: the widest staged box")
                assert forms[i] == 0 and forms[i + 1] == 1 and boxes[i + 1][2] - boxes[i][2] == F(0.25)
                with_boundary += 1
            if (oh, ow, s) == (8, 8, 2):
                assert forms[what.index("the whole frame")] == 1   # the reduction: more than four pixels a sample
            if (oh, ow, s) == (112, 112, 1):
                assert forms[what.index("inside, fractional")] == 0   # an enlargement stages its few pixels
    assert seen[0] > 0 and seen[1] > 0 and with_boundary > 0, (seen, with_boundary)
    # the arguments
    lib, out, box = capi.load(), C.c_int(), np.array([1, 1, 5, 5], dtype=F)
    ok = ccr.spec_of(7, 5, 1)
    assert lib.acf_hip_crop_form(C.byref(ok), capi.fptr(box), 37, 53, 3, 1, C.byref(out)) == 0
    for args in ((None, capi.fptr(box), 37, 53, 3, 1, C.byref(out)), (C.byref(ok), None, 37, 53, 3, 1, C.byref(out)), (C.byref(ok), capi.fptr(box), 0, 53, 3, 1, C.byref(out)),
                 (C.byref(ok), capi.fptr(box), 37, 53, 2, 1, C.byref(out)), (C.byref(ok), capi.fptr(box), 37, 53, 3, 3, C.byref(out)), (C.byref(ok), capi.fptr(box), 37, 53, 3, 1, None)):
        assert lib.acf_hip_crop_form(*args) == capi.E_INVALID


def test_the_stage_budget_decides_wide_codes_sooner():
    """The same box and spec: f32 codes of three channels fill the stage where bytes do not — the second clause of the rule."""
    box = np.array([0, 0, 1500, 100], dtype=F)                   # 1501 x 101 pixels under 128 x 1024 samples: the first clause passes
    spec = ccr.spec_of(64, 512, 2)                               # an output row: at most ceil(2 * 100 / 128) + 3 = 5 rows of 1501 pixels
    assert ccr.form(spec, box, 2000, 4000, 3, 1) == 0            # 1501 x 3 x 5 bytes fit 32 KiB
    assert ccr.form(spec, box, 2000, 4000, 3, 4) == 1            # x 4 bytes a code do not


# ---------------------------------------------------------------- the numpy restatement's own properties

def _frame(seed, h, w, c=3):
    return np.random.RandomState(seed).randint(0, 256, (h, w, c)).astype(F)


def test_ref_identity_crop_reproduces_the_pixels():
    U = _frame(1, 37, 53)
    for (x, y, w, h) in ((0, 0, 53, 37), (5, 9, 16, 11), (52, 36, 1, 1)):
        val = ccr.sample(U, [x, y, w, h], h, w, 1)
        assert np.array_equal(val, U[y:y + h, x:x + w])
        assert np.array_equal(ccr.crop(U, [x, y, w, h], h, w, 1, 1.0, capi.T_U8, 1), U[y:y + h, x:x + w].astype(np.uint8))
        assert np.array_equal(ccr.crop(U, [x, y, w, h], h, w, 1, F(1 / 255.0), capi.T_F32, 0),
                              (U[y:y + h, x:x + w] * F(1 / 255.0)).transpose(2, 0, 1).view(np.uint32))


def test_ref_boxes_outside_the_frame_give_the_border():
    U = _frame(2, 37, 53)
    for box, want in (([60, 40, 9, 9], U[36, 52]), ([-30, -30, 10, 10], U[0, 0]), ([60, -30, 9, 9], U[0, 52]), ([-30, 50, 9, 9], U[36, 0])):
        val = ccr.sample(U, box, 7, 5, 2)
        assert np.array_equal(val, np.broadcast_to(want, val.shape)), box
    # beside the frame: the edge column, row by row
    val = ccr.sample(U, [-20, 4, 6, 8], 8, 3, 1)
    assert np.array_equal(val, np.broadcast_to(U[4:12, 0][:, None, :], val.shape))
    # bad boxes and frames: zeros
    for box in ([np.nan, 0, 5, 5], [0, 0, 0, 5], [0, 0, 5, -1], [0, 0, np.inf, 5]):
        assert not ccr.crop(U, box, 7, 5, 1, 1.0, capi.T_F32, 0).any()
    z = ccr.crops(U[None], np.array([[1, 1, 5, 5]] * 2, dtype=F), [-1, 1], 7, 5, 1, 1.0, capi.T_F32, 0)
    assert z.shape == (2, 3, 7, 5) and not z.any()


def test_ref_eight_orientations_equal_rot90_turned_frames():
    S = _frame(3, 37, 53)
    for code in range(8):
        rot, mirror = code & 3, code >> 2
        U = np.rot90(S[:, ::-1] if mirror else S, k=-rot)
        assert np.array_equal(U, orf.orient(S, code)) and U.shape[:2] == orf.dims(37, 53, code)
        rs, cs = orf.source_index(code, 37, 53)
        assert np.array_equal(U, S[rs, cs])                      # the header's table: upright (r, c) reads stored (rs, cs)
        box = [4.3, 6.1, 21.7, 19.2]
        got = ccr.crop(np.ascontiguousarray(U), box, 7, 5, 2, F(1 / 255.0), capi.T_F16, 0)
        assert np.array_equal(got, ccr.crop(np.ascontiguousarray(S[rs, cs]), box, 7, 5, 2, F(1 / 255.0), capi.T_F16, 0))
    # a crop of the whole upright frame at its own size is the turned frame
    for code in (1, 6):
        U = np.ascontiguousarray(orf.orient(S, code))
        assert np.array_equal(ccr.sample(U, [0, 0, U.shape[1], U.shape[0]], U.shape[0], U.shape[1], 1), U)


def test_ref_output_types():
    v = np.array([[[0.0, 0.5, 1.5]], [[2.5, 254.5, 255.5]], [[-3.0, 300.0, 127.49]]], dtype=F)
    assert ccr.finish(v, 1.0, capi.T_U8, 1).ravel().tolist() == [0, 0, 2, 2, 254, 255, 0, 255, 127]      # rint: halves to even, then the clamp
    x = np.array([[[1.0, 1.00390625, 1.01171875]]], dtype=F)                                               # bf16 keeps 8 bits: ties to even
    assert ccr.finish(x, 1.0, capi.T_BF16, 1).ravel().tolist() == [0x3f80, 0x3f80, 0x3f82]
    assert ccr.finish(x, 1.0, capi.T_F16, 1).ravel().tolist() == x.astype(np.float16).view(np.uint16).ravel().tolist()
    # samples: the s x s mean, accumulated in order, times float(1 / (s * s))
    U = _frame(4, 12, 12, 1)
    val = ccr.sample(U, [0, 0, 12, 12], 4, 4, 3)
    acc = np.zeros((4, 4, 1), dtype=F)
    for a in range(3):
        for b in range(3):
            acc = acc + U[a::3, b::3]
    assert np.array_equal(val, acc * F(1.0 / 9))
