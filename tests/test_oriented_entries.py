"""The oriented entries without a GPU: the header and the exports, and the host arithmetic (acf_hip_oriented_dims,
acf_hip_unorient_rect) against the numpy restatement of the orientation codes (tests/orient_ref.py)."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import orient_ref as orf
import oriented_case as oc
from acf_amd import capi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRIES = ["acf_hip_pyramid_image_oriented", "acf_hip_run_image_oriented", "acf_hip_pyramid_yuv_oriented", "acf_hip_run_yuv_oriented",
           "acf_hip_stream_open_yuv_oriented", "acf_hip_oriented_dims", "acf_hip_unorient_rect"]
CODES = range(8)
SIZES = [(7, 11), (8, 12)]


def rect(lib, code, rows, cols, box):
    a, b = (C.c_int32 * 4)(*box), (C.c_int32 * 4)()
    assert lib.acf_hip_unorient_rect(code, rows, cols, a, b) == capi.OK
    return list(b)


def test_header_declares_the_entries_and_keeps_abi_9():
    hdr = open(os.path.join(ROOT, "include", "acf_hip.h")).read()
    lib = capi.load()
    for e in ENTRIES:
        assert re.search(r"ACF_HIP_API int %s\(" % e, hdr), e
        assert e in capi.DECLARED_SYMBOLS and hasattr(lib, e), e
    assert re.search(r"#define\s+ACF_HIP_ABI_VERSION\s+9\b", hdr) and lib.acf_hip_abi_version() == 9
    names = ["UPRIGHT", "ROT90", "ROT180", "ROT270", "MIRROR", "MIRROR_ROT90", "MIRROR_ROT180", "MIRROR_ROT270"]
    for code, n in enumerate(names):
        assert re.search(r"ACF_HIP_ORIENT_%s = %d\b" % (n, code), hdr), n
        assert getattr(capi, "ORIENT_" + n) == code
    assert "np.rot90(S[:, ::-1] if mirror else S, k=-rot)" in hdr          # which way clockwise is
    for k in ("k_ingest_image_oriented_rows", "k_ingest_image_oriented_cols", "k_ingest_image_oriented_generic", "k_ingest_yuv_oriented_rows",
              "k_ingest_yuv_oriented_cols", "k_ingest_yuv_oriented_generic"):
        assert k in hdr, k


def test_numpy_helper_is_the_table_and_its_inverse_undoes_it():
    for rows, cols in SIZES:
        S = np.arange(rows * cols).reshape(rows, cols)
        for code in CODES:
            U = orf.orient(S, code)
            assert U.shape == orf.dims(rows, cols, code)
            rs, cs = orf.source_index(code, rows, cols)
            assert np.array_equal(U, S[rs, cs]), code
            assert np.array_equal(orf.unorient(U, code), S), code
            assert np.array_equal(orf.orient(U, orf.inverse_code(code)), S), code
    # with leading axes (a batch of interleaved frames)
    B = np.arange(2 * 7 * 11 * 3).reshape(2, 7, 11, 3)
    for code in CODES:
        assert np.array_equal(orf.orient(B, code, axes=(1, 2))[1, :, :, 2], orf.orient(B[1, :, :, 2], code))


@pytest.mark.parametrize("code", CODES)
def test_oriented_dims(code):
    lib = capi.load()
    from acf_amd.detector import HipDetector
    for rows, cols in SIZES + [(1, 5), (1080, 1920)]:
        h, w = C.c_int(), C.c_int()
        assert lib.acf_hip_oriented_dims(rows, cols, code, C.byref(h), C.byref(w)) == capi.OK
        assert (h.value, w.value) == orf.orient(np.zeros((rows, cols)), code).shape
        assert HipDetector.oriented_dims(rows, cols, code) == (h.value, w.value)


@pytest.mark.parametrize("code", CODES)
@pytest.mark.parametrize("rows,cols", SIZES)
def test_unorient_rect_is_the_bounding_box_of_the_mapped_mask(rows, cols, code):
    """Every in-frame box: painted into an upright mask, the mask taken to the source by the inverse permutation."""
    lib = capi.load()
    h, w = orf.dims(rows, cols, code)
    n = 0
    for y in range(h):
        for x in range(w):
            for bh in (1, 2, h - y):
                for bw in (1, 3, w - x):
                    if y + bh > h or x + bw > w:
                        continue
                    m = np.zeros((h, w), bool)
                    m[y:y + bh, x:x + bw] = True
                    src = orf.unorient(m, code)
                    assert src.shape == (rows, cols)
                    assert rect(lib, code, rows, cols, [x, y, bw, bh]) == orf.box_of_mask(src), (code, x, y, bw, bh)
                    n += 1
    assert n > 100


@pytest.mark.parametrize("code", CODES)
def test_unorient_rect_outside_the_frame_and_back(code):
    """Boxes that reach outside (padded detections): the documented closed form; the inverse code returns the box."""
    lib = capi.load()
    rng = np.random.RandomState(code)
    for rows, cols in SIZES:
        h, w = orf.dims(rows, cols, code)
        for _ in range(200):
            box = [int(rng.randint(-9, w + 4)), int(rng.randint(-9, h + 4)), int(rng.randint(1, 30)), int(rng.randint(1, 30))]
            got = rect(lib, code, rows, cols, box)
            assert got == orf.unorient_box(code, rows, cols, box), (code, box)
            # the source is the upright frame of the upright frame under the inverse code
            assert rect(lib, orf.inverse_code(code), h, w, got) == box, (code, box)


def test_unorient_boxes_wrapper():
    from acf_amd.detector import HipDetector
    d = np.zeros(3, capi.DET_DTYPE)
    d["x"], d["y"], d["w"], d["h"], d["score"] = [1, -2, 5], [0, 3, 4], [2, 3, 4], [5, 6, 9], [1.5, 2.5, 3.5]
    for code in CODES:
        out = HipDetector.unorient_boxes(d, code, 7, 11)
        for i in range(3):
            assert [out[k][i] for k in "xywh"] == orf.unorient_box(code, 7, 11, [d[k][i] for k in "xywh"])
        assert np.array_equal(out["score"], d["score"])


def test_bad_codes_and_null_pointers():
    lib = capi.load()
    h, w = C.c_int(), C.c_int()
    a, b = (C.c_int32 * 4)(0, 0, 1, 1), (C.c_int32 * 4)()
    for code in (-1, 8, 12):
        assert lib.acf_hip_oriented_dims(7, 11, code, C.byref(h), C.byref(w)) == capi.E_INVALID
        assert lib.acf_hip_unorient_rect(code, 7, 11, a, b) == capi.E_INVALID
    for rows, cols in ((0, 11), (7, 0), (-1, 3)):
        assert lib.acf_hip_oriented_dims(rows, cols, 1, C.byref(h), C.byref(w)) == capi.E_INVALID
        assert lib.acf_hip_unorient_rect(1, rows, cols, a, b) == capi.E_INVALID
    assert lib.acf_hip_oriented_dims(7, 11, 1, None, C.byref(w)) == capi.E_INVALID
    assert lib.acf_hip_oriented_dims(7, 11, 1, C.byref(h), None) == capi.E_INVALID
    assert lib.acf_hip_unorient_rect(1, 7, 11, None, b) == capi.E_INVALID
    assert lib.acf_hip_unorient_rect(1, 7, 11, a, None) == capi.E_INVALID


@pytest.mark.parametrize("mkey,size,klass", oc.USED, ids=["%s-%dx%d-%s" % (m, s[0], s[1], k if isinstance(k, str) else "sub%d%d" % k) for m, s, k in oc.USED])
def test_every_reference_of_the_gpu_tests_detects_something(oracle, mkey, size, klass):
    """The GPU tests compare detections bit for bit: every model x upright size x frame class they use has at least one detection in
    every frame and every orientation (by the oracle alone), so no comparison there is one of empty lists."""
    for code in CODES:
        counts = oc.oracle_counts(mkey, size, klass, code)
        assert len(counts) == oc.N_FRAMES and min(counts) >= 1, (code, counts)
