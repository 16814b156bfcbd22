"""The image entry for upright device tensors, the parts that need no GPU: the declarations (include/acf_hip.h, capi), the host
arithmetic of acf_hip_image_extent, and the precondition of tests/test_gpu_image_entry.py — every case detects something in
the oracle alone, so the comparison on the device is not vacuous.
"""
import ctypes as C
import os

import pytest

import image_entry_case as iec
from acf_amd import capi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_header_declares_the_entries_and_keeps_the_abi_version():
    header = open(os.path.join(ROOT, "include", "acf_hip.h")).read()
    for name in ("acf_hip_pyramid_image", "acf_hip_run_image", "acf_hip_image_extent"):
        assert "ACF_HIP_API int %s(" % name in header, name
        assert name in capi.DECLARED_SYMBOLS
    assert "typedef struct acf_hip_image_desc" in header
    for k, v in (("ACF_HIP_T_U8", 0), ("ACF_HIP_T_F16", 1), ("ACF_HIP_T_BF16", 2), ("ACF_HIP_T_F32", 3)):
        assert "%s = %d" % (k, v) in header
    assert "#define ACF_HIP_ABI_VERSION 9" in header     # additive: the version stays


def test_struct_has_the_c_layout():
    assert C.sizeof(capi.ImageDesc) == 40
    assert [getattr(capi.ImageDesc, f).offset for f, _ in capi.ImageDesc._fields_] == [0, 4, 8, 16, 24, 32]
    assert (capi.T_U8, capi.T_F16, capi.T_BF16, capi.T_F32) == (0, 1, 2, 3)


def _extent(desc, h, w, n):
    lo, hi = C.c_int64(7), C.c_int64(7)
    rc = capi.load().acf_hip_image_extent(C.byref(desc), h, w, n, C.byref(lo), C.byref(hi))
    return rc, lo.value, hi.value


# name, (dtype, channels, sn, sc, sy, sx), h, w, n, first, last: worked out by hand
EXTENTS = [
    # [2, 3, 4, 5] contiguous: the last element of the tensor
    ("nchw", (capi.T_F32, 3, 60, 20, 5, 1), 4, 5, 2, 0, 119),
    # [2, 4, 5, 3] seen as NCHW: 60 * 1 + 1 * 2 + 15 * 3 + 3 * 4
    ("nhwc", (capi.T_U8, 3, 60, 1, 15, 3), 4, 5, 2, 0, 119),
    # [2, 4, 5, 4][..., :3]: 80 + 2 + 20 * 3 + 4 * 4 = 158; the last alpha (159) is not read
    ("rgba_skip", (capi.T_BF16, 3, 80, 1, 20, 4), 4, 5, 2, 0, 158),
    # rows 5 .. 100, columns 3 .. 130 of [3, 3, 120, 160] from the view's first element: 2 * 57600 + 2 * 19200 + 95 * 160 + 127
    ("padded_roi", (capi.T_F16, 3, 57600, 19200, 160, 1), 96, 128, 3, 0, 168927),
    # packed BGR from the R of pixel 0: B is two elements in front; the last pixel's R is the highest: 60 + 15 * 3 + 3 * 4
    ("bgr", (capi.T_F32, 3, 60, -1, 15, 3), 4, 5, 2, -2, 117),
    # one frame repeated
    ("stride_n_0", (capi.T_F32, 3, 0, 20, 5, 1), 4, 5, 7, 0, 59),
]


@pytest.mark.parametrize("row", EXTENTS, ids=[r[0] for r in EXTENTS])
def test_image_extent_by_hand(row):
    _, d, h, w, n, first, last = row
    assert _extent(capi.ImageDesc(*d), h, w, n) == (capi.OK, first, last)
    assert iec.extent(d[2:], d[1], h, w, n) == (first, last)     # (the helper the layouts below are built with)


def test_image_extent_refusals():
    ok = (capi.T_F32, 3, 60, 20, 5, 1)
    assert _extent(capi.ImageDesc(*ok), 4, 5, 2)[0] == capi.OK
    for bad in ((4, 3, 60, 20, 5, 1), (-1, 3, 60, 20, 5, 1),          # unknown dtype
                (capi.T_F32, 2, 60, 20, 5, 1),                        # channels 2
                (capi.T_F32, 3, 60, 20, 5, 0),                        # stride_x 0
                (capi.T_F32, 3, 60, 20, 0, 1), (capi.T_F32, 3, -60, 20, 5, 1)):
        assert _extent(capi.ImageDesc(*bad), 4, 5, 2)[0] == capi.E_INVALID, bad
    lib = capi.load()
    lo = C.c_int64()
    assert lib.acf_hip_image_extent(None, 4, 5, 2, C.byref(lo), C.byref(lo)) == capi.E_INVALID
    assert lib.acf_hip_image_extent(C.byref(capi.ImageDesc(*ok)), 4, 5, 2, None, C.byref(lo)) == capi.E_INVALID
    assert _extent(capi.ImageDesc(*ok), 0, 5, 2)[0] == capi.E_INVALID
    assert _extent(capi.ImageDesc(*ok), 4, 5, 0)[0] == capi.E_INVALID


@pytest.mark.parametrize("name", iec.CASE_IDS)
def test_case_layout_matches_the_extent_entry(name):
    """Every case's buffer holds its view: the library's extent, from the case's base, lies inside it — and where the case says so the
    view ends with the buffer."""
    b = iec.build(name)
    c = b["case"]
    rc, lo, hi = _extent(b["desc"], c["H"], c["W"], iec.N_FRAMES)
    assert rc == capi.OK and c["base"] + lo >= 0 and c["base"] + hi < b["buf"].size
    if c["size"] is None:
        assert c["base"] + hi == b["buf"].size - 1


@pytest.mark.parametrize("name", iec.CASE_IDS)
def test_every_gpu_case_detects_something_in_the_oracle(oracle, name):
    _, res = iec.oracle_results(name)
    assert sum(len(det) for _, det, _ in res) > 0, "no detections: the comparison on the device would be vacuous"


def test_arith_case_detects_something_in_the_oracles_table_tier(oracle):
    _, res = iec.oracle_results("nchw_f32_luv_vec", True)
    assert sum(len(det) for _, det, _ in res) > 0
