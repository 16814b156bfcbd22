"""Video formats (include/acf_hip.h: acf_hip_yuv_format), the part that needs no GPU: the header's declarations, the constants of
acf_hip_yuv_coeffs against their derivation with fractions.Fraction (tests/video_format_ref.py), acf_hip_video_layout /
acf_hip_video_extent against frames of 16-bit words packed by hand in numpy, and what the host functions refuse."""
import ctypes as C
import fnmatch
import os
import re

import numpy as np
import pytest

import video_format_ref as vr
import yuv_desc_ref as ydr
from acf_amd import capi
from acf_amd.detector import HipDetector, HipError

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ["acf_hip_pyramid_video", "acf_hip_run_video", "acf_hip_stream_open_video", "acf_hip_video_to_rgb", "acf_hip_video_extent",
       "acf_hip_video_layout", "acf_hip_yuv_coeffs"]
TABLE = {  # the issue's table, written out: (matrix, full_range) -> CY, CVR, CVG, CUG, CUB
    (0, 0): (1220542, 1673527, -852492, -409993, 2116026), (0, 1): (1048576, 1470104, -748826, -360853, 1858077),
    (1, 0): (1220945, 1879825, -558796, -223607, 2215014), (1, 1): (1048576, 1651297, -490864, -196424, 1945738),
    (2, 0): (1220945, 1760217, -682019, -196426, 2245811), (2, 1): (1048576, 1546230, -599107, -172546, 1972791),
}


def F(bits=8, shift=0, matrix=0, full=0):
    return capi.YuvFormat(bits, shift, matrix, full)


def _layout(code, fmt, h, w, stride=0):
    d, fb = capi.YuvDesc(), C.c_int64(-1)
    rc = capi.load().acf_hip_video_layout(code, C.byref(fmt) if fmt is not None else None, h, w, stride, C.byref(d), C.byref(fb))
    return rc, d, fb.value


def _extent(d, fmt, h, w, n):
    lo, hi = (C.c_int64 * 3)(), (C.c_int64 * 3)()
    rc = capi.load().acf_hip_video_extent(C.byref(d), C.byref(fmt) if fmt is not None else None, h, w, n, lo, hi)
    return rc, list(lo), list(hi)


def _desc(y, u, v, sx, sy):
    return capi.YuvDesc(capi.YuvPlane(*y), capi.YuvPlane(*u), capi.YuvPlane(*v), sx, sy)


def _same_desc(a, b):
    return all(ydr.plane_tuple(p) == ydr.plane_tuple(q) for p, q in zip((a.y, a.u, a.v), (b.y, b.u, b.v))) and (a.sub_x, a.sub_y) == (b.sub_x, b.sub_y)


# ---------------------------------------------------------------- declarations

def test_header_declares_the_entries_and_keeps_the_abi():
    hdr = open(os.path.join(ROOT, "include", "acf_hip.h")).read()
    lib = capi.load()
    patterns = re.findall(r"global:\s*([^;]+);", open(os.path.join(ROOT, "acf_amd", "csrc", "exports.map")).read())
    assert patterns
    for name in NEW:
        assert re.search(r"ACF_HIP_API int %s\(" % name, hdr), name
        assert name in capi.DECLARED_SYMBOLS and hasattr(lib, name), name
        assert any(fnmatch.fnmatchcase(name, p.strip()) for pat in patterns for p in pat.split()), name
    assert re.search(r"#define ACF_HIP_ABI_VERSION 9\b", hdr) and lib.acf_hip_abi_version() == 9
    assert C.sizeof(capi.YuvFormat) == 16 and C.sizeof(capi.YuvDesc) == 104
    for i, n in enumerate(("BT601", "BT709", "BT2020")):
        assert re.search(r"ACF_HIP_YUV_MATRIX_%s = %d\b" % (n, i), hdr)
        assert capi.YUV_MATRIX_NAMES[n.lower()] == i
    assert "PARITY UNPINNED" in hdr[hdr.index("acf_hip_yuv_format") - 8000:hdr.index("acf_hip_yuv_format")] and "H.273" in hdr


# ---------------------------------------------------------------- the constants

@pytest.mark.parametrize("bits", [8, 10, 12, 16])
@pytest.mark.parametrize("matrix,full", sorted(TABLE))
def test_coeffs_are_the_table_and_the_derivation(bits, matrix, full):
    got = HipDetector.yuv_coeffs(F(bits, 0, matrix, full))
    want = vr.coeffs(bits, matrix, full)
    assert tuple(want[3:]) == TABLE[(matrix, full)]            # the Fraction derivation gives the issue's table
    assert got == want, (bits, matrix, full)
    assert got[:3] == [0 if full else 16 << (bits - 8), 1 << (bits - 1), (1 << bits) - 1 if full else 255 << (bits - 8)]


def test_null_format_is_the_default():
    assert HipDetector.yuv_coeffs(None) == HipDetector.yuv_coeffs(F()) == vr.coeffs(8, 0, 0)


def test_eight_bit_sums_fit_int32():
    """The 8-bit kernels work in int32: the largest magnitude of every sum, for all six rows."""
    for (m, f), (cy, cvr, cvg, cug, cub) in TABLE.items():
        y = (255 - (0 if f else 16)) * cy + (1 << 19)
        for lo, hi in ((min(cvr * -128, cvr * 127), max(cvr * -128, cvr * 127)), (cvg * 127 + cug * 127, cvg * -128 + cug * -128),
                       (min(cub * -128, cub * 127), max(cub * -128, cub * 127))):
            assert -(1 << 31) <= (1 << 19) + lo and y + hi < (1 << 31), (m, f)


# ---------------------------------------------------------------- layouts and extents of 16-bit words

CASES16 = [  # name, layout, bits, shift
    ("p010", "nv12", 10, 6), ("p016", "nv12", 16, 0), ("yuv420p10le", "i420", 10, 0), ("i210", "i422", 10, 0), ("i410", "i444", 10, 0),
    ("y210", "yuyv", 10, 6),
]


@pytest.mark.parametrize("pad", [0, 8], ids=["tight", "padded"])
@pytest.mark.parametrize("tag,name,bits,shift", CASES16, ids=[c[0] for c in CASES16])
def test_layout16_gathers_what_numpy_packed(tag, name, bits, shift, pad):
    rows, cols = 6, 8
    stride = 0 if not pad else (4 * cols if name in ydr.PACKED_ORDER else 2 * cols) + pad
    fmt = F(bits, shift)
    Y, U, V = vr.random_planes16(21, name, rows, cols, bits)
    buf = vr.pack16(name, Y, U, V, shift, stride, fill=0x3333)
    rc, d, fb = _layout(capi.YUV_NAMES[name], fmt, rows, cols, stride)
    assert rc == capi.OK and fb == buf.size, (tag, fb, buf.size)
    assert (d.sub_x, d.sub_y) == ydr.SUB[name] and d.y.stride_n == d.u.stride_n == d.v.stride_n == fb
    if name == "nv12":
        assert d.y.stride_px == 2 and d.u.stride_px == d.v.stride_px == 4 and d.v.offset == d.u.offset + 2
    elif name not in ydr.PACKED_ORDER:
        assert d.y.stride_px == d.u.stride_px == d.v.stride_px == 2
    Y2, U2, V2 = vr.random_planes16(22, name, rows, cols, bits)
    both = np.concatenate([buf, vr.pack16(name, Y2, U2, V2, shift, stride, fill=0x4444)])
    gy, gu, gv = vr.gather(both, d, rows, cols, bits, shift, n=2)
    assert np.array_equal(gy[0], Y) and np.array_equal(gu[0], U) and np.array_equal(gv[0], V), tag
    assert np.array_equal(gy[1], Y2) and np.array_equal(gu[1], U2) and np.array_equal(gv[1], V2), tag
    for n in (1, 2):
        rc, lo, hi = _extent(d, fmt, rows, cols, n)
        assert rc == capi.OK and (lo, hi) == vr.extent(d, rows, cols, bits, n), tag
    # `last` is the high byte of the last word: the three planes together end with the frame, or with its padding
    _, lo, hi = _extent(d, fmt, rows, cols, 1)
    semi_or_packed = name in ydr.PACKED_ORDER or name == "nv12"
    assert min(lo) == 0 and max(hi) == fb - 1 - (pad if semi_or_packed else pad >> d.sub_x)


def test_p010_values_written_out():
    rc, d, fb = _layout(capi.YUV_NV12, F(10, 6), 4, 8)
    assert rc == capi.OK and fb == 96
    assert [ydr.plane_tuple(p) for p in (d.y, d.u, d.v)] == [(0, 96, 16, 2), (64, 96, 16, 4), (66, 96, 16, 4)]
    assert _extent(d, F(10, 6), 4, 8, 1)[1:] == ([0, 64, 66], [63, 93, 95])


def test_extent16_of_hand_built_odd_sizes():
    """5 x 7 planar 4:2:0 words with 3 x 4 chroma planes, an odd word stride, the planes anywhere (one below the base)."""
    d = _desc((0, 1000, 18, 2), (-400, 1000, 10, 2), (500, 0, 10, 2), 1, 1)
    rc, lo, hi = _extent(d, F(12, 4), 5, 7, 3)
    assert rc == capi.OK and lo == [0, -400, 500]
    assert hi == [2000 + 4 * 18 + 6 * 2 + 1, -400 + 2000 + 2 * 10 + 3 * 2 + 1, 500 + 2 * 10 + 3 * 2 + 1]
    assert (lo, hi) == vr.extent(d, 5, 7, 12, 3)


@pytest.mark.parametrize("name", ydr.NAMES)
def test_eight_bit_formats_equal_the_yuv_functions(name):
    for fmt in (None, F(), F(8, 0, 1, 0), F(8, 0, 2, 1)):
        for stride in (0, 40):
            want = HipDetector.yuv_desc(name, 6, 8, stride)
            rc, d, fb = _layout(capi.YUV_NAMES[name], fmt, 6, 8, stride)
            assert rc == capi.OK and fb == want[1] and _same_desc(d, want[0]), (name, stride)
            assert _extent(d, fmt, 6, 8, 2)[1:] == tuple(HipDetector.yuv_extent(d, 6, 8, 2))


# ---------------------------------------------------------------- refusals

BAD_FORMATS = [F(7), F(17), F(8, 1), F(10, 7), F(16, 1), F(10, -1), F(8, 0, 3), F(8, 0, -1), F(8, 0, 0, 2), F(8, 0, 0, -1)]


@pytest.mark.parametrize("i", range(len(BAD_FORMATS)))
def test_host_functions_refuse_a_bad_format(i):
    fmt = BAD_FORMATS[i]
    out = (C.c_int64 * 8)()
    assert capi.load().acf_hip_yuv_coeffs(C.byref(fmt), out) == capi.E_INVALID
    assert _layout(capi.YUV_I420, fmt, 4, 8)[0] == capi.E_INVALID
    d, _ = HipDetector.yuv_desc("i420", 4, 8)
    assert _extent(d, fmt, 4, 8, 1)[0] == capi.E_INVALID
    with pytest.raises(HipError):
        HipDetector.yuv_coeffs(fmt)


def test_host_functions_refuse_the_rest():
    lib = capi.load()
    assert lib.acf_hip_yuv_coeffs(C.byref(F()), None) == capi.E_INVALID
    f10 = F(10, 6)
    d, fb = capi.YuvDesc(), C.c_int64()
    # what acf_hip_yuv_layout refuses, in words: unknown names, sizes, odd sizes of subsampled names, short or odd strides, null outputs
    for code, h, w, stride in ((-1, 4, 8, 0), (9, 4, 8, 0), (capi.YUV_NV12, 0, 8, 0), (capi.YUV_NV12, 4, 0, 0), (capi.YUV_NV12, 5, 8, 0),
                               (capi.YUV_I422, 4, 7, 0), (capi.YUV_NV12, 4, 8, 14), (capi.YUV_NV12, 4, 8, 17), (capi.YUV_NV12, 4, 8, -2),
                               (capi.YUV_I420, 4, 8, 18), (capi.YUV_YUYV, 4, 8, 30)):
        assert lib.acf_hip_video_layout(code, C.byref(f10), h, w, stride, C.byref(d), C.byref(fb)) == capi.E_INVALID, (code, h, w, stride)
    assert lib.acf_hip_video_layout(capi.YUV_NV12, C.byref(f10), 4, 8, 0, None, C.byref(fb)) == capi.E_INVALID
    assert lib.acf_hip_video_layout(capi.YUV_NV12, C.byref(f10), 4, 8, 0, C.byref(d), None) == capi.E_INVALID
    good = _layout(capi.YUV_NV12, f10, 4, 8)[1]
    lo, hi = (C.c_int64 * 3)(), (C.c_int64 * 3)()
    assert lib.acf_hip_video_extent(None, C.byref(f10), 4, 8, 1, lo, hi) == capi.E_INVALID
    assert lib.acf_hip_video_extent(C.byref(good), C.byref(f10), 4, 8, 1, None, hi) == capi.E_INVALID
    assert lib.acf_hip_video_extent(C.byref(good), C.byref(f10), 4, 8, 1, lo, None) == capi.E_INVALID
    for h, w, n in ((0, 8, 1), (4, 0, 1), (4, 8, 0)):
        assert _extent(good, f10, h, w, n)[0] == capi.E_INVALID
    # 16-bit words at odd offsets or strides; what acf_hip_yuv_extent refuses about a descriptor
    for bad in (_desc((1, 96, 16, 2), (64, 96, 16, 4), (66, 96, 16, 4), 1, 1), _desc((0, 95, 16, 2), (64, 96, 16, 4), (66, 96, 16, 4), 1, 1),
                _desc((0, 96, 17, 2), (64, 96, 16, 4), (66, 96, 16, 4), 1, 1), _desc((0, 96, 16, 2), (64, 96, 16, 3), (66, 96, 16, 4), 1, 1),
                _desc((0, 96, 16, 2), (64, 96, 16, 4), (66, 96, 16, 4), 2, 1), _desc((0, 96, 16, 0), (64, 96, 16, 4), (66, 96, 16, 4), 1, 1),
                _desc((0, -2, 16, 2), (64, 96, 16, 4), (66, 96, 16, 4), 1, 1)):
        assert _extent(bad, f10, 4, 8, 1)[0] == capi.E_INVALID
    with pytest.raises(HipError):
        HipDetector.video_desc("p010", 4, 8, f10)  # not a layout name: P010 is ("nv12", bits 10, shift 6)
    assert HipDetector.video_desc("nv12", 4, 8, f10)[1] == 96
    assert HipDetector.video_format(10, 6, "bt2020", True).matrix == 2 and HipDetector.video_format(matrix="rec709").matrix == -1
