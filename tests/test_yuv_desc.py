"""Three-plane YUV descriptors, the part that needs no GPU: acf_hip_yuv_layout's descriptors of the nine named layouts against
frames packed by hand in numpy (tests/yuv_desc_ref.py), acf_hip_yuv_extent against hand-computed byte ranges, what both refuse, and
the header's declarations (include/acf_hip.h: acf_hip_yuv_desc)."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import yuv_desc_ref as ydr
from acf_amd import capi
from acf_amd.detector import HipDetector, HipError

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _layout(code, h, w, stride=0):
    d, fb = capi.YuvDesc(), C.c_int64(-1)
    rc = capi.load().acf_hip_yuv_layout(code, h, w, stride, C.byref(d), C.byref(fb))
    return rc, d, fb.value


def _extent(d, h, w, n):
    lo, hi = (C.c_int64 * 3)(), (C.c_int64 * 3)()
    rc = capi.load().acf_hip_yuv_extent(C.byref(d), h, w, n, lo, hi)
    return rc, list(lo), list(hi)


def _desc(y, u, v, sx, sy):
    return capi.YuvDesc(capi.YuvPlane(*y), capi.YuvPlane(*u), capi.YuvPlane(*v), sx, sy)


# ---------------------------------------------------------------- the named layouts

def test_the_enum_is_its_own_and_in_the_header_order():
    assert [capi.YUV_NAMES[n] for n in ydr.NAMES] == list(range(9))
    hdr = open(os.path.join(ROOT, "include", "acf_hip.h")).read()
    for n in ydr.NAMES:
        assert re.search(r"ACF_HIP_YUV_%s = %d\b" % (n.upper(), capi.YUV_NAMES[n]), hdr), n


@pytest.mark.parametrize("name", ydr.NAMES)
@pytest.mark.parametrize("pad", [0, 6], ids=["tight", "padded"])
def test_layout_descriptor_gathers_what_numpy_packed(name, pad):
    rows, cols = 6, 8
    stride = 0 if not pad else (2 * cols if name in ydr.PACKED_ORDER else cols) + pad
    Y, U, V = ydr.random_planes(11, name, rows, cols)
    buf = ydr.pack(name, Y, U, V, stride, fill=0x33)
    rc, d, fb = _layout(capi.YUV_NAMES[name], rows, cols, stride)
    assert rc == capi.OK
    assert fb == buf.size, (name, fb, buf.size)
    assert (d.sub_x, d.sub_y) == ydr.SUB[name]
    assert d.y.stride_n == d.u.stride_n == d.v.stride_n == fb
    gy, gu, gv = ydr.gather(buf, d, rows, cols)
    assert np.array_equal(gy[0], Y) and np.array_equal(gu[0], U) and np.array_equal(gv[0], V), name
    # two frames back to back: frame 1 through stride_n
    Y2, U2, V2 = ydr.random_planes(12, name, rows, cols)
    both = np.concatenate([buf, ydr.pack(name, Y2, U2, V2, stride, fill=0x44)])
    gy, gu, gv = ydr.gather(both, d, rows, cols, n=2)
    assert np.array_equal(gy[1], Y2) and np.array_equal(gu[1], U2) and np.array_equal(gv[1], V2), name
    # every plane's extent lies inside one frame and the three together end with it
    rc, lo, hi = _extent(d, rows, cols, 1)
    assert rc == capi.OK and min(lo) == 0 and max(hi) == fb - 1 - (pad if name in ydr.PACKED_ORDER or name in ("nv12", "nv21") else pad >> d.sub_x)


def test_layout_values_written_out():
    """The descriptors of 4 x 8, as plain numbers."""
    t = lambda p: ydr.plane_tuple(p)
    rc, d, fb = _layout(capi.YUV_I420, 4, 8)
    assert (rc, fb) == (capi.OK, 48) and (t(d.y), t(d.u), t(d.v)) == ((0, 48, 8, 1), (32, 48, 4, 1), (40, 48, 4, 1))
    rc, d, fb = _layout(capi.YUV_YV12, 4, 8, 16)
    assert (rc, fb) == (capi.OK, 96) and (t(d.y), t(d.u), t(d.v)) == ((0, 96, 16, 1), (80, 96, 8, 1), (64, 96, 8, 1))
    rc, d, fb = _layout(capi.YUV_I422, 3, 8)
    assert (rc, fb) == (capi.OK, 48) and (t(d.y), t(d.u), t(d.v)) == ((0, 48, 8, 1), (24, 48, 4, 1), (36, 48, 4, 1))
    rc, d, fb = _layout(capi.YUV_I444, 3, 5, 6)
    assert (rc, fb) == (capi.OK, 54) and (t(d.y), t(d.u), t(d.v)) == ((0, 54, 6, 1), (18, 54, 6, 1), (36, 54, 6, 1))
    rc, d, fb = _layout(capi.YUV_NV21, 4, 8)
    assert (rc, fb) == (capi.OK, 48) and (t(d.y), t(d.u), t(d.v)) == ((0, 48, 8, 1), (33, 48, 8, 2), (32, 48, 8, 2))
    assert fb == HipDetector.u8_frame_bytes(capi.PIX_NV21, 4, 8)
    rc, d, fb = _layout(capi.YUV_YUYV, 3, 4)
    assert (rc, fb) == (capi.OK, 24) and (t(d.y), t(d.u), t(d.v)) == ((0, 24, 8, 2), (1, 24, 8, 4), (3, 24, 8, 4))
    rc, d, fb = _layout(capi.YUV_UYVY, 3, 4, 12)
    assert (rc, fb) == (capi.OK, 36) and (t(d.y), t(d.u), t(d.v)) == ((1, 36, 12, 2), (0, 36, 12, 4), (2, 36, 12, 4))
    rc, d, fb = _layout(capi.YUV_YVYU, 3, 4)
    assert (rc, fb) == (capi.OK, 24) and (t(d.y), t(d.u), t(d.v)) == ((0, 24, 8, 2), (3, 24, 8, 4), (1, 24, 8, 4))


def test_layout_refusals():
    bad = [(capi.YUV_I420, 5, 8, 0), (capi.YUV_I420, 6, 7, 0), (capi.YUV_YV12, 3, 3, 0), (capi.YUV_NV12, 5, 8, 0), (capi.YUV_NV21, 6, 7, 0),  # odd 4:2:0
           (capi.YUV_I422, 6, 7, 0), (capi.YUV_YUYV, 6, 7, 0), (capi.YUV_UYVY, 6, 7, 0), (capi.YUV_YVYU, 6, 7, 0),                          # odd 4:2:2 width
           (capi.YUV_I420, 6, 8, 7), (capi.YUV_I444, 6, 8, 6), (capi.YUV_NV12, 6, 8, 6), (capi.YUV_YUYV, 6, 8, 15), (capi.YUV_I420, 6, 8, -8),  # short strides
           (capi.YUV_I420, 6, 8, 9), (capi.YUV_I422, 6, 8, 11), (capi.YUV_I444, 6, 8, 9),                                                   # odd planar strides
           (9, 6, 8, 0), (-1, 6, 8, 0), (17, 6, 8, 0),                                                                                       # unknown names
           (capi.YUV_I444, 0, 8, 0), (capi.YUV_I444, 6, 0, 0)]
    for code, h, w, stride in bad:
        assert _layout(code, h, w, stride)[0] == capi.E_INVALID, (code, h, w, stride)
    assert _layout(capi.YUV_I422, 5, 8)[0] == capi.OK and _layout(capi.YUV_I444, 5, 7, 8)[0] == capi.OK and _layout(capi.YUV_UYVY, 5, 8)[0] == capi.OK
    assert _layout(capi.YUV_NV12, 6, 8, 9)[0] == capi.OK      # an odd stride is a stride for the semi-planar and packed names
    lib, d, fb = capi.load(), capi.YuvDesc(), C.c_int64()
    assert lib.acf_hip_yuv_layout(capi.YUV_I420, 6, 8, 0, None, C.byref(fb)) == capi.E_INVALID
    assert lib.acf_hip_yuv_layout(capi.YUV_I420, 6, 8, 0, C.byref(d), None) == capi.E_INVALID
    with pytest.raises(HipError):
        HipDetector.yuv_desc("i420", 5, 8)
    with pytest.raises(HipError):
        HipDetector.yuv_desc("p010", 6, 8)
    d, fb = HipDetector.yuv_desc("I420", 6, 8)
    assert fb == 72 and d.u.offset == 48


# ---------------------------------------------------------------- acf_hip_yuv_extent, by hand

def test_extent_hand_checked():
    # odd sizes, 4:2:0, two frames: 5 x 7 luma, ceil -> 3 x 4 chroma
    d = _desc((0, 100, 8, 1), (40, 100, 4, 1), (52, 100, 4, 1), 1, 1)
    assert _extent(d, 5, 7, 2) == (capi.OK, [0, 40, 52], [100 + 4 * 8 + 6, 40 + 100 + 2 * 4 + 3, 52 + 100 + 2 * 4 + 3])
    assert _extent(d, 5, 7, 2)[2] == [138, 151, 163]
    # stride_n = 0: one frame however many are asked for; 4:2:2 planar of 4 x 8
    d = _desc((0, 0, 8, 1), (32, 0, 4, 1), (48, 0, 4, 1), 1, 0)
    assert _extent(d, 4, 8, 1) == _extent(d, 4, 8, 5) == (capi.OK, [0, 32, 48], [31, 47, 63])
    # negative offsets: U and V allocated below Y; 4:4:4 of 3 x 5 with padded rows
    d = _desc((0, 64, 8, 1), (-1000, 32, 8, 1), (-500, 32, 16, 1), 0, 0)
    assert _extent(d, 3, 5, 3) == (capi.OK, [0, -1000, -500], [2 * 64 + 2 * 8 + 4, -1000 + 64 + 16 + 4, -500 + 64 + 32 + 4])
    # packed 4:2:2 (YUYV of 4 x 4): the luma plane ends one byte before V
    d = _desc((0, 32, 8, 2), (1, 32, 8, 4), (3, 32, 8, 4), 1, 0)
    assert _extent(d, 4, 4, 1) == (capi.OK, [0, 1, 3], [30, 29, 31])
    assert _extent(d, 4, 3, 1) == (capi.OK, [0, 1, 3], [28, 29, 31])   # odd width: Y1 of the last macropixel is not addressed
    assert HipDetector.yuv_extent(d, 4, 4, 2) == ([0, 1, 3], [62, 61, 63])


def test_extent_refusals():
    ok = ((0, 32, 8, 1), (32, 32, 4, 1), (48, 32, 4, 1))
    good = _desc(*ok, 1, 1)
    assert _extent(good, 4, 8, 1)[0] == capi.OK
    for sx, sy in ((2, 0), (0, 2), (-1, 0), (1, -1)):
        assert _extent(_desc(*ok, sx, sy), 4, 8, 1)[0] == capi.E_INVALID, (sx, sy)
    for i in range(3):
        for bad in ((0, 32, 8, 0), (0, 32, 0, 1), (0, -32, 8, 1), (0, 32, -8, 1)):
            planes = list(ok)
            planes[i] = bad
            assert _extent(_desc(*planes, 1, 1), 4, 8, 1)[0] == capi.E_INVALID, (i, bad)
    for h, w, n in ((0, 8, 1), (4, 0, 1), (4, 8, 0)):
        assert _extent(good, h, w, n)[0] == capi.E_INVALID
    lib, arr = capi.load(), (C.c_int64 * 3)()
    assert lib.acf_hip_yuv_extent(None, 4, 8, 1, arr, arr) == capi.E_INVALID
    assert lib.acf_hip_yuv_extent(C.byref(good), 4, 8, 1, None, arr) == capi.E_INVALID
    assert lib.acf_hip_yuv_extent(C.byref(good), 4, 8, 1, arr, None) == capi.E_INVALID


# ---------------------------------------------------------------- the numpy helper itself

def test_helper_converts_like_the_nv12_restatement():
    """The gather + conversion of an NV12 descriptor equals tests/yuv420_ref.py's nv_to_rgb on the same bytes; I420 of the same
    planes gives the same picture."""
    import yuv420_ref as yr
    rows, cols = 6, 8
    Y, U, V = ydr.random_planes(4, "nv12", rows, cols)
    for name, nv21 in (("nv12", False), ("nv21", True)):
        buf = ydr.pack(name, Y, U, V)
        _, d, _ = _layout(capi.YUV_NAMES[name], rows, cols)
        assert np.array_equal(ydr.desc_to_rgb(buf, d, rows, cols)[0], yr.nv_to_rgb(buf, rows, cols, nv21))
    want = yr.nv_to_rgb(ydr.pack("nv12", Y, U, V), rows, cols)
    for name in ("i420", "yv12"):
        _, d, _ = _layout(capi.YUV_NAMES[name], rows, cols)
        assert np.array_equal(ydr.desc_to_rgb(ydr.pack(name, Y, U, V), d, rows, cols)[0], want), name


# ---------------------------------------------------------------- the boundary

def test_header_declares_the_entries_and_the_abi_stays_9():
    hdr = open(os.path.join(ROOT, "include", "acf_hip.h")).read()
    names = ["acf_hip_pyramid_yuv", "acf_hip_run_yuv", "acf_hip_yuv_to_rgb8", "acf_hip_yuv_extent", "acf_hip_yuv_layout", "acf_hip_stream_open_yuv"]
    lib = capi.load()
    for n in names:
        assert re.search(r"ACF_HIP_API\s+int\s+%s\s*\(" % n, hdr), n
        assert n in capi.DECLARED_SYMBOLS and hasattr(lib, n), n
        for f in ("acf_hip_loader.h", "acf_hip_loader.cpp"):
            assert "ACF_HIP_FN(%s)" % n in open(os.path.join(ROOT, "acf_amd", "host", f)).read(), (n, f)
    assert "typedef struct acf_hip_yuv_plane" in hdr and "typedef struct acf_hip_yuv_desc" in hdr
    assert re.search(r"#define\s+ACF_HIP_ABI_VERSION\s+9\b", hdr) and lib.acf_hip_abi_version() == 9
    assert C.sizeof(capi.YuvPlane) == 32 and C.sizeof(capi.YuvDesc) == 104
    # the ACF_HIP_PIX_* enum is untouched: 7 is still no layout of the 8-bit entries
    out = C.c_int64()
    assert lib.acf_hip_u8_frame_bytes(7, 4, 4, 0, C.byref(out)) == capi.E_INVALID
