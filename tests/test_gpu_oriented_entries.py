"""The oriented entries on the GPU (include/acf_hip.h: acf_hip_pyramid_image_oriented / run_image_oriented / pyramid_yuv_oriented /
run_yuv_oriented / stream_open_yuv_oriented; HipDetector's orient= keyword).

The expected result of a rotated or mirrored frame is what the existing entries give for the frame turned upright by numpy
(tests/orient_ref.py): for uint8 images and YUV frames run_u8 on the oriented R, G, B bytes, for float images run_tensor on the
oriented tight tensor.  Every comparison is an equality of bytes or of uint32 views; every reference holds at least one detection a
frame (tests/test_oriented_entries.py checks the same on the CPU, by the oracle alone, for every model, size and frame class here).
"""
import ctypes as C
import os
import sys

import numpy as np
import pytest

import image_entry_case as iec
import orient_ref as orf
import oriented_case as oc
import yuv_desc_ref as ydr
from acf_amd import capi

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CODES = list(range(8))
N = oc.N_FRAMES


def bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def snapshot(det, nF=N):
    """Per frame (levels, detections bytes, hits bytes) of the last run."""
    out = []
    for f in range(nF):
        d, h = det.detections(f)
        out.append(([bits(det.read_level(f, i)) for i in range(len(det.levels))], d.tobytes(), h.tobytes()))
    return out


def same(got, want, tag):
    assert len(got) == len(want), tag
    for f, ((gl, gd, gh), (wl, wd, wh)) in enumerate(zip(got, want)):
        assert len(gl) == len(wl) and len(wl) > 0, tag
        for i, (a, b) in enumerate(zip(gl, wl)):
            assert np.array_equal(a, b), (tag, f, "level", i)
        assert gd == wd and gh == wh, (tag, f)


def dev(buf):
    import torch
    return torch.from_numpy(np.ascontiguousarray(buf)).cuda()


@pytest.fixture(scope="module")
def dets():
    """Detectors by (model, upright h, w, input planes, options), made once."""
    from acf_amd.detector import HipDetector
    cache = {}

    def get(mkey, h, w, d_in=3, **kw):
        key = (mkey, h, w, d_in, tuple(sorted(kw.items())))
        if key not in cache:
            cache[key] = HipDetector(oc.model(mkey), h, w, d_in, max_batch=N, max_hits=1 << 16, **kw)
        return cache[key]
    yield get
    for d in cache.values():
        d.close()


_REF = {}


def nonvacuous(snap, tag):
    assert all(len(s[1]) > 0 for s in snap), ("a reference frame without detections: the comparison would be vacuous", tag)
    return snap


def want_u8(dets, mkey, size, klass, code):
    """The snapshot of run_u8 on the numpy-oriented bytes: klass (sub_x, sub_y) -> PIX_RGB of the converted planes, "gray" -> PIX_GRAY."""
    key = (mkey, size, klass, code)
    if key not in _REF:
        if klass == "gray":
            up = np.ascontiguousarray(orf.orient(oc.rgb_source(size, (0, 0))[..., 1], code, axes=(1, 2)))
        else:
            up = np.ascontiguousarray(orf.orient(oc.rgb_source(size, klass), code, axes=(1, 2)))
        det = dets(mkey, up.shape[1], up.shape[2], 1 if klass == "gray" else 3)
        x = dev(up)                                                       # (alive until the snapshot has synchronised)
        det.run_u8(x, capi.PIX_GRAY if klass == "gray" else capi.PIX_RGB)
        _REF[key] = nonvacuous(snapshot(det), key)
    return _REF[key]


def want_float(dets, mkey, size, dtype, code):
    """The snapshot of run_tensor on the numpy-oriented tight tensor of a float type."""
    key = (mkey, size, dtype, code)
    if key not in _REF:
        stored = oc.stored_float(size, dtype)[0]
        up = np.ascontiguousarray(orf.orient(stored, code, axes=(2, 3)))
        det = dets(mkey, up.shape[2], up.shape[3])
        t = iec.to_device(up.ravel(), dtype)
        det.run_tensor(t.view(up.shape))
        _REF[key] = nonvacuous(snapshot(det), key)
    return _REF[key]


def profiled(det, fn):
    """The kernel names option "profile" reports for fn()."""
    det.set_option("profile", 1)
    try:
        det.profile()
        fn()
        return set(det.profile())
    finally:
        det.set_option("profile", 0)


def ingest_names(names):
    return sorted(n for n in names if n.startswith("k_ingest"))


def form_name(kind, fast, code):
    return "k_ingest_%s_oriented_%s" % (kind, ("cols" if code & 1 else "rows") if fast else "generic")


# ---------------------------------------------------------------- tensors

def _float_src(size, dtype):
    return oc.stored_float(size, dtype)[0]                                                   # [n][3][rows][cols]


def _u8_src(size):
    return np.ascontiguousarray(oc.rgb_source(size, (0, 0)).transpose(0, 3, 1, 2))          # [n][3][rows][cols]


def _layouts(size):
    """id -> (model, dtype, source elements [n][c][rows][cols], strides, base element, buffer elements or None, fast form expected,
    reference class).  Padded rows are a multiple of four elements (180), so every row start stays one."""
    R, Cc = size
    P = (Cc + 7) // 4 * 4 if Cc % 4 else Cc + 4
    u8 = _u8_src(size)
    return {
        "nchw_f32": ("inria", capi.T_F32, _float_src(size, capi.T_F32), (3 * R * P, R * P, P, 1), 0, None, True, capi.T_F32),
        "channels_last_u8": ("inria", capi.T_U8, u8, (R * Cc * 3, 1, Cc * 3, 3), 0, None, True, (0, 0)),
        "packed_bgr_u8": ("inria", capi.T_U8, u8, (R * Cc * 3, -1, Cc * 3, 3), 2, None, True, (0, 0)),
        "rgba_alpha_skipped_u8": ("inria", capi.T_U8, u8, (R * Cc * 4, 1, Cc * 4, 4), 0, N * R * Cc * 4, True, (0, 0)),
        "f16_padded_rows": ("inria", capi.T_F16, _float_src(size, capi.T_F16), (3 * R * P, R * P, P, 1), 0, None, True, capi.T_F16),
        "bf16_padded_rows": ("inria", capi.T_BF16, _float_src(size, capi.T_BF16), (3 * R * P, R * P, P, 1), 0, None, True, capi.T_BF16),
        # the view [:, :, 3:3 + R, 1:1 + Cc] of a larger surface: aligned strides, a first element that is not
        "window_unaligned_f32": ("inria", capi.T_F32, _float_src(size, capi.T_F32), (3 * (R + 8) * (P + 24), (R + 8) * (P + 24), P + 24, 1), 3 * (P + 24) + 1,
                                 N * 3 * (R + 8) * (P + 24), False, capi.T_F32),
        "gray_one_plane_u8": ("face64", capi.T_U8, u8[:, 1:2], (R * P, 0, P, 1), 0, None, True, "gray"),
        # the store phase's other two conversions behind load forms the rows above do not take them through: packed f16 pixels into a
        # model that takes its planes as they are; every second bf16 element of a row (element-wise loads) into rgb2gray on three planes
        "packed_f16_isluv": ("tiny", capi.T_F16, _float_src(size, capi.T_F16), (R * Cc * 3, 1, Cc * 3, 3), 0, None, True, capi.T_F16),
        "stride2_bf16_gray": ("face64", capi.T_BF16, _float_src(size, capi.T_BF16), (3 * R * Cc * 2, R * Cc * 2, Cc * 2, 2), 0, None, False, capi.T_BF16),
    }


LAYOUT_IDS = ["nchw_f32", "channels_last_u8", "packed_bgr_u8", "rgba_alpha_skipped_u8", "f16_padded_rows", "bf16_padded_rows", "window_unaligned_f32",
              "gray_one_plane_u8", "packed_f16_isluv", "stride2_bf16_gray"]


def _run_layout(dets, size, lid, code, entry="run"):
    """The oriented image entry on one layout -> (detector, expected snapshot, profile names, expected form name)."""
    mkey, dtype, src, strides, base, total, fast, klass = _layouts(size)[lid]
    ch = src.shape[1]
    h, w = orf.dims(size[0], size[1], code)
    det = dets(mkey, h, w, ch)
    want = want_u8(dets, mkey, size, klass, code) if isinstance(klass, (tuple, str)) else want_float(dets, mkey, size, klass, code)
    t = iec.to_device(iec.lay_out(src, dtype, strides, base, total), dtype)
    desc = capi.ImageDesc(dtype, ch, *strides)
    lo, hi = det.image_extent(desc, size[0], size[1], N)
    assert base + lo >= 0 and base + hi < t.numel()                       # the extent at src_rows x src_cols is what is read
    fn = det.run_image_oriented if entry == "run" else det.pyramid_image_oriented
    names = profiled(det, lambda: fn(t.data_ptr() + base * t.element_size(), N, desc, size[0], size[1], code))
    det.synchronize()
    return det, want, names, form_name("image", fast, code)


@pytest.mark.parametrize("code", CODES)
@pytest.mark.parametrize("lid", LAYOUT_IDS)
def test_tensor_layouts_three_tiles_each_way(dets, lid, code):
    """Source 130 x 174 (upright 174 x 130 for odd rot): every layout in every orientation, and the load form it is there for."""
    det, want, names, form = _run_layout(dets, oc.TILES3, lid, code)
    same(snapshot(det), want, (lid, code))
    if code == 0:
        assert ingest_names(names) == ["k_ingest_image"], names         # code 0 is the un-oriented entry: today's kernel names
    else:
        assert ingest_names(names) == [form], (names, form)


def test_run_tensor_orient_keyword(dets):
    """The torch wrapper: an NCHW float tensor with padded rows and a channels_last uint8 tensor, orient=3 and orient=5."""
    import torch
    R, Cc = oc.TILES3
    for code in (3, 5):
        h, w = orf.dims(R, Cc, code)
        det = dets("inria", h, w)
        src = _float_src(oc.TILES3, capi.T_F32)
        big = torch.full((N, 3, R, 176), float("nan"), device="cuda")
        big[..., :Cc] = dev(src)
        det.run_tensor(big[..., :Cc], orient=code)
        same(snapshot(det), want_float(dets, "inria", oc.TILES3, capi.T_F32, code), ("nchw", code))
        x = dev(oc.rgb_source(oc.TILES3, (0, 0)))                         # [n][rows][cols][3]
        det.pyramid_tensor(x, layout="nhwc", orient=code)
        det.detect()
        same(snapshot(det), want_u8(dets, "inria", oc.TILES3, (0, 0), code), ("nhwc", code))
    assert det.oriented_dims(R, Cc, 5) == (Cc, R)


@pytest.mark.parametrize("code", CODES)
@pytest.mark.parametrize("lid", ["channels_last_u8", "nchw_f32", "window_unaligned_f32"])
def test_tensor_odd_source_size(dets, lid, code):
    """131 x 175: H * W % 4 == 1 (the scalar rgb2luv body), a row tail of three elements, scalar plane stores."""
    det, want, names, form = _run_layout(dets, oc.ODD, lid, code)
    same(snapshot(det), want, (lid, code))
    if code:
        assert ingest_names(names) == [form], (names, form)


@pytest.mark.parametrize("code", CODES)
@pytest.mark.parametrize("lid", ["packed_f16_isluv", "stride2_bf16_gray"])
def test_tensor_layouts_with_float4_stores(dets, lid, code):
    """132 x 136: the pass-through and grey layouts of the table again where H % 4 == 0 in every orientation."""
    det, want, names, form = _run_layout(dets, oc.VEC3, lid, code)
    same(snapshot(det), want, (lid, code))
    if code:
        assert ingest_names(names) == [form], (names, form)


# ---------------------------------------------------------------- YUV

def batch(name, planes, stride=0):
    """The frames of `planes` in the named layout back to back -> (flat buffer, descriptor, frame bytes)."""
    from acf_amd.detector import HipDetector
    rows, cols = planes[0][0].shape
    d, fb = HipDetector.yuv_desc(name, rows, cols, stride)
    buf = np.concatenate([ydr.pack(name, Y, U, V, stride) for Y, U, V in planes])
    assert buf.size == fb * len(planes)
    return buf, d, fb


def yuv_fast(d):
    """Whether a description (at a 256-aligned base) meets a wide load form's conditions: everything four-aligned."""
    planes = (d.y, d.u, d.v)
    if d.y.stride_px == 2:
        offs = [min(p.offset for p in planes)]                            # one plane of macropixels
    elif d.u.stride_px == 2:
        offs = [d.y.offset, min(d.u.offset, d.v.offset)]                  # luma, and one plane of chroma pairs
    else:
        offs = [p.offset for p in planes]
    return all(o % 4 == 0 for o in offs) and all(p.stride_row % 4 == 0 and p.stride_n % 4 == 0 for p in planes)


def _run_yuv(dets, mkey, size, sub, buf, d, code, lead=0):
    """run_yuv_oriented on a buffer -> (detector, expected snapshot, profile names)."""
    h, w = orf.dims(size[0], size[1], code)
    det = dets(mkey, h, w)
    want = want_u8(dets, mkey, size, sub, code)
    assert np.array_equal(ydr.desc_to_rgb(buf, d, size[0], size[1], N, lead), oc.rgb_source(size, sub))   # the buffer holds the planes
    lo, hi = det.yuv_extent(d, size[0], size[1], N)
    assert lead + min(lo) >= 0 and lead + max(hi) < buf.size
    x = dev(buf)
    names = profiled(det, lambda: det.run_yuv(x.data_ptr() + lead, N, d, code, size[0], size[1]))
    det.synchronize()
    return det, want, names


@pytest.mark.parametrize("padded", [False, True], ids=["tight", "padded"])
@pytest.mark.parametrize("name", ydr.NAMES)
def test_named_yuv_layouts_in_every_orientation(dets, name, padded):
    """The nine named layouts at 130 x 174, tight and with rows padded to four-aligned strides, all eight codes."""
    sub = ydr.SUB[name]
    size = oc.TILES3
    stride = 0 if not padded else (352 if name in ydr.PACKED_ORDER else 192 if name not in ("nv12", "nv21") else 176)
    buf, d, fb = batch(name, oc.yuv_planes(size, sub), stride)
    fast = yuv_fast(d)
    assert fast or not padded                                             # the padded strides are there for the wide forms
    if not padded and name not in ydr.PACKED_ORDER:
        assert not fast                                                   # rows of 174 bytes: the byte form
    for code in CODES:
        det, want, names = _run_yuv(dets, "inria", size, sub, buf, d, code)
        same(snapshot(det), want, (name, padded, code))
        if code == 0:
            assert not [n for n in names if "oriented" in n], names       # today's kernel names
        else:
            assert ingest_names(names) == [form_name("yuv", fast, code)], (name, padded, code, names)


def test_three_separate_allocations_with_negative_offsets(dets):
    import torch
    size = oc.TILES3
    planes = oc.yuv_planes(size, (1, 1))
    Y, U, V = (np.stack([p[i] for p in planes]) for i in range(3))       # [n][rows][cols] each
    arena = torch.empty(V.size + U.size + Y.size + 64, dtype=torch.uint8, device="cuda")    # V and U below Y
    v = arena[:V.size].view(V.shape)
    u = arena[V.size:V.size + U.size].view(U.shape)
    y = arena[V.size + U.size:V.size + U.size + Y.size].view(Y.shape)
    v.copy_(dev(V)), u.copy_(dev(U)), y.copy_(dev(Y))
    torch.cuda.synchronize()
    for code in CODES:
        h, w = orf.dims(size[0], size[1], code)
        det = dets("inria", h, w)
        base, n, d = det.yuv_planes_desc(y, u, v, 1, 1)
        assert n == N and d.u.offset < 0 and d.v.offset < 0
        det.run_yuv_planes(y, u, v, 1, 1, orient=code)
        same(snapshot(det), want_u8(dets, "inria", size, (1, 1), code), ("separate planes", code))


ODD_CASES = {
    # id: (sub, builder(planes) -> (buf, d, fb), fast)
    "i420_byte_loads": ((1, 1), lambda p: oc.planar_buffer(p, 175, 88, (1, 1)), False),
    "i420_dword_loads": ((1, 1), lambda p: oc.planar_buffer(p, 176, 88, (1, 1)), True),
    "i422_dword_loads": ((1, 0), lambda p: oc.planar_buffer(p, 176, 88, (1, 0)), True),
    "yuyv_half_macropixel": ((1, 0), lambda p: oc.yuyv_buffer(p, 352), True),
    "yuyv_from_an_odd_base": ((1, 0), lambda p: oc.yuyv_buffer(p, 352, lead=1), False),
    # a fourth field: the model, where it is not "inria" — rgb2gray behind a wide and behind the element-wise load form
    "i420_gray_dword_loads": ((1, 1), lambda p: oc.planar_buffer(p, 176, 88, (1, 1)), True, "face64"),
    "yuyv_gray_from_an_odd_base": ((1, 0), lambda p: oc.yuyv_buffer(p, 352, lead=1), False, "face64"),
    # a fifth field: the source size, where it is not 131 x 175 — the grey model with float4 stores
    "i420_gray_float4_stores": ((1, 1), lambda p: oc.planar_buffer(p, 136, 68, (1, 1)), True, "face64", oc.VEC3),
}


@pytest.mark.parametrize("case", sorted(ODD_CASES))
def test_yuv_odd_source_size(dets, case):
    """131 x 175 with 66 x 88 (4:2:0) and 131 x 88 (4:2:2) chroma planes: the chroma sample of a reversed odd axis is
    (Hs - 1 - c) >> 1, which no strided view of the upright frame gives; H * W % 4 == 1: the scalar rgb2luv body."""
    sub, build, fast = ODD_CASES[case][:3]
    mkey = (ODD_CASES[case] + ("inria",))[3]
    size = ODD_CASES[case][4] if len(ODD_CASES[case]) > 4 else oc.ODD
    buf, d, fb = build(oc.yuv_planes(size, sub))
    lead = 1 if case.endswith("odd_base") else 0
    for code in CODES:
        det, want, names = _run_yuv(dets, mkey, size, sub, buf, d, code, lead)
        same(snapshot(det), want, (case, code))
        if code:
            assert ingest_names(names) == [form_name("yuv", fast, code)], (case, code, names)


@pytest.mark.parametrize("code", CODES)
def test_one_tile_or_less_along_an_axis(dets, code):
    """Source 40 x 203 (upright 203 x 40 for odd rot) with a 16 x 16 model: hand-built I420 (20 x 102 chroma) and channels_last uint8."""
    size = oc.THIN
    buf, d, fb = oc.planar_buffer(oc.yuv_planes(size, (1, 1)), 204, 104, (1, 1))
    det, want, names = _run_yuv(dets, "tiny", size, (1, 1), buf, d, code)
    same(snapshot(det), want, ("i420", code))
    if code:
        assert ingest_names(names) == [form_name("yuv", True, code)], names
    # the same model behind the other two load forms: tight odd strides (byte loads), hand-packed YUYV with half a macropixel at the row end
    buf, d, fb = oc.planar_buffer(oc.yuv_planes(size, (1, 1)), 203, 102, (1, 1))
    det, want, names = _run_yuv(dets, "tiny", size, (1, 1), buf, d, code)
    same(snapshot(det), want, ("i420 bytes", code))
    if code:
        assert ingest_names(names) == [form_name("yuv", False, code)], names
    buf, d, fb = oc.yuyv_buffer(oc.yuv_planes(size, (1, 0)), 408)
    det, want, names = _run_yuv(dets, "tiny", size, (1, 0), buf, d, code)
    same(snapshot(det), want, ("yuyv", code))
    if code:
        assert ingest_names(names) == [form_name("yuv", True, code)], names
    x = dev(oc.rgb_source(size, (0, 0)))
    det.run_tensor(x, layout="nhwc", orient=code)
    same(snapshot(det), want_u8(dets, "tiny", size, (0, 0), code), ("channels_last", code))


# ---------------------------------------------------------------- code 0, the arithmetic tier, pyramid + detect, the tap

def test_code_0_is_the_unoriented_entry(dets):
    size = oc.TILES3
    det = dets("inria", *size)
    buf, d, fb = batch("i420", oc.yuv_planes(size, (1, 1)), 192)
    x = dev(buf)
    det.run_yuv(x, N, d)
    a = nonvacuous(snapshot(det), "run_yuv")
    names = profiled(det, lambda: det.run_yuv(x, N, d, 0, size[0], size[1]))     # acf_hip_run_yuv_oriented with code 0
    same(snapshot(det), a, "yuv, code 0")
    assert ingest_names(names) == ["k_ingest_yuv_planar"], names
    rgb = dev(oc.rgb_source(size, (0, 0)))
    desc = capi.ImageDesc(capi.T_U8, 3, size[0] * size[1] * 3, 1, size[1] * 3, 3)
    det.run_image(rgb.data_ptr(), N, desc)
    b = nonvacuous(snapshot(det), "run_image")
    names = profiled(det, lambda: det.run_image_oriented(rgb.data_ptr(), N, desc, size[0], size[1], 0))
    same(snapshot(det), b, "image, code 0")
    assert ingest_names(names) == ["k_ingest_image"], names


@pytest.mark.parametrize("code", [0, 3])
def test_reference_arithmetic_tier(oracle, code):
    """Option "arith" = 1 with the committed x86 tables: one image and one YUV case against run_u8 under the same option."""
    from acf_amd.detector import HipDetector
    size = oc.TILES3
    h, w = orf.dims(size[0], size[1], code)
    det = HipDetector(oc.model("inria"), h, w, 3, max_batch=N, max_hits=1 << 16)
    up = dev(np.ascontiguousarray(orf.orient(oc.rgb_source(size, (1, 1)), code, axes=(1, 2))))
    det.run_u8(up, capi.PIX_RGB)
    exact = snapshot(det)
    det.set_x86_tables(*oracle.x86_fixture())
    det.set_option("arith", 1)
    det.run_u8(up, capi.PIX_RGB)
    want = nonvacuous(snapshot(det), "arith")
    assert any(not np.array_equal(a, b) for a, b in zip(want[0][0], exact[0][0]))            # (the tier is not a no-op)
    buf, d, fb = batch("nv12", oc.yuv_planes(size, (1, 1)), 176)
    x = dev(buf)
    det.run_yuv(x, N, d, code, size[0], size[1])
    same(snapshot(det), want, ("yuv arith", code))
    src = dev(oc.rgb_source(size, (1, 1)))
    det.run_tensor(src, layout="nhwc", orient=code) if code else det.run_image_oriented(
        src.data_ptr(), N, capi.ImageDesc(capi.T_U8, 3, size[0] * size[1] * 3, 1, size[1] * 3, 3), size[0], size[1], 0)
    same(snapshot(det), want, ("image arith", code))
    det.close()


def test_pyramid_then_detect_equals_run_and_the_image_tap(dets):
    size = oc.TILES3
    for code in (1, 6):
        h, w = orf.dims(size[0], size[1], code)
        det = dets("inria", h, w, taps=True)
        up = dev(np.ascontiguousarray(orf.orient(oc.rgb_source(size, (1, 1)), code, axes=(1, 2))))
        det.pyramid_u8(up, capi.PIX_RGB)
        first = next(l for l in det.levels if l.isReal)                  # the image of the first real scale: whole cells of the frame
        shape = (3, first.wC * oc.model("inria")["shrink"], first.hC * oc.model("inria")["shrink"])
        tap = [det.read_tap(f, capi.TAP_IMAGE, 0, shape) for f in range(N)]
        assert all(np.any(t) for t in tap)
        det.detect()
        want = nonvacuous(snapshot(det), "taps")
        buf, d, fb = batch("i420", oc.yuv_planes(size, (1, 1)), 192)
        x = dev(buf)
        det.pyramid_yuv(x, N, d, code, size[0], size[1])
        for f in range(N):
            assert np.array_equal(bits(det.read_tap(f, capi.TAP_IMAGE, 0, shape)), bits(tap[f])), (code, f)
        det.detect()
        same(snapshot(det), want, ("pyramid_yuv + detect", code))
        det.run_yuv(x, N, d, code, size[0], size[1])
        same(snapshot(det), want, ("run_yuv", code))
        src = dev(oc.rgb_source(size, (1, 1)))
        det.pyramid_tensor(src, layout="nhwc", orient=code)
        for f in range(N):
            assert np.array_equal(bits(det.read_tap(f, capi.TAP_IMAGE, 0, shape)), bits(tap[f])), (code, f)
        det.detect()
        same(snapshot(det), want, ("pyramid_tensor + detect", code))


# ---------------------------------------------------------------- streaming

@pytest.mark.parametrize("code", [1, 6])
def test_stream_of_oriented_frames_matches_blocking_calls(code):
    """Two batches through a depth-2 stream give the records of run_yuv(orient) + export_detections of each batch."""
    import torch
    from acf_amd.detector import HipDetector, PinnedBuffer
    size, cap, depth = oc.TILES3, 512, 2
    h, w = orf.dims(size[0], size[1], code)
    det = HipDetector(oc.model("inria"), h, w, 3, max_batch=N, max_hits=4096)
    planes = oc.yuv_planes(size, (1, 1))
    buf, d, fb = batch("nv12", planes, 176)
    batches = [buf.reshape(N, fb), np.ascontiguousarray(buf.reshape(N, fb)[::-1])]
    want = []
    for x in batches:
        xd = dev(x)
        det.run_yuv(xd, N, d, code, size[0], size[1])
        dst = torch.zeros((N, 1 + 6 * cap), dtype=torch.int32, device="cuda")
        torch.cuda.synchronize()                                          # (torch fills dst on its own stream: before the export writes it)
        det.export_detections(dst, cap)
        det.synchronize()
        want.append(dst.cpu().numpy())
    assert all((x[:, 0] > 0).all() for x in want)
    pins = [PinnedBuffer(N * fb) for _ in range(depth)]
    det.stream_open_yuv(d, fb, cap, depth, orient=code, src_rows=size[0], src_cols=size[1])
    tickets = []
    for b, x in enumerate(batches):
        pins[b].array[:x.size] = x.ravel()
        tickets.append(det.stream_submit(pins[b].ptr.value, N))
    got = [det.stream_collect(t) for t in tickets]
    for b in range(2):
        for f in range(N):
            n = want[b][f, 0]
            assert got[b][f, 0] == n
            assert np.array_equal(got[b][f, :1 + 6 * n], want[b][f, :1 + 6 * n]), (b, f)
    det.stream_close()
    det.close()
    for p in pins:
        p.close()


# ---------------------------------------------------------------- what is refused

def test_refusals_leave_the_context_usable():
    import torch
    from acf_amd.detector import HipDetector, HipError
    model = oc.model("tiny")
    R, Cc = 96, 128                                                       # the stored frame; upright 128 x 96 for odd rot
    x = torch.zeros(4 * R * Cc * 3, dtype=torch.uint8).cuda()             # room for every call below, were it not refused
    good, fb = HipDetector.yuv_desc("i420", R, Cc)
    img = capi.ImageDesc(capi.T_U8, 3, R * Cc * 3, 1, Cc * 3, 3)

    def refused(fn, code=capi.E_INVALID):
        with pytest.raises(HipError) as e:
            fn()
        assert e.value.code == code, e.value

    det = HipDetector(model, Cc, R, 3, max_batch=2)                       # the plan of codes 1, 3, 5, 7

    def works():
        det.run_yuv(x, 2, good, 1, R, Cc)
        det.run_image_oriented(x.data_ptr(), 2, img, R, Cc, 3)
        det.synchronize()
    works()
    for bad in (-1, 8, 100):
        refused(lambda: det.run_yuv(x, 1, good, bad, R, Cc))
        refused(lambda: det.pyramid_yuv(x, 1, good, bad, R, Cc))
        refused(lambda: det.run_image_oriented(x.data_ptr(), 1, img, R, Cc, bad))
        refused(lambda: det.pyramid_image_oriented(x.data_ptr(), 1, img, R, Cc, bad))
        refused(lambda: det.stream_open_yuv(good, fb, 64, 2, orient=bad, src_rows=R, src_cols=Cc))
    for rows, cols in ((0, Cc), (R, 0), (-R, Cc)):
        refused(lambda: det.run_yuv(x, 1, good, 1, rows, cols))
        refused(lambda: det.run_image_oriented(x.data_ptr(), 1, img, rows, cols, 1))
        refused(lambda: det.stream_open_yuv(good, fb, 64, 2, orient=1, src_rows=rows, src_cols=cols))
    # a plan whose h x w is not oriented_dims(...): even codes on this plan (code 0 included), a frame of another size
    for code in (0, 2, 4, 6):
        refused(lambda: det.run_yuv(x, 1, good, code, R, Cc))
        refused(lambda: det.run_image_oriented(x.data_ptr(), 1, img, R, Cc, code))
        refused(lambda: det.stream_open_yuv(good, fb, 64, 2, orient=code, src_rows=R, src_cols=Cc))
    refused(lambda: det.run_yuv(x, 1, good, 1, R, Cc - 2))
    refused(lambda: det.run_image_oriented(x.data_ptr(), 1, img, R - 1, Cc, 1))
    # whatever the un-oriented entry refuses: null pointers, the batch size, a bad description
    lib = det.lib
    assert lib.acf_hip_run_yuv_oriented(det.ctx, None, 1, C.byref(good), R, Cc, 1) == capi.E_INVALID
    assert lib.acf_hip_run_yuv_oriented(det.ctx, C.c_void_p(x.data_ptr()), 1, None, R, Cc, 1) == capi.E_INVALID
    assert lib.acf_hip_run_image_oriented(det.ctx, None, 1, C.byref(img), R, Cc, 1) == capi.E_INVALID
    assert lib.acf_hip_pyramid_image_oriented(None, C.c_void_p(x.data_ptr()), 1, C.byref(img), R, Cc, 1) == capi.E_INVALID
    refused(lambda: det.run_yuv(x, 3, good, 1, R, Cc))                    # max_batch is 2
    refused(lambda: det.run_yuv(x, 0, good, 1, R, Cc))
    bad_yuv = capi.YuvDesc.from_buffer_copy(good)
    bad_yuv.u.stride_px = -1
    refused(lambda: det.run_yuv(x, 1, bad_yuv, 1, R, Cc))
    refused(lambda: det.stream_open_yuv(bad_yuv, fb, 64, 2, orient=1, src_rows=R, src_cols=Cc))
    refused(lambda: det.run_image_oriented(x.data_ptr(), 1, capi.ImageDesc(capi.T_U8, 3, R * Cc * 3, 1, -Cc * 3, 3), R, Cc, 1))
    refused(lambda: det.run_image_oriented(x.data_ptr(), 1, capi.ImageDesc(capi.T_U8, 1, R * Cc, 0, Cc, 1), R, Cc, 1))      # channels != d
    # the stream's own rules, with the extents at src_rows x src_cols
    refused(lambda: det.stream_open_yuv(good, fb - 1, 64, 2, orient=1, src_rows=R, src_cols=Cc))
    refused(lambda: det.stream_open_yuv(good, fb, 64, 1, orient=1, src_rows=R, src_cols=Cc))
    works()
    # an active input resize
    small = HipDetector(model, *HipDetector.resize_dims(192, 256, 0.5), 3, max_batch=1)                 # 96 x 128
    small.set_input_resize(192, 256, 0.5)
    refused(lambda: small.run_yuv(x, 1, good, 2, R, Cc))
    refused(lambda: small.run_image_oriented(x.data_ptr(), 1, img, R, Cc, 2))
    refused(lambda: small.stream_open_yuv(good, fb, 64, 2, orient=2, src_rows=R, src_cols=Cc))
    small.set_input_resize(0, 0, 1.0)
    small.run_yuv(x, 1, good, 2, R, Cc)                                   # ... and accepted once it is off
    small.synchronize()
    small.close()
    # a five-plane plan; no plan; sub-batch contexts
    five = HipDetector(model, Cc, R, 5, max_batch=1)
    refused(lambda: five.run_yuv(x, 1, good, 1, R, Cc))
    refused(lambda: five.run_image_oriented(x.data_ptr(), 1, img, R, Cc, 1))
    five.close()
    bare = HipDetector(model)
    refused(lambda: bare.run_yuv(x, 1, good, 1, R, Cc), capi.E_NOPLAN)
    refused(lambda: bare.run_image_oriented(x.data_ptr(), 1, img, R, Cc, 1), capi.E_NOPLAN)
    refused(lambda: bare.stream_open_yuv(good, fb, 64, 2, orient=1, src_rows=R, src_cols=Cc), capi.E_NOPLAN)
    bare.close()
    multi = HipDetector(model, Cc, R, 3, max_batch=4, streams=2)
    refused(lambda: multi.run_yuv(x, 2, good, 1, R, Cc), capi.E_UNSUPPORTED)
    refused(lambda: multi.run_image_oriented(x.data_ptr(), 2, img, R, Cc, 1), capi.E_UNSUPPORTED)
    refused(lambda: multi.stream_open_yuv(good, fb, 64, 2, orient=1, src_rows=R, src_cols=Cc), capi.E_UNSUPPORTED)
    multi.close()
    works()
    det.close()


# ---------------------------------------------------------------- the C++ host

@pytest.mark.parametrize("mode", [[], ["--stream", "2"]], ids=["detectYuv", "streamOpenYuv"])
def test_cli_orient_matches_the_python_path(tmp_path, mode):
    """acf::HipDetector::setInputOrientation through detectYuv and through streamOpenYuv / streamSubmit (acf_hip_detect --yuv i420
    --orient 1) prints what run_yuv(orient=1) returns, in upright coordinates, and says so."""
    import subprocess
    from acf_amd.detector import HipDetector
    from acf_amd.modelio import write_model
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    from test_host_cpp import parse, run
    host = os.path.join(ROOT, "acf_amd", "host")
    subprocess.check_call(["make", "-s", "-C", host])
    size, code, cnt = oc.TILES3, 1, 3
    h, w = orf.dims(size[0], size[1], code)
    planes = oc.yuv_planes(size, (1, 1))
    planes = [planes[0], planes[1], planes[0]]
    write_model(str(tmp_path / "m.acfm"), oc.model("inria"))
    buf, d, fb = batch("i420", planes)
    (tmp_path / "f.yuv").write_bytes(buf.tobytes())
    p = run(os.path.join(host, "acf_hip_detect"), ["--model", str(tmp_path / "m.acfm"), "--frames", str(tmp_path / "f.yuv"), "--yuv", "i420",
                                                   "--rows", str(size[0]), "--cols", str(size[1]), "--count", str(cnt), "--orient", str(code)] + mode)
    heads = [l for l in p.stdout.splitlines() if l.startswith("frame")]
    assert len(heads) == cnt and all(l.endswith("upright %dx%d orient %d" % (h, w, code)) for l in heads), heads
    got = parse(p.stdout)
    det = HipDetector(oc.model("inria"), h, w, 3, max_batch=cnt, max_hits=1 << 16)
    x = dev(buf)
    det.run_yuv(x, cnt, d, code, size[0], size[1])
    for f in range(cnt):
        dd, _ = det.detections(f)
        py = [(int(r["x"]), int(r["y"]), int(r["w"]), int(r["h"]), int(np.float32(r["score"]).view(np.uint32))) for r in dd]
        assert len(py) > 0 and got[f] == py, f
    # ... and a box mapped back by the C ABI lies where numpy puts it
    r = dd[0]
    box = HipDetector.unorient_boxes(dd[:1], code, size[0], size[1])
    assert [int(box[k][0]) for k in "xywh"] == orf.unorient_box(code, size[0], size[1], [int(r[k]) for k in "xywh"])
    det.close()
