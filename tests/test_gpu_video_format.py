"""Video formats on the GPU (include/acf_hip.h: acf_hip_yuv_format; acf_hip_pyramid_video / run_video / video_to_rgb /
stream_open_video): 9 .. 16-bit samples, BT.709 / BT.2020, full range.

The expected R, G, B come from the numpy restatement (tests/video_format_ref.py: a gather through the descriptor, mask and shift, the
header's formula in int64 with constants derived by fractions.Fraction).  8-bit formats are then what run_u8(PIX_RGB) gives for those
bytes (through numpy's upright frame and the image entries' resize where the call turns or reduces); more than 8 bits what run_image
gives for the packed float32 image float(R) * float(1.0 / out_max).  Every comparison is an equality of bytes or of uint32 views.
"""
import ctypes as C
import os
import sys

import numpy as np
import pytest

import orient_ref as orf
import video_format_ref as vr
import oriented_case as oc
import yuv_desc_ref as ydr
from acf_amd import capi, synth
from test_gpu_yuv_desc import INRIA, batch, dev, rgb_expect, same, snapshot

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

H, W = 130, 174  # three tiles each way, ragged edges, H % 4 == 2
ROWS = [(m, f) for m in (0, 1, 2) for f in (0, 1)]
ROW_IDS = ["%s_%s" % (("bt601", "bt709", "bt2020")[m], ("limited", "full")[f]) for m, f in ROWS]


def F(bits=8, shift=0, matrix=0, full=0):
    return capi.YuvFormat(bits, shift, matrix, full)


def tup(fmt):
    return fmt.bits, fmt.shift, fmt.matrix, fmt.full_range


def nonvacuous(want, tag):
    assert sum(len(w[1]) for w in want) > 0, (tag, "no detections: the cascade comparison would be vacuous")
    return want


def f32_expect(det, rgb, fmt):
    """run_image on the tight packed float32 image of uint16 R, G, B [n][rows][cols][3] -> snapshot."""
    x = dev(vr.rgb_to_f32(rgb, tup(fmt)))
    det.run_tensor(x, layout="nhwc")
    return snapshot(det, rgb.shape[0])


def names_of(det, fn):
    """The profile's kernel names of one call (option "profile" is on)."""
    det.profile()
    fn()
    det.synchronize()
    return set(det.profile())


def video_planes(seed, h, w, sx, sy, bits=8):
    """A video-like frame: Y in limited range, chroma around mid grey, scaled to `bits` bits."""
    p = synth.make_frame(seed, h, w, "rgb").transpose(0, 2, 1)            # [3][h][w] in [0, 1]
    up = 1 << (bits - 8)
    dt = np.uint8 if bits == 8 else np.uint16
    Y = np.rint((16 + 219 * p[0]) * up).astype(dt)
    U = np.rint((128 + 90 * (p[1] - 0.5)) * up).astype(dt)[::1 << sy, ::1 << sx]
    V = np.rint((128 + 90 * (p[2] - 0.5)) * up).astype(dt)[::1 << sy, ::1 << sx]
    return Y, np.ascontiguousarray(U), np.ascontiguousarray(V)


def batch16(name, planes, fmt, stride=0, junk_seed=None):
    """Frames of 16-bit words in the named layout back to back -> (flat uint8 buffer, descriptor, frame bytes).  junk_seed: random
    bits in every word OUTSIDE the sample field, which the mask must drop."""
    from acf_amd.detector import HipDetector
    rows, cols = planes[0][0].shape
    d, fb = HipDetector.video_desc(name, rows, cols, fmt, stride)
    buf = np.concatenate([vr.pack16(name, Y, U, V, fmt.shift, stride) for Y, U, V in planes])
    assert buf.size == fb * len(planes)
    if junk_seed is not None:
        field = np.uint16(((1 << fmt.bits) - 1) << fmt.shift)
        w = buf.view(np.uint16)
        w |= np.random.RandomState(junk_seed).randint(0, 1 << 16, w.size).astype(np.uint16) & ~field
    return buf, d, fb


@pytest.fixture(scope="module")
def det130():
    from acf_amd.detector import HipDetector
    det = HipDetector(synth.make_model(seed=3, **INRIA), H, W, 3, max_batch=2, max_hits=1 << 16)
    yield det
    det.close()


@pytest.fixture(scope="module")
def bare():
    from acf_amd.detector import HipDetector
    det = HipDetector()
    yield det
    det.close()


# ---------------------------------------------------------------- 1. the conversion alone, 8 bits: every (Y, U, V)

_TRIPLES = {}


def _triples():
    if not _TRIPLES:
        idx = np.arange(1 << 24, dtype=np.int32).reshape(4096, 4096)
        Y, U, V = (idx >> 16).astype(np.uint8), ((idx >> 8) & 255).astype(np.uint8), (idx & 255).astype(np.uint8)
        _TRIPLES["yuv"] = (Y, U, V)
        _TRIPLES["dev"] = dev(np.concatenate([Y.ravel(), U.ravel(), V.ravel()]))
    return _TRIPLES["yuv"], _TRIPLES["dev"]


@pytest.mark.parametrize("matrix,full", ROWS, ids=ROW_IDS)
def test_video_to_rgb_8_bits_on_every_triple(bare, matrix, full):
    from acf_amd.detector import HipDetector
    (Y, U, V), x = _triples()
    d, fb = HipDetector.yuv_desc("i444", 4096, 4096)
    got = bare.video_to_rgb(x, 1, 4096, 4096, d, F(8, 0, matrix, full)).cpu().numpy()
    want = vr.to_rgb(Y, U, V, 8, matrix, full).astype(np.uint8)
    assert got.dtype == np.uint8 and np.array_equal(got[0], want)


# ---------------------------------------------------------------- 2. the conversion alone, 10 / 12 / 16 bits

def _lattice(bits):
    cmid, top = 1 << (bits - 1), (1 << bits) - 1
    fixed = [0, 1, cmid - 1, cmid, cmid + 1, top - 1, top]
    spread = [int(v) for v in np.linspace(2, top - 2, 28)[1:-1]]          # 26 values strictly inside
    lat = sorted(set(fixed + spread))
    assert len(lat) == 33
    return np.array(lat, np.int64)


_LATTICE = {}


def _lattice_frame(bits, shift):
    """An I444 frame of words: row u * 33 + v holds every Y against lattice (U, V) = (lat[u], lat[v])."""
    if bits not in _LATTICE:
        lat = _lattice(bits)
        n = 1 << bits
        Y = np.broadcast_to(np.arange(n, dtype=np.uint16) << shift, (33 * 33, n))
        U = np.broadcast_to((np.repeat(lat, 33).astype(np.uint16) << shift)[:, None], (33 * 33, n))
        V = np.broadcast_to((np.tile(lat, 33).astype(np.uint16) << shift)[:, None], (33 * 33, n))
        _LATTICE.clear()                                                  # (one device frame at a time: 16 bits is 428 MB)
        _LATTICE[bits] = (lat, dev(np.concatenate([Y.ravel(), U.ravel(), V.ravel()]).view(np.uint8)))
    return _LATTICE[bits]


@pytest.mark.parametrize("matrix,full", ROWS, ids=ROW_IDS)
@pytest.mark.parametrize("bits", [10, 12, 16])
def test_video_to_rgb_wide_every_luma_against_the_chroma_lattice(bare, bits, matrix, full):
    from acf_amd.detector import HipDetector
    shift = 16 - bits                                                     # the sample in the high bits, as P010 / P012
    fmt = F(bits, shift, matrix, full)
    lat, x = _lattice_frame(bits, shift)
    n = 1 << bits
    d, fb = HipDetector.video_desc("i444", 33 * 33, n, fmt)
    got = bare.video_to_rgb(x, 1, 33 * 33, n, d, fmt).cpu().numpy().view(np.uint16)[0].reshape(33, 33, n, 3)
    yoff, cmid, omax, cy, cvr, cvg, cug, cub = vr.coeffs(bits, matrix, full)
    y = np.maximum(0, np.arange(n, dtype=np.int64) - yoff) * cy + (1 << 19)
    c = lat - cmid
    clip = lambda a: np.clip(a >> 20, 0, omax).astype(np.uint16)
    assert np.array_equal(got[..., 0], np.broadcast_to(clip(y[None, :] + cvr * c[:, None])[None], (33, 33, n)))          # R: (V, Y)
    assert np.array_equal(got[..., 2], np.broadcast_to(clip(y[None, :] + cub * c[:, None])[:, None], (33, 33, n)))       # B: (U, Y)
    assert np.array_equal(got[..., 1], clip(y[None, None, :] + (cvg * c)[None, :, None] + (cug * c)[:, None, None]))     # G: (U, V, Y)
    # the broadcast form above is the helper's formula: held against vr.to_rgb on a slice
    assert np.array_equal(got[5, 7], vr.to_rgb(np.arange(n), lat[5], lat[7], bits, matrix, full))


@pytest.mark.parametrize("matrix,full", ROWS, ids=ROW_IDS)
@pytest.mark.parametrize("bits", [10, 12, 16])
def test_video_to_rgb_wide_random_words_with_bits_outside_the_field(bare, bits, matrix, full):
    rows, cols, shift = 257, 511, (16 - bits) // 2                        # junk below AND above the field (none at 16 bits)
    fmt = F(bits, shift, matrix, full)
    words = np.random.RandomState(1000 + bits).randint(0, 1 << 16, 3 * rows * cols).astype(np.uint16)
    if bits < 16:
        assert (words & np.uint16(~(((1 << bits) - 1) << shift) & 0xFFFF)).any()
    pw = rows * cols * 2
    d = capi.YuvDesc(capi.YuvPlane(0, 3 * pw, cols * 2, 2), capi.YuvPlane(pw, 3 * pw, cols * 2, 2), capi.YuvPlane(2 * pw, 3 * pw, cols * 2, 2), 0, 0)
    got = bare.video_to_rgb(dev(words.view(np.uint8)), 1, rows, cols, d, fmt).cpu().numpy().view(np.uint16)
    assert np.array_equal(got, vr.desc_to_rgb(words.view(np.uint8), d, rows, cols, tup(fmt)))


# ---------------------------------------------------------------- 3. the default format forwards

def _stored(case):
    """(stored rows, cols, orient, scale, plan h, w) of the four families, the plan at 130 x 174 (or turned)."""
    from acf_amd.detector import HipDetector
    orient, scale = case
    sr, sc = (H, W) if not scale else (216, 290)
    if orient & 1:
        sr, sc = sc, sr
    ph, pw = HipDetector.oriented_resized_dims(sr, sc, orient, scale) if scale else HipDetector.oriented_dims(sr, sc, orient)
    return sr, sc, orient, scale, ph, pw


FAMILIES = [(0, None), (5, None), (0, 0.6), (5, 0.6)]
FAMILY_IDS = ["plain", "orient5", "scale06", "orient5_scale06"]


@pytest.mark.parametrize("case", FAMILIES, ids=FAMILY_IDS)
def test_default_format_is_the_existing_entry(case):
    from acf_amd.detector import HipDetector
    sr, sc, orient, scale, ph, pw = _stored(case)
    det = HipDetector(synth.make_model(seed=3, **INRIA), ph, pw, 3, max_batch=2, max_hits=1 << 16)
    planes = [video_planes(300 + f, sr, sc, 1, 1) for f in range(2)]
    buf, d, fb = batch("i420", planes)
    x = dev(buf)
    det.set_option("profile", 1)
    if scale:
        old = lambda: det.run_yuv_resized(x, 2, d, sr, sc, scale, orient)
    else:
        old = lambda: det.run_yuv(x, 2, d, orient, sr, sc) if orient else det.run_yuv(x, 2, d)
    want_names = names_of(det, old)
    want = nonvacuous(snapshot(det, 2), case)
    size = (sr, sc) if (orient or scale) else (None, None)
    for fmt in (None, F(8, 0, capi.YUV_MATRIX_BT601, 0)):
        got_names = names_of(det, lambda: det.run_video(x, 2, d, fmt, size[0], size[1], orient, scale))
        same(snapshot(det, 2), want, (case, fmt is None))
        assert got_names == want_names, (got_names, want_names)
    det.close()


# ---------------------------------------------------------------- 4. 8 bits, other formats

_REF8 = {}


def reference8(det, sx, sy, fmt):
    """Two frames of random planes (every code value), numpy's R, G, B for the format and the RGB entry's result: computed once."""
    key = (sx, sy) + tup(fmt)
    if key not in _REF8:
        name = {(1, 1): "i420", (1, 0): "i422", (0, 0): "i444"}[(sx, sy)]
        planes = [ydr.random_planes(170 + 10 * sx + sy + 100 * f, name, H, W) for f in range(2)]
        rgb = np.stack([vr.to_rgb(Y, ydr.upsample(U, H, W, sx, sy), ydr.upsample(V, H, W, sx, sy), 8, fmt.matrix, fmt.full_range).astype(np.uint8)
                        for Y, U, V in planes])
        _REF8[key] = (planes, rgb, nonvacuous(rgb_expect(det, rgb), key))
    return _REF8[key]


@pytest.mark.parametrize("name", ["i420", "nv12", "yuyv", "i444"])
@pytest.mark.parametrize("fmt", [F(8, 0, 1, 0), F(8, 0, 2, 1)], ids=["bt709_limited", "bt2020_full"])
def test_8_bit_formats_equal_the_rgb_entry(det130, name, fmt):
    det = det130
    sx, sy = ydr.SUB[name]
    planes, rgb, want = reference8(det, sx, sy, fmt)
    buf, d, fb = batch(name, planes, 176 if name != "yuyv" else 0)                # 4-aligned rows and chroma rows
    assert np.array_equal(vr.desc_to_rgb(buf, d, H, W, tup(fmt), 2), rgb)          # the helper's gather sees the planes that went in
    x = dev(buf)
    assert np.array_equal(det.video_to_rgb(x, 2, H, W, d, fmt).cpu().numpy(), rgb)
    det.set_option("profile", 1)
    try:
        names = names_of(det, lambda: det.run_video(x, 2, d, fmt))
    finally:
        det.set_option("profile", 0)
    same(snapshot(det, 2), want, (name, tup(fmt)))
    expect = {"nv12": "k_ingest_yuv420", "i420": "k_ingest_yuv_planar", "yuyv": "k_ingest_yuv_packed422", "i444": "k_ingest_yuv_planar"}[name]
    assert expect in names and not any(n.startswith("k_ingest") and n != expect for n in names), names


FACE64_32 = dict(name="FACE64", nTrees=128, cascThr=-4.0, minDs_h=32, minDs_w=32)
TINY_96 = dict(name="TINY", nTrees=96, cascThr=-3.0)
# orientation code, scale, model (none: INRIA): rgb2luv_sse, then rgb2gray and the planes as they are behind the turned, the reduced and the
# turned and reduced (staged: code 3; generic: code 6) entries
COMPOSED = [(1, None), (6, None), (0, 0.6), (0, 1.5), (3, 0.6),
            (1, None, FACE64_32), (6, None, TINY_96), (0, 0.6, FACE64_32), (0, 0.6, TINY_96), (3, 0.6, FACE64_32), (6, 0.6, TINY_96)]


@pytest.mark.parametrize("case", COMPOSED, ids=["orient1", "orient6", "scale06", "scale15", "orient3_scale06", "orient1_gray", "orient6_isluv", "scale06_gray",
                                                "scale06_isluv", "orient3_scale06_gray", "orient6_scale06_isluv"])
def test_bt709_turned_and_reduced_matches_its_composed_definition(case):
    """numpy's R, G, B of the stored frame, turned upright by numpy, then run_u8(PIX_RGB) — through the image entry's resize (the
    apps' Resizer on tight upright bytes) where the call reduces."""
    from acf_amd.detector import HipDetector
    orient, scale = case[:2]
    model = case[2] if len(case) > 2 else INRIA
    fmt = F(8, 0, capi.YUV_MATRIX_BT709, 0)
    sr, sc = (H, W) if not scale else ((216, 290) if scale < 1 else (88, 116))
    if orient & 1:
        sr, sc = sc, sr
    ph, pw = HipDetector.oriented_resized_dims(sr, sc, orient, scale) if scale else HipDetector.oriented_dims(sr, sc, orient)
    det = HipDetector(synth.make_model(seed=3, **model), ph, pw, 3, max_batch=2, max_hits=1 << 16)
    planes = [video_planes(320 + f, sr, sc, 1, 1) for f in range(2)]
    buf, d, fb = batch("nv12" if orient != 6 else "i420", planes)
    rgb = vr.desc_to_rgb(buf, d, sr, sc, tup(fmt), 2)
    up = np.ascontiguousarray(orf.orient(rgb, orient, axes=(1, 2)))
    if scale:
        xu = dev(up)
        det.run_tensor_resized(xu, scale, layout="nhwc")
        want = nonvacuous(snapshot(det, 2), case)
    else:
        want = nonvacuous(rgb_expect(det, up), case)
    x = dev(buf)
    det.run_video(x, 2, d, fmt, sr, sc, orient, scale)
    same(snapshot(det, 2), want, case)
    det.pyramid_video(x, 2, d, fmt, sr, sc, orient, scale)
    det.detect()
    same(snapshot(det, 2), want, (case, "pyramid + detect"))
    det.close()


# ---------------------------------------------------------------- 5. 16-bit words

WIDE = [  # id, layout, format, row stride in bytes
    ("p010_bt2020", "nv12", F(10, 6, 2, 0), 352),
    ("p016_bt709_full", "nv12", F(16, 0, 1, 1), 0),
    ("yuv420p10le", "i420", F(10, 0, 1, 0), 0),
    ("i210", "i422", F(10, 0, 1, 0), 352),
    ("i410", "i444", F(10, 0, 2, 1), 0),
    ("y210", "yuyv", F(10, 6, 1, 0), 0),
    ("bits12_shift4", "i420", F(12, 4, 0, 1), 0),
]


@pytest.mark.parametrize("case", WIDE, ids=[c[0] for c in WIDE])
def test_wide_formats_equal_run_image_on_the_float_image(det130, case):
    det = det130
    tag, name, fmt, stride = case
    sx, sy = ydr.SUB[name]
    planes = [vr.random_planes16(500 + 10 * f + fmt.bits, name, H, W, fmt.bits) for f in range(2)]
    buf, d, fb = batch16(name, planes, fmt, stride, junk_seed=77)
    rgb = vr.desc_to_rgb(buf, d, H, W, tup(fmt), 2)
    clean = np.stack([vr.to_rgb(Y, ydr.upsample(U, H, W, sx, sy), ydr.upsample(V, H, W, sx, sy), fmt.bits, fmt.matrix, fmt.full_range) for Y, U, V in planes])
    assert np.array_equal(rgb, clean)                                     # the gather masks the junk and sees the planes that went in
    want = nonvacuous(f32_expect(det, rgb, fmt), tag)
    x = dev(buf)
    assert np.array_equal(det.video_to_rgb(x, 2, H, W, d, fmt).cpu().numpy().view(np.uint16), rgb)
    det.run_video(x, 2, d, fmt)
    same(snapshot(det, 2), want, tag)
    det.pyramid_video(x, 2, d, fmt)
    det.detect()
    same(snapshot(det, 2), want, (tag, "pyramid + detect"))


def _planar16(planes, ystride, cstride, lead, shift):
    """Hand-packed planar frames of words with any even byte strides, `lead` bytes in front -> (buffer, descriptor from buf[lead])."""
    h, w = planes[0][0].shape
    ch, cw = planes[0][1].shape
    fb = ystride * h + 2 * cstride * ch
    buf = np.full(lead + fb * len(planes), 0x5A, np.uint8)
    for f, (Y, U, V) in enumerate(planes):
        fr = buf[lead + f * fb:lead + (f + 1) * fb]
        for at, P, st in ((0, Y, ystride), (ystride * h, U, cstride), (ystride * h + cstride * ch, V, cstride)):
            rows, cols = P.shape
            fr[at:at + st * rows].reshape(rows, st)[:, :2 * cols] = (P.astype(np.uint16) << shift).view(np.uint8).reshape(rows, 2 * cols)
    sub = (1 if cw < w else 0, 1 if ch < h else 0)
    d = capi.YuvDesc(capi.YuvPlane(0, fb, ystride, 2), capi.YuvPlane(ystride * h, fb, cstride, 2), capi.YuvPlane(ystride * h + cstride * ch, fb, cstride, 2), *sub)
    return buf, d


def test_the_three_load_forms_give_identical_pyramids_and_report_their_names(det130):
    det = det130
    fmt = F(10, 6, capi.YUV_MATRIX_BT2020, 0)
    planes = [vr.random_planes16(610 + f, "i420", H, W, 10) for f in range(2)]
    clean = np.stack([vr.to_rgb(Y, ydr.upsample(U, H, W, 1, 1), ydr.upsample(V, H, W, 1, 1), 10, 2, 0) for Y, U, V in planes]).astype(np.uint16)
    want = nonvacuous(f32_expect(det, clean, fmt), "forms")
    det.set_option("profile", 1)
    try:
        def run(x, off, d):
            names = names_of(det, lambda: det.run_video(x.data_ptr() + off, 2, d, fmt))
            return snapshot(det, 2), names
        buf, d = _planar16(planes, 352, 176, 0, 6)                        # every plane, row and frame 4-aligned
        a, names = run(dev(buf), 0, d)
        assert "k_ingest_yuv16_planar" in names and not (names & {"k_ingest_yuv16_generic", "k_ingest_yuv16_pairs"}), names
        buf, d = _planar16(planes, 350, 178, 2, 6)                        # the same pictures from a base 2 bytes further, rows 2 (mod 4)
        b, names = run(dev(buf), 2, d)
        assert "k_ingest_yuv16_generic" in names and not (names & {"k_ingest_yuv16_planar", "k_ingest_yuv16_pairs"}), names
        buf, d, fb = batch16("nv12", planes, fmt)                         # P010
        c, names = run(dev(buf), 0, d)
        assert "k_ingest_yuv16_pairs" in names and not (names & {"k_ingest_yuv16_planar", "k_ingest_yuv16_generic"}), names
        buf, d, fb = batch16("nv21", planes, fmt)                         # (V, U) pairs
        e, names = run(dev(buf), 0, d)
        assert "k_ingest_yuv16_pairs" in names, names
    finally:
        det.set_option("profile", 0)
    same(a, want, "planar form")
    same(b, a, "generic against planar")
    same(c, a, "pairs against planar")
    same(e, a, "pairs, V first, against planar")


def _pairs16(planes, stride, shift):
    """Hand-packed P010-like frames of any size: Y words, then rows of (U, V) word pairs, `stride` bytes a row -> (buffer, descriptor)."""
    h, w = planes[0][0].shape
    ch, cw = planes[0][1].shape
    assert stride % 4 == 0 and stride >= 2 * w and stride >= 4 * cw
    fb = stride * (h + ch)
    buf = np.full(fb * len(planes), 0x5A, np.uint8)
    for f, (Y, U, V) in enumerate(planes):
        fr = buf[f * fb:(f + 1) * fb]
        fr[:stride * h].reshape(h, stride)[:, :2 * w] = (Y.astype(np.uint16) << shift).view(np.uint8).reshape(h, 2 * w)
        uv = (np.stack([U, V], axis=-1).astype(np.uint16) << shift).reshape(ch, 2 * cw)
        fr[stride * h:].reshape(ch, stride)[:, :4 * cw] = uv.view(np.uint8).reshape(ch, 4 * cw)
    d = capi.YuvDesc(capi.YuvPlane(0, fb, stride, 2), capi.YuvPlane(stride * h, fb, stride, 4), capi.YuvPlane(stride * h + 2, fb, stride, 4), 1, 1)
    return buf, d


ODD_FORMS = [
    # id, builder(planes) -> (buffer, descriptor), format, the kernel it must reach
    ("odd_word_stride_generic", lambda p: _planar16(p, 2 * 175, 2 * 89, 0, 0), F(10, 0, capi.YUV_MATRIX_BT709, 0), "k_ingest_yuv16_generic"),
    ("dword_loads_with_tails", lambda p: _planar16(p, 352, 176, 0, 0), F(10, 0, capi.YUV_MATRIX_BT709, 0), "k_ingest_yuv16_planar"),
    ("p010_pairs", lambda p: _pairs16(p, 352, 6), F(10, 6, capi.YUV_MATRIX_BT2020, 0), "k_ingest_yuv16_pairs"),
    # 8 bits, not the default format: the scalar rgb2luv behind the kernels that take the constants as an argument
    ("bt709_planar_8", lambda p: oc.planar_buffer(p, 176, 88, (1, 1))[:2], F(8, 0, capi.YUV_MATRIX_BT709, 0), "k_ingest_yuv_planar"),
    ("bt709_bytes_8", lambda p: oc.planar_buffer(p, 175, 89, (1, 1))[:2], F(8, 0, capi.YUV_MATRIX_BT709, 0), "k_ingest_yuv_generic"),
    ("bt2020_full_yuyv_8", lambda p: oc.yuyv_buffer(p, 352)[:2], F(8, 0, capi.YUV_MATRIX_BT2020, 1), "k_ingest_yuv_packed422"),
]


@pytest.mark.parametrize("case", ODD_FORMS, ids=[c[0] for c in ODD_FORMS])
def test_odd_sizes_reach_the_scalar_luv_body(case):
    """131 x 175 (h * w % 4 == 1: IG_LUV) as hand-built frames with ceil-sized chroma planes (66 x 88; packed 4:2:2: 131 x 88)."""
    from acf_amd.detector import HipDetector
    tag, build, fmt, kernel = case
    h, w, nF = 131, 175, 2
    ch = h if "yuyv" in tag else 66
    top = 1 << fmt.bits
    det = HipDetector(synth.make_model(seed=3, name="INRIA", nTrees=64, cascThr=-2.5, nOctUp=0), h, w, 3, max_batch=nF, max_hits=1 << 16)
    rng = np.random.RandomState(19)
    planes = [(rng.randint(0, top, (h, w)), rng.randint(0, top, (ch, 88)), rng.randint(0, top, (ch, 88))) for _ in range(nF)]
    buf, d = build(planes)
    assert (d.sub_x, d.sub_y) == (1, 1 if ch == 66 else 0)
    rgb = vr.desc_to_rgb(buf, d, h, w, tup(fmt), nF)
    assert np.array_equal(rgb, np.stack([vr.to_rgb(Y, ydr.upsample(U, h, w, 1, d.sub_y), ydr.upsample(V, h, w, 1, d.sub_y), fmt.bits, fmt.matrix, fmt.full_range)
                                         for Y, U, V in planes]))
    want = nonvacuous(f32_expect(det, rgb, fmt) if fmt.bits > 8 else rgb_expect(det, rgb.astype(np.uint8)), tag)
    x = dev(buf)
    got = det.video_to_rgb(x, nF, h, w, d, fmt).cpu().numpy()
    assert np.array_equal(got.view(np.uint16) if fmt.bits > 8 else got, rgb)
    det.set_option("profile", 1)
    names = names_of(det, lambda: det.run_video(x, nF, d, fmt))
    assert kernel in names, names
    same(snapshot(det, nF), want, tag)
    det.close()


def test_three_separate_allocations_one_below_the_base(det130):
    import torch
    det = det130
    fmt = F(10, 0, capi.YUV_MATRIX_BT709, 1)
    planes = [vr.random_planes16(640 + f, "i420", H, W, 10) for f in range(2)]
    Y, U, V = (np.stack([p[i] for p in planes]).astype(np.int16) for i in range(3))
    rgb = np.stack([vr.to_rgb(y, ydr.upsample(u, H, W, 1, 1), ydr.upsample(v, H, W, 1, 1), 10, 1, 1) for y, u, v in planes]).astype(np.uint16)
    want = nonvacuous(f32_expect(det, rgb, fmt), "separate")
    arena = torch.empty(V.size + Y.size + U.size + 32, dtype=torch.int16, device="cuda")       # V, Y, U: V lies below the base
    v = arena[:V.size].view(V.shape)
    y = arena[V.size:V.size + Y.size].view(Y.shape)
    u = arena[V.size + Y.size:V.size + Y.size + U.size].view(U.shape)
    v.copy_(dev(V)), y.copy_(dev(Y)), u.copy_(dev(U))
    torch.cuda.synchronize()
    base, n, d = det.video_planes_desc(y, u, v, 1, 1)
    assert n == 2 and d.v.offset < 0 < d.u.offset and d.y.stride_px == 2
    lo, hi = det.video_extent(d, fmt, H, W, 2)
    assert lo == [0, d.u.offset, d.v.offset] and hi[0] == 2 * Y.size - 1 and hi[2] == d.v.offset + 2 * V.size - 1
    det.run_video_planes(y, u, v, 1, 1, fmt)
    same(snapshot(det, 2), want, "separate allocations")


def test_stride_n_zero_repeats_one_frame(det130):
    det = det130
    fmt = F(10, 6, capi.YUV_MATRIX_BT2020, 0)
    planes = [vr.random_planes16(660, "i420", H, W, 10)]
    buf, d, fb = batch16("nv12", planes, fmt)
    rgb = vr.desc_to_rgb(buf, d, H, W, tup(fmt), 1)
    want = nonvacuous(f32_expect(det, np.concatenate([rgb, rgb]), fmt), "repeat")
    for p in (d.y, d.u, d.v):
        p.stride_n = 0
    x = dev(buf)
    det.run_video(x, 2, d, fmt)
    same(snapshot(det, 2), want, "stride_n = 0")


MODE_CASES = [
    ("face64_gray", 120, 160, dict(name="FACE64", nTrees=128, cascThr=-4.0, minDs_h=32, minDs_w=32)),   # IG_GRAY
    ("tiny_isluv", 96, 128, dict(name="TINY", nTrees=96, cascThr=-3.0)),                                # planes taken as they are
    # the same two on 3 x 3 ragged tiles (a ragged width of 6: not a multiple of 16); tight rows of 134 samples put the first layout on the
    # element-wise load form.  H % 4 == 2: scalar stores, a last quad of two rows; H % 4 == 0: float4 stores
    ("face64_gray_ragged", 130, 134, dict(name="FACE64", nTrees=128, cascThr=-4.0, minDs_h=32, minDs_w=32)),
    ("face64_gray_ragged_vec", 132, 134, dict(name="FACE64", nTrees=128, cascThr=-4.0, minDs_h=32, minDs_w=32)),
    ("tiny_isluv_ragged", 130, 134, dict(name="TINY", nTrees=96, cascThr=-3.0)),
    ("tiny_isluv_ragged_vec", 132, 134, dict(name="TINY", nTrees=96, cascThr=-3.0)),
]


@pytest.mark.parametrize("case", MODE_CASES, ids=[c[0] for c in MODE_CASES])
def test_grey_and_pass_through_models(case):
    from acf_amd.detector import HipDetector
    tag, h, w, kw = case
    det = HipDetector(synth.make_model(seed=3, **kw), h, w, 3, max_batch=2, max_hits=1 << 16)
    total = 0
    # (tight rows of w samples: the wide forms need every plane's rows four-aligned)
    layouts = (("nv12", F(10, 6, 2, 0), "k_ingest_yuv16_pairs"), ("i422", F(12, 0, 1, 1), "k_ingest_yuv16_planar" if w % 4 == 0 else "k_ingest_yuv16_generic"),
               # 8 bits, not the default format: the instantiations that take the constants as an argument
               ("nv12", F(8, 0, 1, 0), "k_ingest_yuv420"), ("i420", F(8, 0, 1, 0), "k_ingest_yuv_planar" if w % 8 == 0 else "k_ingest_yuv_generic"),
               ("yuyv", F(8, 0, 2, 1), "k_ingest_yuv_packed422"))
    for name, fmt, kernel in layouts:
        sx, sy = ydr.SUB[name]
        planes = [video_planes(40 + f, h, w, sx, sy, fmt.bits) for f in range(2)]
        buf, d, fb = batch16(name, planes, fmt) if fmt.bits > 8 else batch(name, planes)
        rgb = vr.desc_to_rgb(buf, d, h, w, tup(fmt), 2)
        want = f32_expect(det, rgb, fmt) if fmt.bits > 8 else rgb_expect(det, rgb.astype(np.uint8))
        x = dev(buf)
        det.set_option("profile", 1)
        try:
            names = names_of(det, lambda: det.run_video(x, 2, d, fmt))
        finally:
            det.set_option("profile", 0)
        assert kernel in names and not any(n.startswith("k_ingest") and n != kernel for n in names), (tag, name, names)
        same(snapshot(det, 2), want, (tag, name, tup(fmt)))
        total += sum(len(s[1]) for s in want)
    assert total > 0, "no detections: the cascade comparison would be vacuous"
    det.close()


def test_reference_arithmetic_tier(oracle):
    """Option "arith" = 1 with the committed x86 tables: P010 against run_image, BT.709 NV12 against run_u8, under the same option."""
    from acf_amd.detector import HipDetector
    det = HipDetector(synth.make_model(seed=3, **INRIA), H, W, 3, max_batch=2, max_hits=1 << 16)
    f10, f8 = F(10, 6, 2, 0), F(8, 0, 1, 0)
    p10 = [vr.random_planes16(700 + f, "i420", H, W, 10) for f in range(2)]
    buf10, d10, _ = batch16("nv12", p10, f10)
    rgb10 = vr.desc_to_rgb(buf10, d10, H, W, tup(f10), 2)
    p8 = [ydr.random_planes(710 + f, "nv12", H, W) for f in range(2)]
    buf8, d8, _ = batch("nv12", p8)
    rgb8 = vr.desc_to_rgb(buf8, d8, H, W, tup(f8), 2)
    exact = f32_expect(det, rgb10, f10)
    det.set_x86_tables(*oracle.x86_fixture())
    det.set_option("arith", 1)
    want10 = nonvacuous(f32_expect(det, rgb10, f10), "arith 10")
    assert any(not np.array_equal(a, b) for a, b in zip(want10[0][0], exact[0][0]))             # (the tier is not a no-op)
    x = dev(buf10)
    det.run_video(x, 2, d10, f10)
    same(snapshot(det, 2), want10, "P010 arith")
    want8 = nonvacuous(rgb_expect(det, rgb8), "arith 8")
    x = dev(buf8)
    det.run_video(x, 2, d8, f8)
    same(snapshot(det, 2), want8, "BT.709 NV12 arith")
    det.close()


# ---------------------------------------------------------------- 6. the stream

@pytest.mark.parametrize("kind", ["p010", "i420_bt709"])
def test_stream_matches_blocking_calls(kind):
    """Four batches (one short) from pinned memory, two in flight, give the records of run_video + export of each batch."""
    import torch
    from acf_amd.detector import HipDetector, PinnedBuffer
    h, w, cap, nB, depth = 120, 160, 512, 3, 2
    det = HipDetector(synth.make_model(seed=3, **INRIA), h, w, 3, max_batch=nB, max_hits=4096)
    fmt, name = (F(10, 6, 2, 0), "nv12") if kind == "p010" else (F(8, 0, 1, 0), "i420")
    d, fb = HipDetector.video_desc(name, h, w, fmt)
    batches = []
    for b in range(4):
        n = nB if b != 2 else 1
        planes = [video_planes(100 + 10 * b + i, h, w, 1, 1, fmt.bits) for i in range(n)]
        buf = batch16(name, planes, fmt)[0] if fmt.bits > 8 else batch(name, planes)[0]
        batches.append(buf.reshape(n, fb))
    want = []
    for x in batches:
        xd = dev(x)                                                       # (alive until the synchronise: the call is asynchronous)
        det.run_video(xd, x.shape[0], d, fmt)
        dst = torch.zeros((x.shape[0], 1 + 6 * cap), dtype=torch.int32, device="cuda")
        torch.cuda.synchronize()                                          # (torch fills dst on its own stream: before the export writes it)
        det.export_detections(dst, cap)
        det.synchronize()
        want.append(dst.cpu().numpy())
    assert sum(int(x[:, 0].sum()) for x in want) > 0
    pins = [PinnedBuffer(nB * fb) for _ in range(depth)]
    det.stream_open_video(d, fmt, fb, cap, depth)
    got, inflight = [], []
    for b, x in enumerate(batches):
        if len(inflight) == depth:
            got.append(det.stream_collect(inflight.pop(0)))
        pin = pins[b % depth]
        pin.array[:x.size] = x.ravel()
        inflight.append(det.stream_submit(pin.ptr.value, x.shape[0]))
    while inflight:
        got.append(det.stream_collect(inflight.pop(0)))
    for b in range(4):
        assert got[b].shape == want[b].shape, b
        for f in range(want[b].shape[0]):
            n = want[b][f, 0]
            assert got[b][f, 0] == n
            assert np.array_equal(got[b][f, :1 + 6 * n], want[b][f, :1 + 6 * n]), (b, f)
    det.stream_close()
    det.close()
    for p in pins:
        p.close()


# ---------------------------------------------------------------- 7. what is refused

def test_video_entry_argument_checks():
    import torch
    from acf_amd.detector import HipDetector, HipError
    model = synth.make_model(seed=3, name="TINY", nTrees=16)
    h, w = 96, 128
    x = torch.zeros(8 * h * w * 3, dtype=torch.uint8).cuda()             # room for every call below, were it not refused
    f8, f10 = F(8, 0, 1, 0), F(10, 6, 2, 0)
    good8, fb8 = HipDetector.video_desc("i420", h, w, f8)
    good10, fb10 = HipDetector.video_desc("nv12", h, w, f10)
    det = HipDetector(model, h, w, 3, max_batch=2)

    def refused(fn, code=capi.E_INVALID):
        with pytest.raises(HipError) as e:
            fn()
        assert e.value.code == code, e.value
        det.run_video(x, 2, good10, f10)                                 # the context still works
        det.run_video(x, 2, good8, f8)
        det.synchronize()

    def variant(good, **kw):
        d = capi.YuvDesc.from_buffer_copy(good)
        for k, v in kw.items():
            plane, _, field = k.partition("_")
            setattr(getattr(d, plane), field, v) if plane in ("y", "u", "v") else setattr(d, k, v)
        return d
    lib = det.lib
    ptr = C.c_void_p(x.data_ptr())
    # what the family's existing entry refuses
    assert lib.acf_hip_run_video(det.ctx, None, 1, C.byref(good10), C.byref(f10), 0, 0, 0, 0.0) == capi.E_INVALID
    assert lib.acf_hip_run_video(det.ctx, ptr, 1, None, C.byref(f10), 0, 0, 0, 0.0) == capi.E_INVALID
    assert lib.acf_hip_pyramid_video(None, ptr, 1, C.byref(good10), C.byref(f10), 0, 0, 0, 0.0) == capi.E_INVALID
    for good, fmt in ((good8, f8), (good10, f10)):
        refused(lambda: det.run_video(x, 0, good, fmt))
        refused(lambda: det.run_video(x, 3, good, fmt))                   # max_batch is 2
        for bad in (variant(good, sub_x=2), variant(good, y_stride_px=0), variant(good, u_stride_row=0), variant(good, v_stride_n=-4)):
            refused(lambda: det.run_video(x, 1, bad, fmt))
            refused(lambda: det.pyramid_video(x, 1, bad, fmt))
            refused(lambda: det.video_to_rgb(x, 1, h, w, bad, fmt))
            refused(lambda: det.stream_open_video(bad, fmt, fb10, 64, 2))
    refused(lambda: det.run_video(x, 1, good8, f8, h, w, 8))              # orient outside 0 .. 7
    refused(lambda: det.run_video(x, 1, good8, f8, h + 2, w, 0))          # not the plan's size
    refused(lambda: det.run_video(x, 1, good8, f8, h, w, 0, -0.5))
    refused(lambda: det.run_video(x, 1, good8, f8, h, w, 0, float("nan")))
    refused(lambda: det.run_video(x, 1, good8, f8, h, w, 0, 0.5))         # the plan is not for the reduced size
    # the format
    for bad in (F(7), F(17), F(8, 1), F(10, 7), F(16, 1), F(8, 0, 3), F(8, 0, 0, 2)):
        refused(lambda: det.run_video(x, 1, good8, bad))
        refused(lambda: det.pyramid_video(x, 1, good8, bad))
        refused(lambda: det.video_to_rgb(x, 1, h, w, good8, bad))
        refused(lambda: det.stream_open_video(good8, bad, fb8, 64, 2))
    # 16-bit words: an odd base, offset or stride
    refused(lambda: det.run_video(x.data_ptr() + 1, 1, good10, f10))
    refused(lambda: det.video_to_rgb(x.data_ptr() + 1, 1, h, w, good10, f10))
    for bad in (variant(good10, y_offset=1), variant(good10, u_stride_row=2 * w + 1), variant(good10, v_stride_n=fb10 + 1), variant(good10, u_stride_px=3)):
        refused(lambda: det.run_video(x, 1, bad, f10))
        refused(lambda: det.video_to_rgb(x, 1, h, w, bad, f10))
        refused(lambda: det.stream_open_video(bad, f10, fb10, 64, 2))
    # more than 8 bits, turned or reduced
    refused(lambda: det.run_video(x, 1, good10, f10, w, h, 1), capi.E_UNSUPPORTED)
    refused(lambda: det.pyramid_video(x, 1, good10, f10, h, w, 2), capi.E_UNSUPPORTED)
    refused(lambda: det.run_video(x, 1, good10, f10, 2 * h, 2 * w, 0, 0.5), capi.E_UNSUPPORTED)
    refused(lambda: det.stream_open_video(good10, f10, fb10, 64, 2, h, w, 2), capi.E_UNSUPPORTED)
    refused(lambda: det.stream_open_video(good10, f10, fb10, 64, 2, 2 * h, 2 * w, 0, 0.5), capi.E_UNSUPPORTED)
    # the conversion alone: null destination, empty sizes
    assert lib.acf_hip_video_to_rgb(det.ctx, ptr, 1, h, w, C.byref(good10), C.byref(f10), None) == capi.E_INVALID
    refused(lambda: det.video_to_rgb(x, 1, 0, w, good10, f10))
    refused(lambda: det.video_to_rgb(x, 0, h, w, good8, f8))
    # the stream: the last word's high byte outside frame_bytes, stride_n other than frame_bytes, depth, cap
    refused(lambda: det.stream_open_video(good10, f10, fb10 - 1, 64, 2))
    refused(lambda: det.stream_open_video(variant(good10, y_stride_n=fb10 + 4), f10, fb10, 64, 2))
    refused(lambda: det.stream_open_video(good10, f10, fb10, 64, 1))
    refused(lambda: det.stream_open_video(good8, f8, fb8, 0, 2))
    # plans of one and of five input planes; no plan; sub-batch contexts
    g = HipDetector(synth.make_model(seed=3, name="FACE64", nTrees=16), h, w, 1, max_batch=1)
    refused(lambda: g.run_video(x, 1, good10, f10))
    refused(lambda: g.run_video(x, 1, good8, f8))
    g.close()
    five = HipDetector(model, h, w, 5, max_batch=1)
    refused(lambda: five.run_video(x, 1, good10, f10))
    five.close()
    none = HipDetector(model)
    refused(lambda: none.run_video(x, 1, good10, f10), capi.E_NOPLAN)
    refused(lambda: none.stream_open_video(good10, f10, fb10, 64, 2), capi.E_NOPLAN)
    none.close()
    multi = HipDetector(model, h, w, 3, max_batch=4, streams=2)
    refused(lambda: multi.run_video(x, 2, good10, f10), capi.E_UNSUPPORTED)
    refused(lambda: multi.run_video(x, 2, good8, f8), capi.E_UNSUPPORTED)
    refused(lambda: multi.stream_open_video(good10, f10, fb10, 64, 2), capi.E_UNSUPPORTED)
    multi.close()
    small = HipDetector(model, *HipDetector.resize_dims(192, 256, 0.5), 3, max_batch=1)
    small.set_input_resize(192, 256, 0.5)
    refused(lambda: small.run_video(x, 1, good10, f10))
    small.close()
    det.close()


# ---------------------------------------------------------------- 8. the C++ host

CLI = [("p010_bt2020", "nv12", F(10, 6, 2, 0), ["--bits", "10", "--shift", "6", "--matrix", "bt2020"], []),
       ("i420_bt709_full_stream", "i420", F(8, 0, 1, 1), ["--matrix", "bt709", "--range", "full"], ["--stream", "2"])]


@pytest.mark.parametrize("case", CLI, ids=[c[0] for c in CLI])
def test_cli_video_format_matches_the_python_path(tmp_path, case):
    """acf::HipDetector::setVideoFormat with detectYuv and streamOpenYuv / streamSubmit through the CLI print what run_video returns."""
    import subprocess
    from acf_amd.detector import HipDetector
    from acf_amd.modelio import write_model
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    from test_host_cpp import parse, run
    tag, name, fmt, flags, mode = case
    host = os.path.join(ROOT, "acf_amd", "host")
    subprocess.check_call(["make", "-s", "-C", host])
    h, w, cnt = 120, 160, 5
    model = synth.make_model(seed=3, **INRIA)
    write_model(str(tmp_path / "m.acfm"), model)
    planes = [video_planes(60 + i, h, w, 1, 1, fmt.bits) for i in range(cnt)]
    buf, d, fb = batch16(name, planes, fmt) if fmt.bits > 8 else batch(name, planes)
    (tmp_path / "f.yuv").write_bytes(buf.tobytes())
    p = run(os.path.join(host, "acf_hip_detect"), ["--model", str(tmp_path / "m.acfm"), "--frames", str(tmp_path / "f.yuv"), "--yuv", name,
                                                   "--rows", str(h), "--cols", str(w), "--count", str(cnt)] + flags + mode)
    got = parse(p.stdout)
    det = HipDetector(model, h, w, 3, max_batch=cnt, max_hits=1 << 16)
    x = dev(buf)
    det.run_video(x, cnt, d, fmt)
    total = 0
    for f in range(cnt):
        dd, _ = det.detections(f)
        py = [(int(r["x"]), int(r["y"]), int(r["w"]), int(r["h"]), int(np.float32(r["score"]).view(np.uint32))) for r in dd]
        assert got[f] == py, f
        total += len(py)
    assert total > 0
    det.close()
