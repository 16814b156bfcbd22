"""YUV 4:2:0 (NV12 / NV21) input, the part that needs no GPU: the numpy restatement of the conversion (tests/yuv420_ref.py) against
hand-computed vectors and against the real-valued BT.601 matrix on every (Y, U, V); the frozen fixture; and the library's host
arithmetic for frame sizes (acf_hip_u8_frame_bytes).

The conversion is cvtColor(COLOR_YUV2RGB_NV12 / _NV21) restated from OpenCV's published source; OpenCV itself is compared where
`cv2` is importable and skipped otherwise — what this file pins without it is that no constant is mistyped, not OpenCV's bits.
"""
import ctypes as C
import os

import numpy as np
import pytest

import yuv420_ref as yr
from acf_amd import capi

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "yuv420_rgb.npz")


def one(Y, U, V):
    return tuple(int(x) for x in yr.yuv_to_rgb(Y, U, V))


def test_hand_computed_vectors():
    assert one(16, 128, 128) == (0, 0, 0)            # black: y = 0, (1 << 19) >> 20 = 0
    assert one(235, 128, 128) == (255, 255, 255)     # white: (219 * 1220542 + 524288) >> 20 = 267823986 >> 20 = 255
    assert one(0, 128, 128) == one(16, 128, 128)     # Y < 16 is black: max(0, Y - 16)
    assert one(7, 128, 128) == (0, 0, 0)
    assert one(255, 128, 128) == (255, 255, 255)     # (239 * 1220542 + 524288) >> 20 = 278 -> clamped
    assert one(126, 128, 128) == (128, 128, 128)     # (110 * 1220542 + 524288) >> 20 = 134783908 >> 20 = 128
    # saturation at both ends of every component
    # y = 219 * 1220542 = 267298698; R: (y + 524288 + 1673527 * 127) >> 20 = 458 -> 255; G: (y + 524288 - 852492 * 127) >> 20 =
    # 159556502 >> 20 = 152; B: 267822986 >> 20 = 255
    assert one(235, 128, 255) == (255, 152, 255)
    # y = 0; R: (524288 - 1673527 * 128) >> 20 = -213687168 >> 20 = -204 -> 0; G: (524288 + 852492 * 128 + 409993 * 128) >> 20 =
    # 162122368 >> 20 = 154; B: -270327040 >> 20 = -258 -> 0
    assert one(16, 0, 0) == (0, 154, 0)
    assert one(16, 255, 255) == (203, 0, 255)        # 213062217 >> 20 = 203; -159811307 >> 20 = -153 -> 0; 269259590 >> 20 = 256 -> 255
    assert one(255, 255, 0) == (74, 255, 255)        # y = 239 * 1220542 = 291709538; 78022370 >> 20 = 74; 333 and 534 -> 255
    # a negative sum just below zero floors to -1 (arithmetic shift), not to 0 — and the standard's primaries come out as primaries:
    assert one(81, 90, 240) == (254, 0, 0)           # red:   267294542 >> 20 = 254; -39852 >> 20 = -1 -> 0; -549470 >> 20 = -1 -> 0
    assert one(145, 54, 34) == (0, 255, 1)           # green: 662668 >> 20 = 0; 268447936 >> 20 = 256 -> 255; 1388282 >> 20 = 1
    assert one(41, 240, 110) == (0, 0, 255)          # blue


def _scalar(Y, U, V):
    """The definition with Python integers (no numpy, no fixed width): include/acf_hip.h, line for line."""
    y = max(0, Y - 16) * 1220542
    ruv = (1 << 19) + 1673527 * (V - 128)
    guv = (1 << 19) - 852492 * (V - 128) - 409993 * (U - 128)
    buv = (1 << 19) + 2116026 * (U - 128)
    cl = lambda x: min(max(x, 0), 255)
    return cl((y + ruv) >> 20), cl((y + guv) >> 20), cl((y + buv) >> 20)


def test_numpy_restatement_equals_python_integers():
    """int32 is wide enough (largest magnitude: 239 * CY + 2^19 + 127 * CUB < 2^30) and >> floors negatives in both."""
    rng = np.random.RandomState(5)
    trip = np.concatenate([rng.randint(0, 256, (4000, 3)), [[0, 0, 0], [255, 255, 255], [255, 0, 255], [255, 255, 0], [0, 255, 0], [16, 0, 255]]])
    got = yr.yuv_to_rgb(trip[:, 0], trip[:, 1], trip[:, 2])
    for t, g in zip(trip, got):
        assert tuple(int(x) for x in g) == _scalar(*[int(x) for x in t]), t


def test_nv21_is_nv12_with_the_chroma_bytes_swapped():
    rows, cols = 6, 8
    a = yr.random_frame(3, rows, cols, nv21=False)
    b = a.copy()
    c = b[rows * cols:].reshape(-1, 2)
    c[:] = c[:, ::-1]
    assert np.array_equal(yr.nv_to_rgb(a, rows, cols, nv21=False), yr.nv_to_rgb(b, rows, cols, nv21=True))
    assert not np.array_equal(yr.nv_to_rgb(a, rows, cols, nv21=False), yr.nv_to_rgb(a, rows, cols, nv21=True))


def test_which_chroma_pair_each_pixel_takes():
    """4 x 6 frame, row stride 9, chroma at byte 40 (the luma plane ends at 36): pixel (r, c) takes the pair of block (r // 2, c // 2),
    and padding bytes are never read."""
    rows, cols, stride, off = 4, 6, 9, 40
    Y = np.full((rows, cols), 126, np.uint8)
    U = np.array([[128, 0, 255], [90, 128, 200]], np.uint8)
    V = np.array([[128, 255, 0], [200, 30, 128]], np.uint8)
    buf = yr.pack(Y, U, V, stride=stride, chroma_offset=off, fill=0x33)
    assert buf.size == off + stride * 2 and buf[cols] == 0x33 and buf[36] == 0x33
    assert list(buf[off:off + cols]) == [128, 128, 0, 255, 255, 0]  # U, V interleaved
    rgb = yr.nv_to_rgb(buf, rows, cols, stride=stride, chroma_offset=off)
    for r in range(rows):
        for c in range(cols):
            assert tuple(int(x) for x in rgb[r, c]) == _scalar(126, int(U[r // 2, c // 2]), int(V[r // 2, c // 2])), (r, c)
    other = yr.nv_to_rgb(yr.pack(Y, U, V, stride=stride, chroma_offset=off, fill=0xCC), rows, cols, stride=stride, chroma_offset=off)
    assert np.array_equal(rgb, other)


def test_within_one_code_value_of_the_real_matrix_on_every_triple():
    """All 2^24 (Y, U, V): |restated - round(real BT.601 limited range)| <= 1 per component after clamping to 0..255.  The real
    matrix is the standard's: 255/219 on max(Y - 16, 0); 1.596027, -0.812968, -0.391762, 2.017232 on the chroma differences.  One
    code value is what a truncating shift against rounding allows; the maximum is exactly 1 on each component."""
    U, V = np.meshgrid(np.arange(256), np.arange(256), indexing="ij")
    u, v = (U - 128).astype(np.float64), (V - 128).astype(np.float64)
    worst = np.zeros(3, np.int64)
    for Y in range(256):
        y = max(Y - 16, 0) * (255.0 / 219.0)
        real = np.stack([y + 1.596027 * v, y - 0.812968 * v - 0.391762 * u, y + 2.017232 * u], axis=-1)
        want = np.clip(np.rint(real), 0, 255).astype(np.int64)
        got = yr.yuv_to_rgb(np.int32(Y), U, V).astype(np.int64)
        worst = np.maximum(worst, np.abs(got - want).reshape(-1, 3).max(axis=0))
    assert list(worst) == [1, 1, 1], worst


def test_equals_opencv_where_it_is_importable():
    cv2 = pytest.importorskip("cv2", reason="OpenCV is not installed: parity with cvtColor's bits stays unpinned here")
    buf = yr.all_triples_frame()
    for nv21, code in ((False, cv2.COLOR_YUV2RGB_NV12), (True, cv2.COLOR_YUV2RGB_NV21)):
        got = cv2.cvtColor(buf.reshape(4096 * 3 // 2, 4096), code)
        assert np.array_equal(got, yr.nv_to_rgb(buf, 4096, 4096, nv21)), nv21


def test_all_triples_frame_enumerates_every_triple_once():
    buf = yr.all_triples_frame()
    Y, U, V = yr.planes(buf, 4096, 4096)
    up = lambda c: np.repeat(np.repeat(c, 2, axis=0), 2, axis=1)
    key = (Y.astype(np.int64) << 16) | (up(U).astype(np.int64) << 8) | up(V)
    assert np.array_equal(np.sort(key.ravel()), np.arange(1 << 24))


def test_frozen_fixture_is_what_the_restatement_gives():
    z = np.load(GOLDEN)
    names = sorted({k.split("/")[0] for k in z.files})
    assert len(names) >= 5
    for n in names:
        rows, cols, nv21, stride, off = (int(x) for x in z[n + "/geom"])
        assert np.array_equal(yr.nv_to_rgb(z[n + "/frame"], rows, cols, bool(nv21), stride, off), z[n + "/rgb"]), n


# ---------------------------------------------------------------- the library's host arithmetic (no GPU)

def _frame_bytes(pix, rows, cols, stride=0):
    out = C.c_int64(-1)
    rc = capi.load().acf_hip_u8_frame_bytes(pix, rows, cols, stride, C.byref(out))
    return rc, out.value


def test_u8_frame_bytes_for_all_seven_layouts():
    H, W = 1080, 1920
    for pix, cpp in capi.PIX_CPP.items():
        assert _frame_bytes(pix, H, W) == (capi.OK, H * W * cpp), pix
        assert _frame_bytes(pix, H, W, W * cpp + 64) == (capi.OK, H * (W * cpp + 64)), pix
        assert _frame_bytes(pix, 7, 5) == (capi.OK, 35 * cpp), pix           # the packed layouts take any size
    for pix in (capi.PIX_NV12, capi.PIX_NV21):
        assert _frame_bytes(pix, H, W) == (capi.OK, H * W * 3 // 2), pix     # 3110400: half of RGB's 6220800
        assert _frame_bytes(pix, H, W, 2048) == (capi.OK, 2048 * H * 3 // 2), pix
        assert _frame_bytes(pix, 2, 2) == (capi.OK, 6), pix
        assert _frame_bytes(pix, 66, 130, 131) == (capi.OK, 131 * 99), pix   # an odd stride is a stride
    assert (capi.PIX_NV12, capi.PIX_NV21) == (5, 6)


def test_u8_frame_bytes_refuses_what_no_frame_has():
    bad = [(9, 4, 4, 0), (-1, 4, 4, 0), (7, 4, 4, 0),                          # unknown layouts
           (capi.PIX_RGB, 0, 4, 0), (capi.PIX_RGB, 4, 0, 0), (capi.PIX_NV12, -2, 4, 0),
           (capi.PIX_RGB, 4, 4, 11), (capi.PIX_BGRA, 4, 4, 15), (capi.PIX_GRAY, 4, 4, 3), (capi.PIX_NV12, 4, 4, 3), (capi.PIX_RGB, 4, 4, -12),
           (capi.PIX_NV12, 5, 4, 0), (capi.PIX_NV12, 4, 5, 0), (capi.PIX_NV21, 3, 3, 0)]  # odd NV12 / NV21 sizes
    for pix, rows, cols, stride in bad:
        assert _frame_bytes(pix, rows, cols, stride)[0] == capi.E_INVALID, (pix, rows, cols, stride)
    assert capi.load().acf_hip_u8_frame_bytes(capi.PIX_RGB, 4, 4, 0, None) == capi.E_INVALID


def test_python_handle_sizes_frames_through_the_library():
    from acf_amd.detector import HipDetector, HipError
    assert HipDetector.u8_frame_bytes(capi.PIX_NV12, 480, 640) == 460800
    assert HipDetector.u8_frame_bytes(capi.PIX_BGRA, 480, 640, 2600) == 480 * 2600
    with pytest.raises(HipError):
        HipDetector.u8_frame_bytes(capi.PIX_NV21, 481, 640)
