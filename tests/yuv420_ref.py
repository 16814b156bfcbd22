"""The YUV 4:2:0 (NV12 / NV21) -> RGB conversion of the 8-bit entries, restated in numpy (include/acf_hip.h "YUV 4:2:0 input"):
cvtColor(COLOR_YUV2RGB_NV12 / _NV21) as OpenCV's imgproc/src/color_yuv.simd.hpp publishes it — BT.601 limited range in 20-bit fixed
point, int32, arithmetic shift; the chroma pair of a 2 x 2 block shared by its four pixels.  Helper of tests/test_yuv420.py and
tests/test_gpu_yuv420.py; also makes their frames."""
import numpy as np

CY, CVR, CVG, CUG, CUB, SHIFT = 1220542, 1673527, -852492, -409993, 2116026, 20


def yuv_to_rgb(Y, U, V):
    """int arrays (broadcastable) of Y, U, V code values -> uint8 array [..., 3] of R, G, B."""
    Y, U, V = (np.asarray(a).astype(np.int32) for a in (Y, U, V))
    y = np.maximum(0, Y - 16) * np.int32(CY)
    u, v = U - 128, V - 128
    half = np.int32(1 << (SHIFT - 1))
    ruv = half + np.int32(CVR) * v
    guv = half + np.int32(CVG) * v + np.int32(CUG) * u
    buv = half + np.int32(CUB) * u
    out = np.stack(np.broadcast_arrays((y + ruv) >> SHIFT, (y + guv) >> SHIFT, (y + buv) >> SHIFT), axis=-1)  # >> on int32: floor
    assert out.dtype == np.int32
    return np.clip(out, 0, 255).astype(np.uint8)


def frame_bytes(rows, cols, stride=0, chroma_offset=0):
    stride = stride or cols
    return (chroma_offset or stride * rows) + stride * (rows // 2)


def planes(buf, rows, cols, nv21=False, stride=0, chroma_offset=0):
    """The Y [rows][cols], U and V [rows / 2][cols / 2] code values of one frame held in the flat uint8 buffer `buf`."""
    assert rows % 2 == 0 and cols % 2 == 0
    stride = stride or cols
    chroma_offset = chroma_offset or stride * rows
    assert stride >= cols and chroma_offset >= stride * rows and buf.size >= chroma_offset + stride * (rows // 2)
    Y = buf[:stride * rows].reshape(rows, stride)[:, :cols]
    C = buf[chroma_offset:chroma_offset + stride * (rows // 2)].reshape(rows // 2, stride)[:, :cols].reshape(rows // 2, cols // 2, 2)
    return Y, C[..., 1 if nv21 else 0], C[..., 0 if nv21 else 1]


def nv_to_rgb(buf, rows, cols, nv21=False, stride=0, chroma_offset=0):
    """One NV12 / NV21 frame -> uint8 [rows][cols][3] R, G, B."""
    Y, U, V = planes(np.asarray(buf, np.uint8).ravel(), rows, cols, nv21, stride, chroma_offset)
    up = lambda c: np.repeat(np.repeat(c, 2, axis=0), 2, axis=1)  # every 2 x 2 block takes its one pair
    return yuv_to_rgb(Y, up(U), up(V))


def pack(Y, U, V, nv21=False, stride=0, chroma_offset=0, total=0, fill=0xA5):
    """Y [rows][cols], U, V [rows / 2][cols / 2] -> the flat frame buffer (padding bytes = `fill`, `total` bytes long if given)."""
    rows, cols = Y.shape
    stride = stride or cols
    chroma_offset = chroma_offset or stride * rows
    buf = np.full(max(total, chroma_offset + stride * (rows // 2)), fill, np.uint8)
    buf[:stride * rows].reshape(rows, stride)[:, :cols] = Y
    C = np.stack([V, U] if nv21 else [U, V], axis=-1).reshape(rows // 2, cols)
    buf[chroma_offset:chroma_offset + stride * (rows // 2)].reshape(rows // 2, stride)[:, :cols] = C
    return buf


def from_rgb(rgb, nv21=False, stride=0, chroma_offset=0, total=0):
    """A plausible video frame from uint8 RGB [rows][cols][3] (test data only: the forward BT.601 matrix in floating point, chroma
    averaged over each 2 x 2 block).  What the frame then *means* is defined by nv_to_rgb alone."""
    r, g, b = (rgb[..., i].astype(np.float64) for i in range(3))
    y = 16 + (65.481 * r + 128.553 * g + 24.966 * b) / 255.0
    u = 128 + (-37.797 * r - 74.203 * g + 112.0 * b) / 255.0
    v = 128 + (112.0 * r - 93.786 * g - 18.214 * b) / 255.0
    rows, cols = y.shape
    sub = lambda c: c.reshape(rows // 2, 2, cols // 2, 2).mean(axis=(1, 3))
    q = lambda c: np.clip(np.rint(c), 0, 255).astype(np.uint8)
    return pack(q(y), q(sub(u)), q(sub(v)), nv21, stride, chroma_offset, total)


def random_frame(seed, rows, cols, nv21=False, stride=0, chroma_offset=0, total=0):
    """Every code value, the out-of-range ones (Y < 16, Y > 235, saturating chroma) included."""
    rng = np.random.RandomState(seed)
    Y = rng.randint(0, 256, (rows, cols)).astype(np.uint8)
    U = rng.randint(0, 256, (rows // 2, cols // 2)).astype(np.uint8)
    V = rng.randint(0, 256, (rows // 2, cols // 2)).astype(np.uint8)
    return pack(Y, U, V, nv21, stride, chroma_offset, total)


def all_triples_frame():
    """A 4096 x 4096 NV12 frame whose 2 x 2 blocks enumerate every (U, V) 64 times, each with four luma values, so that every
    (Y, U, V) triple occurs exactly once: block (by, bx) has U = bx & 255, V = by & 255 and
    Y = 4 * (8 * (by >> 8) + (bx >> 8)) + (2 * (row & 1) + (col & 1))."""
    by, bx = np.meshgrid(np.arange(2048), np.arange(2048), indexing="ij")
    U, V = (bx & 255).astype(np.uint8), (by & 255).astype(np.uint8)
    base = 4 * (8 * (by >> 8) + (bx >> 8))
    Y = np.zeros((4096, 4096), np.uint8)
    for j in range(2):
        for i in range(2):
            Y[j::2, i::2] = base + 2 * j + i
    return pack(Y, U, V)
