"""Three-plane YUV descriptors (include/acf_hip.h: acf_hip_yuv_desc) restated in numpy: the named layouts packed by hand, a gather
through any descriptor, and the conversion by tests/yuv420_ref.py's per-pixel formula.  Helper of tests/test_yuv_desc.py and
tests/test_gpu_yuv_desc.py; nothing here calls the library — the descriptors it is given come from the tests."""
import numpy as np

import yuv420_ref as yr

NAMES = ["nv12", "nv21", "i420", "yv12", "i422", "i444", "yuyv", "uyvy", "yvyu"]
SUB = {"nv12": (1, 1), "nv21": (1, 1), "i420": (1, 1), "yv12": (1, 1), "i422": (1, 0), "i444": (0, 0), "yuyv": (1, 0), "uyvy": (1, 0), "yvyu": (1, 0)}
PACKED_ORDER = {"yuyv": "yuyv", "uyvy": "uyvy", "yvyu": "yvyu"}  # the macropixel's bytes, y = Y0 then Y1


def chroma_shape(name, rows, cols):
    sx, sy = SUB[name]
    return (rows + sy) >> sy, (cols + sx) >> sx


def random_planes(seed, name, rows, cols):
    """Y [rows][cols], U, V [chroma rows][chroma cols], every code value (the out-of-range ones included)."""
    rng = np.random.RandomState(seed)
    cs = chroma_shape(name, rows, cols)
    return tuple(rng.randint(0, 256, s).astype(np.uint8) for s in ((rows, cols), cs, cs))


def pack(name, Y, U, V, stride=0, fill=0xA5):
    """One frame of the named layout as a flat uint8 buffer, written out by hand (no descriptor): `stride` bytes between luma rows
    (0 = tight); planar chroma planes at stride >> sub_x, tight behind one another."""
    rows, cols = Y.shape
    sx, sy = SUB[name]
    if name in PACKED_ORDER:
        stride = stride or 2 * cols
        buf = np.full(stride * rows, fill, np.uint8)
        img = buf.reshape(rows, stride)[:, :2 * cols].reshape(rows, cols // 2, 4)
        src = {"u": U, "v": V}
        ny = 0
        for b, ch in enumerate(PACKED_ORDER[name]):
            if ch == "y":
                img[:, :, b] = Y[:, ny::2]
                ny += 1
            else:
                img[:, :, b] = src[ch]
        return buf
    stride = stride or cols
    if name in ("nv12", "nv21"):
        return yr.pack(Y, U, V, name == "nv21", stride, fill=fill)
    cstride, crows = stride >> sx, rows >> sy
    buf = np.full(stride * rows + 2 * cstride * crows, fill, np.uint8)
    buf[:stride * rows].reshape(rows, stride)[:, :cols] = Y
    first, second = (V, U) if name == "yv12" else (U, V)
    at = stride * rows
    for P in (first, second):
        buf[at:at + cstride * crows].reshape(crows, cstride)[:, :P.shape[1]] = P
        at += cstride * crows
    return buf


def plane_tuple(p):
    return int(p.offset), int(p.stride_n), int(p.stride_row), int(p.stride_px)


def gather(buf, desc, rows, cols, n=1, base=0):
    """Y [n][rows][cols], U, V [n][chroma rows][chroma cols] as the descriptor addresses them in the flat uint8 buffer `buf`, the
    base pointer at buf[base].  Asserts that every addressed byte lies inside the buffer."""
    buf = np.asarray(buf, np.uint8).ravel()
    sx, sy = int(desc.sub_x), int(desc.sub_y)
    out = []
    for i, p in enumerate((desc.y, desc.u, desc.v)):
        off, sn, sr, sp = plane_tuple(p)
        r, c = (rows, cols) if i == 0 else ((rows + sy) >> sy, (cols + sx) >> sx)
        idx = base + off + sn * np.arange(n)[:, None, None] + sr * np.arange(r)[None, :, None] + sp * np.arange(c)[None, None, :]
        assert idx.min() >= 0 and idx.max() < buf.size, (i, int(idx.min()), int(idx.max()), buf.size)
        out.append(buf[idx])
    return tuple(out)


def upsample(C, rows, cols, sx, sy):
    """Chroma [..., chroma rows, chroma cols] -> [..., rows, cols]: pixel (r, c) takes sample (r >> sy, c >> sx), no interpolation."""
    return C[..., np.arange(rows) >> sy, :][..., np.arange(cols) >> sx]


def planes_to_rgb(Y, U, V, sx, sy):
    """-> uint8 [..., rows, cols, 3] R, G, B by the header's formula (yuv420_ref.yuv_to_rgb)."""
    rows, cols = Y.shape[-2:]
    return yr.yuv_to_rgb(Y, upsample(U, rows, cols, sx, sy), upsample(V, rows, cols, sx, sy))


def desc_to_rgb(buf, desc, rows, cols, n=1, base=0):
    Y, U, V = gather(buf, desc, rows, cols, n, base)
    return planes_to_rgb(Y, U, V, int(desc.sub_x), int(desc.sub_y))
