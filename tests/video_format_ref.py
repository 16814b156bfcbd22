"""Video formats (include/acf_hip.h: acf_hip_yuv_format) restated in numpy: the constants derived with fractions.Fraction from
Kr / Kb (NOT copied from the library), a gather through a descriptor with 8- or 16-bit samples, the mask and shift, and the header's
formula in int64.  Helper of tests/test_video_format.py and tests/test_gpu_video_format.py; nothing here calls the library."""
from fractions import Fraction as F

import numpy as np

import yuv_desc_ref as ydr

BT601, BT709, BT2020 = 0, 1, 2
KRKB = {BT601: (F(299, 1000), F(114, 1000)), BT709: (F(2126, 10000), F(722, 10000)), BT2020: (F(2627, 10000), F(593, 10000))}
CVT_COLOR_601 = (1220542, 1673527, -852492, -409993, 2116026)  # cvtColor's, from coefficients rounded to three decimals (the header)


def _round(q):
    """round(2^20 * q), half away from zero, exactly."""
    q = q * (1 << 20)
    n = (abs(q) * 2 + 1) // 2
    return int(n if q >= 0 else -n)


def coeffs(bits, matrix, full_range):
    """[yoff, cmid, out_max, CY, CVR, CVG, CUG, CUB] by the header's definition."""
    kr, kb = KRKB[matrix]
    kg = 1 - kr - kb
    ly = F(1) if full_range else F(255, 219)
    lc = F(1) if full_range else F(255, 224)
    c = (_round(ly), _round(lc * 2 * (1 - kr)), _round(-lc * 2 * (1 - kr) * kr / kg), _round(-lc * 2 * (1 - kb) * kb / kg), _round(lc * 2 * (1 - kb)))
    if matrix == BT601 and not full_range:
        c = CVT_COLOR_601
    yoff = 0 if full_range else 16 << (bits - 8)
    omax = (1 << bits) - 1 if full_range else 255 << (bits - 8)
    return [yoff, 1 << (bits - 1), omax] + list(c)


def to_rgb(Y, U, V, bits, matrix, full_range):
    """Samples (already masked and shifted; U, V at Y's resolution) -> int64 [..., 3] R, G, B in [0, out_max]."""
    yoff, cmid, omax, cy, cvr, cvg, cug, cub = coeffs(bits, matrix, full_range)
    Y, U, V = (np.asarray(a).astype(np.int64) for a in (Y, U, V))
    y = np.maximum(0, Y - yoff) * cy + (1 << 19)
    u, v = U - cmid, V - cmid
    r = (y + cvr * v) >> 20
    g = (y + cvg * v + cug * u) >> 20
    b = (y + cub * u) >> 20
    return np.clip(np.stack([r, g, b], -1), 0, omax)


def gather(buf, desc, rows, cols, bits, shift, n=1, base=0):
    """Y [n][rows][cols], U, V [n][chroma rows][chroma cols] (int64 samples) as the descriptor addresses them in the flat uint8
    buffer `buf`, base pointer at buf[base]: one byte, or the little-endian word at the byte offset, >> shift, & mask."""
    buf = np.asarray(buf).view(np.uint8).ravel()
    sx, sy = int(desc.sub_x), int(desc.sub_y)
    out = []
    for i, p in enumerate((desc.y, desc.u, desc.v)):
        off, sn, sr, sp = ydr.plane_tuple(p)
        r, c = (rows, cols) if i == 0 else ((rows + sy) >> sy, (cols + sx) >> sx)
        idx = base + off + sn * np.arange(n)[:, None, None] + sr * np.arange(r)[None, :, None] + sp * np.arange(c)[None, None, :]
        hi = idx.max() + (1 if bits > 8 else 0)
        assert idx.min() >= 0 and hi < buf.size, (i, int(idx.min()), int(hi), buf.size)
        if bits == 8:
            out.append(buf[idx].astype(np.int64))
        else:
            w = buf[idx].astype(np.int64) | (buf[idx + 1].astype(np.int64) << 8)
            out.append((w >> shift) & ((1 << bits) - 1))
    return tuple(out)


def desc_to_rgb(buf, desc, rows, cols, fmt, n=1, base=0):
    """-> [n][rows][cols][3] R, G, B: uint8 for 8 bits, else uint16.  fmt = (bits, shift, matrix, full_range)."""
    bits, shift, matrix, full = fmt
    Y, U, V = gather(buf, desc, rows, cols, bits, shift, n, base)
    sx, sy = int(desc.sub_x), int(desc.sub_y)
    rgb = to_rgb(Y, ydr.upsample(U, rows, cols, sx, sy), ydr.upsample(V, rows, cols, sx, sy), bits, matrix, full)
    return rgb.astype(np.uint8 if bits == 8 else np.uint16)


def rgb_to_f32(rgb, fmt):
    """The packed float32 image the entries for more than 8 bits are defined on: float(R) * float(1.0 / out_max)."""
    omax = coeffs(fmt[0], fmt[2], fmt[3])[2]
    return rgb.astype(np.float32) * np.float32(1.0 / omax)


def extent(desc, rows, cols, bits, n=1):
    """(first[3], last[3]) in bytes; last is the high byte of the last word for 16-bit samples."""
    sx, sy = int(desc.sub_x), int(desc.sub_y)
    first, last = [], []
    for i, p in enumerate((desc.y, desc.u, desc.v)):
        off, sn, sr, sp = ydr.plane_tuple(p)
        r, c = (rows, cols) if i == 0 else ((rows + sy) >> sy, (cols + sx) >> sx)
        first.append(off)
        last.append(off + (n - 1) * sn + (r - 1) * sr + (c - 1) * sp + (1 if bits > 8 else 0))
    return first, last


# ---- the named layouts with 16-bit words, written out by hand (no descriptor) ----

def pack16(name, Y, U, V, shift, stride=0, fill=0xA5A5):
    """One frame of the named layout of 16-bit words (sample << shift; the bits outside the sample field are zero: a test that wants
    them set ORs them in afterwards) as a flat uint8 buffer; stride in BYTES between luma rows (0 = tight)."""
    rows, cols = Y.shape
    sx, sy = ydr.SUB[name]
    Y, U, V = (np.asarray(a).astype(np.uint16) << shift for a in (Y, U, V))
    if name in ydr.PACKED_ORDER:
        sw = (stride or 4 * cols) // 2
        buf = np.full(sw * rows, fill, np.uint16)
        img = buf.reshape(rows, sw)[:, :2 * cols].reshape(rows, cols // 2, 4)
        src = {"u": U, "v": V}
        ny = 0
        for b, ch in enumerate(ydr.PACKED_ORDER[name]):
            if ch == "y":
                img[:, :, b] = Y[:, ny::2]
                ny += 1
            else:
                img[:, :, b] = src[ch]
        return buf.view(np.uint8)
    sw = (stride or 2 * cols) // 2
    if name in ("nv12", "nv21"):
        buf = np.full(sw * rows + sw * (rows // 2), fill, np.uint16)
        buf[:sw * rows].reshape(rows, sw)[:, :cols] = Y
        ch = buf[sw * rows:].reshape(rows // 2, sw)[:, :cols].reshape(rows // 2, cols // 2, 2)
        ch[:, :, 0], ch[:, :, 1] = (V, U) if name == "nv21" else (U, V)
        return buf.view(np.uint8)
    cw, crows = sw >> sx, rows >> sy
    buf = np.full(sw * rows + 2 * cw * crows, fill, np.uint16)
    buf[:sw * rows].reshape(rows, sw)[:, :cols] = Y
    first, second = (V, U) if name == "yv12" else (U, V)
    at = sw * rows
    for P in (first, second):
        buf[at:at + cw * crows].reshape(crows, cw)[:, :P.shape[1]] = P
        at += cw * crows
    return buf.view(np.uint8)


def random_planes16(seed, name, rows, cols, bits):
    """Y, U, V of every code value of `bits` bits."""
    rng = np.random.RandomState(seed)
    cs = ydr.chroma_shape(name, rows, cols)
    return tuple(rng.randint(0, 1 << bits, s).astype(np.uint16) for s in ((rows, cols), cs, cs))
