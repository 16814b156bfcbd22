"""Crops of the stored frame (include/acf_hip.h: acf_hip_cut_crops / cut_detections / crop_box / crop_bytes / crop_form; kernel
k_cut_crops): the header's definition restated in numpy, and the boxes and specs the CPU and GPU tests share.  Helper of
tests/test_cut_crops.py, tests/test_gpu_cut_crops.py and tests/test_host_cpp_cut_crops.py.

Every operation is a float32 operation rounded once, as the header says: numpy's float32 arithmetic is exactly that, so the GPU tests
compare raw bits.  The reference takes the UPRIGHT frame U [Hu][Wu][C] as exact float32 code values (for an image the addressed
elements, for YUV the integer R, G, B of the format's arithmetic, turned by tests/orient_ref.py) — never the stored frame."""
import numpy as np

from acf_amd import capi

F = np.float32
T_BYTES = {capi.T_U8: 1, capi.T_F16: 2, capi.T_BF16: 2, capi.T_F32: 4}


def crop_box(det, scale, grow):
    """acf_hip_crop_box: cv::Rect2f(o) * (1.f / scale), then grown about the centre; float32 [4]."""
    inv = F(1) if scale == 0 else F(1) / F(scale)
    x, y, w, h = (F(int(v)) * inv for v in det)
    cx, cy = x + w * F(0.5), y + h * F(0.5)
    w2, h2 = w * F(grow), h * F(grow)
    return np.array([cx - w2 * F(0.5), cy - h2 * F(0.5), w2, h2], dtype=F)


def box_ok(box):
    b = np.asarray(box, dtype=F)
    return bool(np.all(np.isfinite(b)) and b[2] > 0 and b[3] > 0)


def axis(b0, bs, n_out, s, n_pix):
    """(i0, i1, frac) of the n_out * s sample coordinates along an axis of n_pix pixels."""
    with np.errstate(over="ignore"):
        step = F(bs) / F(n_out * s)
        m = np.arange(n_out * s).astype(F)
        v = (F(b0) + (m + F(0.5)) * step) - F(0.5)
    v = np.maximum(v, F(0))
    v = np.minimum(v, F(n_pix - 1))
    assert v.dtype == F
    i0 = np.floor(v).astype(np.int64)
    return i0, np.minimum(i0 + 1, n_pix - 1), v - i0.astype(F)


def sample(U, box, oh, ow, s):
    """val [oh][ow][C] float32 of one box on the upright frame U [Hu][Wu][C] float32 (not yet scaled by unit)."""
    U = np.asarray(U)
    assert U.dtype == F and U.ndim == 3
    bx, by, bw, bh = (F(v) for v in box)
    r0, r1, fy = axis(by, bh, oh, s, U.shape[0])
    c0, c1, fx = axis(bx, bw, ow, s, U.shape[1])
    fx, fy = fx[None, :, None], fy[:, None, None]
    p00, p01, p10, p11 = U[r0][:, c0], U[r0][:, c1], U[r1][:, c0], U[r1][:, c1]
    with np.errstate(all="ignore"):
        top = p00 + fx * (p01 - p00)
        bot = p10 + fx * (p11 - p10)
        smp = (top + fy * (bot - top)).reshape(oh, s, ow, s, U.shape[2])
        acc = np.zeros((oh, ow, U.shape[2]), dtype=F)
        for a in range(s):
            for b in range(s):
                acc = acc + smp[:, a, :, b, :]
        val = acc * F(1.0 / (s * s))
    assert val.dtype == F
    return val


def bf16_bits(v):
    """float32 -> bfloat16 bits, round to nearest even (finite values)."""
    u = np.ascontiguousarray(v, dtype=F).view(np.uint32).astype(np.uint64)
    return ((u + 0x7fff + ((u >> 16) & 1)) >> 16).astype(np.uint16)


def finish(val, unit, dtype, layout):
    """val [oh][ow][C] -> the crop's elements as raw bits (uint8 / uint16 / uint32) in the spec's layout."""
    if dtype == capi.T_U8:
        out = np.clip(np.rint(val), 0, 255).astype(np.uint8)
    else:
        with np.errstate(all="ignore"):
            x = val * F(unit)
            out = x.view(np.uint32) if dtype == capi.T_F32 else (x.astype(np.float16).view(np.uint16) if dtype == capi.T_F16 else bf16_bits(x))
    return np.ascontiguousarray(out if layout == 1 else out.transpose(2, 0, 1))


def crop(U, box, oh, ow, s, unit, dtype, layout):
    """One crop of the upright frame U as raw bits; a bad box gives zeros."""
    if not box_ok(box):
        shape = (oh, ow, U.shape[2]) if layout == 1 else (U.shape[2], oh, ow)
        return np.zeros(shape, dtype={1: np.uint8, 2: np.uint16, 4: np.uint32}[T_BYTES[dtype]])
    return finish(sample(U, box, oh, ow, s), unit, dtype, layout)


def crops(Us, boxes, frames, oh, ow, s, unit, dtype, layout):
    """[n] crops: box i on upright frame frames[i] of Us [nF][Hu][Wu][C]; a frame index outside [0, nF) gives zeros."""
    bad = np.full(4, np.nan, dtype=F)
    return np.stack([crop(Us[f if 0 <= f < len(Us) else 0], b if 0 <= f < len(Us) else bad, oh, ow, s, unit, dtype, layout) for b, f in zip(boxes, frames)])


def raw_bits(a):
    """a device result copied to the host -> its raw bits, the type crop() returns"""
    a = np.ascontiguousarray(a)
    return a.view({1: np.uint8, 2: np.uint16, 4: np.uint32}[a.dtype.itemsize])


# ---------------------------------------------------------------- the boxes and specs of the GPU cases (the CPU test holds crop_form on them)

# (out_h, out_w, samples): 1 x 1, an odd size that is no multiple of anything, more than one pass of the 256 lanes, the workload's
SPECS = [(1, 1, 1), (7, 5, 1), (7, 5, 3), (64, 64, 2), (112, 112, 1), (8, 8, 2)]


def spec_of(oh, ow, s, dtype=capi.T_F32, layout=0, k=1, grow=1.0):
    return capi.CropSpec(oh, ow, s, dtype, layout, k, grow, 0)


def form(spec, box, Hu, Wu, C, sb):
    import ctypes as Ct
    out = Ct.c_int(-1)
    b = np.ascontiguousarray(box, dtype=F)
    rc = capi.load().acf_hip_crop_form(Ct.byref(spec), capi.fptr(b), Hu, Wu, C, sb, Ct.byref(out))
    assert rc == 0, rc
    return out.value


def boundary_boxes(spec, Hu, Wu, C, sb):
    """Two square boxes at the frame's centre, one just on each side of acf_hip_crop_form's staged / gather boundary: the widest staged
    one and the next width (steps of 1 / 4 pixel), found by asking the library.  None when this spec has no boundary inside the frame."""
    cx, cy = F(Wu) * F(0.5), F(Hu) * F(0.5)
    mk = lambda w: np.array([cx - F(w) * F(0.5), cy - F(w) * F(0.5), w, w], dtype=F)
    prev = None
    for q in range(1, 4 * max(Hu, Wu) + 1):
        w = F(q) * F(0.25)
        f = form(spec, mk(w), Hu, Wu, C, sb)
        if prev is not None and prev[1] == 0 and f == 1:
            return mk(prev[0]), mk(w)
        prev = (w, f)
    return None


def boxes_for(Hu, Wu, nF, spec, C, sb):
    """(boxes float32 [n][4], frame index int32 [n], what each is) for one source and spec: the issue's list."""
    W, H = F(Wu), F(Hu)
    rows = [
        ("inside, fractional", [3.3, 2.7, 17.6, 12.2], 0),
        ("inside, frame 1", [W * F(0.25) + F(0.125), H * F(0.25), W * F(0.5), H * F(0.5) + F(0.3)], nF - 1),
        ("over the left edge", [-4.5, 5.2, 15.0, 11.0], 0),
        ("over the top edge", [6.1, -3.7, 12.0, 14.0], nF - 1),
        ("over the right edge", [W - F(9.3), 4.0, 16.0, 13.0], 0),
        ("over the bottom edge", [5.5, H - F(6.6), 18.0, 12.5], nF - 1),
        ("wholly outside, beyond the corner", [W + F(5), H + F(3), 9.0, 9.0], 0),
        ("wholly outside, left", [-40.0, 6.0, 10.0, 10.0], nF - 1),
        ("narrower than one pixel", [10.3, 8.6, 0.6, 0.45], 0),
        ("the whole frame", [0.0, 0.0, W, H], nF - 1),
        ("far larger than the frame", [-3.0e4, -2.0e4, 6.0e4, 5.0e4], 0),
        ("NaN member", [np.nan, 2.0, 8.0, 8.0], 0),
        ("infinite width", [2.0, 2.0, np.inf, 8.0], 0),
        ("zero width", [4.0, 4.0, 0.0, 9.0], 0),
        ("negative height", [4.0, 4.0, 9.0, -2.0], 0),
        ("frame -1", [3.0, 3.0, 9.0, 9.0], -1),
        ("frame n_frames", [3.0, 3.0, 9.0, 9.0], nF),
    ]
    bb = boundary_boxes(spec, Hu, Wu, C, sb)
    if bb is not None:
        rows += [("boundary: the widest staged box", bb[0], 0), ("boundary: the next width, gather", bb[1], nF - 1)]
    return (np.array([np.asarray(r[1], dtype=F) for r in rows], dtype=F), np.array([r[2] for r in rows], dtype=np.int32), [r[0] for r in rows])
