"""Shared case table and helpers of the image entry for upright device tensors (acf_hip_pyramid_image / acf_hip_run_image):
tests/test_image_entry.py (CPU: extents, the precondition that every case detects something) and tests/test_gpu_image_entry.py.

A frame is synth.make_frame(seed, H, W, kind) rounded to the case's element type, laid out by the case's strides inside a larger
buffer whose other elements are NaN (floats) or 0xA5 (bytes); `planes` are the f32 planes [c][W][H] the oracle reads.
"""
import functools

import numpy as np

from acf_amd import capi, synth

N_FRAMES = 3
SEED0 = 40

_TINY = dict(name="TINY", nTrees=96, cascThr=-3.0)


def _nchw(c, H, W):
    return (c * H * W, H * W, W, 1)


# name, H, W, dtype, d_in, frame kind, model kwargs, (stride_n, stride_c, stride_y, stride_x) in elements, base element, buffer elements
# (None: exactly up to the last addressed element, so the view ends with its allocation)
def _cases():
    out = []

    def add(name, H, W, dtype, d_in, kind, model, strides, base=0, size=None):
        out.append(dict(name=name, H=H, W=W, dtype=dtype, d_in=d_in, kind=kind, model=model, strides=strides, base=base, size=size))

    # contiguous NCHW: planar vector loads, fused vector rgb2luv
    add("nchw_f32_luv_vec", 240, 320, capi.T_F32, 3, "rgb", dict(name="INRIA", nTrees=128, cascThr=-2.5), _nchw(3, 240, 320))
    # channels_last memory behind an [n, 3, H, W] shape, one element into the buffer: tile edges on both axes, H * W % 4 != 0
    add("nhwc_f32_luv_scalar", 131, 175, capi.T_F32, 3, "rgb", dict(name="INRIA", nTrees=64, nOctUp=0, cascThr=-2.5),
        (131 * 175 * 3, 1, 175 * 3, 3), base=1)
    # the view [:, :, 5:101, 3:131] of a 120 x 160 tensor: padded rows, odd base, isLuv pass-through
    add("f16_roi_passthrough", 96, 128, capi.T_F16, 3, "luv", _TINY, _nchw(3, 120, 160), base=5 * 160 + 3, size=N_FRAMES * 3 * 120 * 160)
    # [n, H, W, 4][..., :3] seen as [n, 3, H, W]: the fourth element of every pixel is skipped
    add("bf16_rgba_skip", 120, 160, capi.T_BF16, 3, "rgb", dict(name="FACE64", nTrees=128, minDs_h=32, minDs_w=32, cascThr=-4.0),
        (120 * 160 * 4, 1, 160 * 4, 4), size=N_FRAMES * 120 * 160 * 4)
    add("u8_nchw_gray1", 240, 320, capi.T_U8, 1, "gray", dict(name="FACE64", nTrees=128, cascThr=-2.5), _nchw(1, 240, 320))
    add("u8_nchw_hsv", 120, 160, capi.T_U8, 3, "rgb", dict(name="INRIA", nTrees=64, nOctUp=0, colorSpace=capi.CS_HSV, cascThr=-3.0), _nchw(3, 120, 160))
    # packed BGR: the pointer at the R of the first pixel, channels backwards
    add("bgr_negative_stride", 96, 128, capi.T_F32, 3, "luv", _TINY, (96 * 128 * 3, -1, 128 * 3, 3), base=2)
    # 3 x 3 ragged tiles with a ragged width of 6 (not a multiple of 16), through conversions and load forms the rows above do not pair:
    # packed bytes into the vector rgb2luv body (H % 4 == 0: float4 stores); every second f16 element of a row (the element-wise form)
    # into rgb2gray (H % 4 == 2: scalar stores, a last quad of two rows)
    add("u8_nhwc_luv_vec_ragged", 132, 134, capi.T_U8, 3, "rgb", dict(name="INRIA", nTrees=64, nOctUp=0, cascThr=-2.5), (132 * 134 * 3, 1, 134 * 3, 3))
    add("f16_stride2_gray_ragged", 130, 134, capi.T_F16, 3, "rgb", dict(name="FACE64", nTrees=128, minDs_h=32, minDs_w=32, cascThr=-4.0),
        (3 * 130 * 134 * 2, 130 * 134 * 2, 134 * 2, 2))
    # the element type x conversion pairs no row above takes: element-wise and packed at 132 x 134, then the row-vector form on rows of 136
    # (four-element aligned, a ragged width of 8)
    add("bf16_stride2_luv_vec_ragged", 132, 134, capi.T_BF16, 3, "rgb", dict(name="INRIA", nTrees=64, nOctUp=0, cascThr=-2.5),
        (3 * 132 * 134 * 2, 132 * 134 * 2, 134 * 2, 2))
    add("f16_nhwc_luv_vec_ragged", 132, 134, capi.T_F16, 3, "rgb", dict(name="INRIA", nTrees=64, nOctUp=0, cascThr=-2.5), (132 * 134 * 3, 1, 134 * 3, 3))
    add("f32_nchw_gray_ragged", 130, 136, capi.T_F32, 3, "rgb", dict(name="FACE64", nTrees=128, minDs_h=32, minDs_w=32, cascThr=-4.0), _nchw(3, 130, 136))
    add("bf16_nchw_isluv_ragged", 130, 136, capi.T_BF16, 3, "luv", _TINY, _nchw(3, 130, 136))
    return out


CASES = _cases()
CASE_IDS = [c["name"] for c in CASES]

NP_STORAGE = {capi.T_U8: np.uint8, capi.T_F16: np.float16, capi.T_BF16: np.uint16, capi.T_F32: np.float32}


def case(name):
    return next(c for c in CASES if c["name"] == name)


def round_to(v, dtype):
    """f32 array -> (the stored elements, the f32 values the entry reads back from them)."""
    v = np.ascontiguousarray(v, np.float32)
    if dtype == capi.T_F32:
        return v, v
    if dtype == capi.T_F16:
        s = v.astype(np.float16)
        return s, s.astype(np.float32)
    if dtype == capi.T_BF16:
        u = v.view(np.uint32).astype(np.uint64)
        hi = ((u + 0x7FFF + ((u >> 16) & 1)) >> 16).astype(np.uint16)      # round to nearest even, the upper 16 bits
        return hi, (hi.astype(np.uint32) << 16).view(np.float32)
    s = np.clip(np.rint(v.astype(np.float64) * 255.0), 0, 255).astype(np.uint8)
    return s, s.astype(np.float32) * np.float32(1.0 / 255.0)               # float(v) * float(1 / 255.0), ACF.cpp:114-119


def extent(strides, channels, H, W, n):
    """The lowest and highest element offset a description addresses, by hand."""
    lo = hi = 0
    for cnt, s in zip((n, channels, H, W), strides):
        v = (cnt - 1) * s
        if v < 0:
            lo += v
        else:
            hi += v
    return lo, hi


def lay_out(upright, dtype, strides, base=0, size=None):
    """upright: stored elements [n][c][H][W] -> a 1-D buffer with element (n, c, y, x) at base + n * sn + c * sc + y * sy + x * sx and
    poison everywhere else (NaN; 0xA5 bytes)."""
    n, ch, H, W = upright.shape
    lo, hi = extent(strides, ch, H, W, n)
    assert base + lo >= 0
    size = size if size is not None else base + hi + 1
    assert base + hi < size
    if dtype == capi.T_U8:
        buf = np.full(size, 0xA5, np.uint8)
    elif dtype == capi.T_BF16:
        buf = np.full(size, 0x7FC0, np.uint16)
    else:
        buf = np.full(size, np.nan, NP_STORAGE[dtype])
    idx = base
    for axis, (cnt, s) in enumerate(zip((n, ch, H, W), strides)):
        shape = [1, 1, 1, 1]
        shape[axis] = cnt
        idx = idx + (np.arange(cnt, dtype=np.int64) * s).reshape(shape)
    buf[idx.ravel()] = upright.ravel()
    return buf


@functools.lru_cache(maxsize=None)
def build(name, n=N_FRAMES, seed0=SEED0):
    """-> dict(buf, planes [n][c][W][H] f32, desc = capi.ImageDesc, base, case, model)."""
    c = case(name)
    stored, planes = [], []
    for f in range(n):
        s, v = round_to(synth.make_frame(seed0 + f, c["H"], c["W"], c["kind"]), c["dtype"])   # [c][W][H]
        stored.append(s.transpose(0, 2, 1))                                                  # upright [c][H][W]
        planes.append(v)
    buf = lay_out(np.stack(stored), c["dtype"], c["strides"], c["base"], c["size"])
    desc = capi.ImageDesc(c["dtype"], c["d_in"], *c["strides"])
    return dict(buf=buf, planes=np.stack(planes), desc=desc, base=c["base"], case=c, model=synth.make_model(seed=3, **c["model"]))


@functools.lru_cache(maxsize=None)
def oracle_results(name, arith=False):
    """The oracle alone on the case's planes, once: [(pyramid, detections, hits)] per frame and the plan."""
    from oracle import binding as ob
    b = build(name)
    c = b["case"]
    plan = ob.Plan(b["model"], c["H"], c["W"], c["d_in"])
    out = []
    for f in range(N_FRAMES):
        if arith:
            ob.set_x86_tables(*ob.x86_fixture())
            ob.set_approx(3)
        try:
            pyr, _, _ = ob.chns_pyramid(plan, np.ascontiguousarray(b["planes"][f]))
        finally:
            if arith:
                ob.set_approx(0)
        det, hits = ob.detect(plan, pyr)
        out.append((pyr, det, hits))
    return plan, out


def to_device(buf, dtype):
    """The 1-D buffer as a device tensor of the case's element type."""
    import torch
    t = torch.from_numpy(buf).cuda()
    return t.view(torch.bfloat16) if dtype == capi.T_BF16 else t


def tensor_view(b, n=N_FRAMES):
    """The case as the [n, c, H, W] device view a torch user holds (slices, channels_last, [..., :3]): torch.as_strided of the buffer.
    Returns (view, the buffer's tensor: keep it alive)."""
    import torch
    c = b["case"]
    t = to_device(b["buf"], c["dtype"])
    return torch.as_strided(t, (n, c["d_in"], c["H"], c["W"]), c["strides"], c["base"]), t
