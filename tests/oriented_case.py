"""The frames, models and sizes of the oriented-entry tests (tests/test_oriented_entries.py checks on the CPU that every one of them
detects something in every orientation; tests/test_gpu_oriented_entries.py runs them).  Nothing here calls the GPU."""
import functools

import numpy as np

import image_entry_case as iec
import orient_ref as orf
import yuv_desc_ref as ydr
from acf_amd import capi, synth

N_FRAMES = 2
MODELS = {
    "inria": dict(name="INRIA", nTrees=64, cascThr=-3.0, nOctUp=0),   # 128 x 64 padded window
    "face64": dict(name="FACE64", nTrees=128, cascThr=-4.0, minDs_h=32, minDs_w=32),   # a grey model: takes a one-plane image
    "tiny": dict(name="TINY", nTrees=96, cascThr=-3.0),               # 16 x 16: fits a frame of 40 rows
}
# source sizes (rows, cols); the upright frame is the transpose for odd rot
TILES3 = (130, 174)   # three tiles each way, ragged edges, H % 4 == 2
ODD = (131, 175)      # H * W % 4 == 1: the scalar rgb2luv body; ceil-sized chroma planes
THIN = (40, 203)      # one tile or less along an axis
VEC3 = (132, 136)     # three tiles each way, ragged edges of 4 and 8, H % 4 == 0 in every orientation: float4 stores
SUB_NAME = {(1, 1): "i420", (1, 0): "i422", (0, 0): "i444"}

# (model, source size, class) of every reference the GPU tests take: class = (sub_x, sub_y) for RGB from YUV planes of that
# subsampling, "gray" for one plane, "f16" / "bf16" for the 4:4:4 RGB as rounded float elements
USED = [("inria", TILES3, (1, 1)), ("inria", TILES3, (1, 0)), ("inria", TILES3, (0, 0)), ("face64", TILES3, "gray"), ("inria", TILES3, "f16"),
        ("inria", TILES3, "bf16"), ("inria", ODD, (1, 1)), ("inria", ODD, (1, 0)), ("inria", ODD, (0, 0)), ("tiny", THIN, (1, 1)), ("tiny", THIN, (0, 0)),
        ("tiny", TILES3, "f16"), ("face64", TILES3, "bf16"), ("face64", ODD, (1, 1)), ("face64", ODD, (1, 0)),
        ("tiny", THIN, (1, 0)), ("tiny", VEC3, "f16"), ("face64", VEC3, "bf16"), ("face64", VEC3, (1, 1))]


@functools.lru_cache(maxsize=None)
def model(key):
    return synth.make_model(seed=3, **MODELS[key])


@functools.lru_cache(maxsize=None)
def yuv_planes(size, sub):
    """[(Y, U, V)] * N_FRAMES of the subsampling class, every code value; chroma planes ceil-sized."""
    sx, sy = sub
    return [ydr.random_planes(70 + 10 * sx + sy + 100 * f + size[0], SUB_NAME[sub], *size) for f in range(N_FRAMES)]


@functools.lru_cache(maxsize=None)
def rgb_source(size, sub):
    """uint8 [n][rows][cols][3]: the R, G, B of the source frames (chroma chosen in source coordinates)."""
    return np.stack([ydr.planes_to_rgb(Y, U, V, *sub) for Y, U, V in yuv_planes(size, sub)])


def stored_float(size, dtype):
    """The 4:4:4 RGB as elements of a float type: (stored [n][3][rows][cols], their f32 values)."""
    v = rgb_source(size, (0, 0)).astype(np.float32) * np.float32(1.0 / 255.0)
    return iec.round_to(np.ascontiguousarray(v.transpose(0, 3, 1, 2)), dtype)


def upright_values(size, klass, code):
    """f32 [n][c][h][w]: the values the detector sees for a reference class in orientation `code`."""
    if klass in ("f16", "bf16"):
        v = stored_float(size, capi.T_F16 if klass == "f16" else capi.T_BF16)[1]
    else:
        u8 = rgb_source(size, (0, 0))[..., 1:2] if klass == "gray" else rgb_source(size, klass)
        v = u8.transpose(0, 3, 1, 2).astype(np.float32) * np.float32(1.0 / 255.0)      # float(v) * float(1 / 255.0), ACF.cpp:114-119
    return np.ascontiguousarray(orf.orient(v, code, axes=(2, 3)))


def oracle_counts(mkey, size, klass, code):
    """Detections per frame by the oracle alone."""
    from oracle import binding as ob
    v = upright_values(size, klass, code)
    n, c, h, w = v.shape
    plan = ob.Plan(model(mkey), h, w, c)
    out = []
    for f in range(n):
        pyr, _, _ = ob.chns_pyramid(plan, np.ascontiguousarray(v[f].transpose(0, 2, 1)))   # planes [c][W][H]
        out.append(len(ob.detect(plan, pyr)[0]))
    return out


def planar_buffer(planes, ystride, cstride, sub, lead=0, fill=0x5A):
    """Hand-packed planar frames (Y, then U, then V; any sizes, ceil-sized chroma) with the given strides, `lead` bytes in front
    -> (buffer, descriptor relative to buf[lead], frame bytes)."""
    h, w = planes[0][0].shape
    ch, cw = planes[0][1].shape
    fb = ystride * h + 2 * cstride * ch
    buf = np.full(lead + fb * len(planes), fill, np.uint8)
    for f, (Y, U, V) in enumerate(planes):
        fr = buf[lead + f * fb:lead + (f + 1) * fb]
        fr[:ystride * h].reshape(h, ystride)[:, :w] = Y
        fr[ystride * h:ystride * h + cstride * ch].reshape(ch, cstride)[:, :cw] = U
        fr[ystride * h + cstride * ch:].reshape(ch, cstride)[:, :cw] = V
    d = capi.YuvDesc(capi.YuvPlane(0, fb, ystride, 1), capi.YuvPlane(ystride * h, fb, cstride, 1), capi.YuvPlane(ystride * h + cstride * ch, fb, cstride, 1),
                     sub[0], sub[1])
    return buf, d, fb


def yuyv_buffer(planes, stride, lead=0, fill=0x5A):
    """Hand-packed YUYV frames of any width (an odd width ends on half a macropixel: Y0 U . V) -> (buffer, descriptor, frame bytes)."""
    h, w = planes[0][0].shape
    cw = (w + 1) // 2
    assert stride >= 4 * cw
    fb = stride * h
    buf = np.full(lead + fb * len(planes), fill, np.uint8)
    for f, (Y, U, V) in enumerate(planes):
        rows = buf[lead + f * fb:lead + (f + 1) * fb].reshape(h, stride)
        rows[:, 0:2 * w:2] = Y
        rows[:, 1:4 * cw:4] = U
        rows[:, 3:4 * cw:4] = V
    d = capi.YuvDesc(capi.YuvPlane(0, fb, stride, 2), capi.YuvPlane(1, fb, stride, 4), capi.YuvPlane(3, fb, stride, 4), 1, 0)
    return buf, d, fb
