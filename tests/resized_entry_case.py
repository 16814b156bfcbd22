"""The resized tensor and YUV entries (include/acf_hip.h: acf_hip_pyramid_yuv_resized / run_yuv_resized / pyramid_image_resized /
run_image_resized / stream_open_yuv_resized): the case table and what the CPU and GPU tests share.  Helper of
tests/test_resized_entries.py and tests/test_gpu_resized_entries.py.

A case is two frames (so that stride_n matters) at the smallest shape at which its fork can go wrong.  build(case) writes the frames
out by hand and gives the descriptor, the buffer, and `packed`: the upright interleaved 8-bit image the entry's definition names —
for YUV the R, G, B bytes of the numpy restatement (tests/yuv_desc_ref.py), for an image the addressed bytes — i.e. what the chain
of existing entries starts from.  expected(oracle, case) is the oracle chain on `packed`: oracle.resize_u8 -> acfo_ingest_u8 ->
chnsPyramid -> acfDetect, computed once per process and shared."""
import numpy as np

import yuv_desc_ref as ydr
from acf_amd import capi, synth
from acf_amd.detector import HipDetector

NF = 2
S150 = HipDetector.resize_scale(80, 150)   # 0.5333...: INTER_AREA, fractional
S64 = HipDetector.resize_scale(80, 64)     # 1.25: INTER_LINEAR, enlarging

FACE80 = dict(seed=3, name="FACE80", nTrees=64, cascThr=-4.0)          # isLuv = 1: the planes pass through
FACE80_RGB = dict(FACE80, isLuv=0)                                     # rgb2luv on R, G, B
FACE80_HSV = dict(FACE80, isLuv=0, colorSpace=capi.CS_HSV)             # planar to d_stage, then k_rgb2hsv
FACE64 = dict(seed=3, name="FACE64", nTrees=64, cascThr=-4.0)          # grey, one plane

# name, source rows, cols, reduced rows, cols, scale, resize form, input, model, input planes
CASES = [
    ("i420_area_frac", 240, 320, 128, 171, S150, "area", "i420", FACE80, 3),                # x tile edge
    ("nv12_linear_up", 240, 320, 300, 400, S64, "linear", "nv12", FACE80, 3),               # y tile edge
    ("yuyv_padded_half", 240, 320, 120, 160, 0.5, "area_int", "yuyv_padded", FACE80_RGB, 3),  # 2 x 2; rgb2luv_sse body
    ("i444_odd_third", 299, 401, 100, 134, 1.0 / 3.0, "area_int", "i444_odd", FACE80_RGB, 3),  # partial edge cells
    ("planes_odd_037", 241, 321, 89, 119, 0.37, "area", "three_planes", FACE80_RGB, 3),     # odd reduced size: scalar rgb2luv, no float4
    ("nchw_area_frac", 240, 320, 128, 171, S150, "area", "nchw", FACE80_RGB, 3),
    ("bgr_packed_half", 240, 320, 120, 160, 0.5, "area_int", "bgr", FACE80, 3),              # stride_c -1, stride_x 3, base + 2
    ("rgba_linear_up_hsv", 240, 320, 300, 400, S64, "linear", "rgba", FACE80_HSV, 3),       # alpha skipped; the d_stage route
    ("gray_064", 240, 320, 154, 205, 0.64, "area", "gray", FACE64, 1),
    # (both reduce to two whole 64-pixel tiles and a ragged one on each axis)
    ("i420_gray_frac", 246, 326, 131, 174, S150, "area", "i420", FACE64, 3),                # rgb2gray on a YUV frame's R, G, B
    ("nchw_odd_037", 353, 359, 131, 133, 0.37, "area", "nchw", FACE80_RGB, 3),              # an image into the scalar rgb2luv, no float4
]
IDS = [c[0] for c in CASES]
YUV_INPUTS = ("i420", "nv12", "yuyv_padded", "i444_odd", "three_planes")


def form_of(scale):
    """The form cv::resize takes for the apps' Resizer (host_plan.cpp buildResizeTables): INTER_AREA when scale < 1 — integral where
    1 / scale is an integer — else INTER_LINEAR."""
    sc = 1.0 / scale
    if scale < 1.0 and sc >= 1:
        return "area_int" if abs(sc - round(sc)) < 2.220446049250313e-16 else "area"
    return "linear"


def rgb_u8(seed, h, w):
    """A video-like upright frame, uint8 [h][w][3]."""
    return np.clip(np.rint(synth.make_frame(seed, h, w, "rgb").transpose(2, 1, 0) * 255.0), 0, 255).astype(np.uint8)


def yuv_planes(seed, h, w, sx, sy):
    """Video-like Y [h][w] (limited range) and U, V [ceil(h / 2^sy)][ceil(w / 2^sx)] around 128, from the synthetic frame's planes."""
    p = synth.make_frame(seed, h, w, "rgb").transpose(0, 2, 1)                               # [3][h][w] in [0, 1]
    Y = np.rint(16 + 219 * p[0]).astype(np.uint8)
    U = np.rint(128 + 90 * (p[1] - 0.5)).astype(np.uint8)[::1 << sy, ::1 << sx]
    V = np.rint(128 + 90 * (p[2] - 0.5)).astype(np.uint8)[::1 << sy, ::1 << sx]
    return Y, np.ascontiguousarray(U), np.ascontiguousarray(V)


def _place(buf, at, P, stride):
    """Plane P into the flat buffer at byte `at`, rows `stride` bytes apart."""
    r, c = P.shape
    idx = at + stride * np.arange(r)[:, None] + np.arange(c)[None, :]
    buf[idx] = P


class Built:
    """kind "yuv" or "image"; desc: capi.YuvDesc / capi.ImageDesc at the source size; buf: the flat uint8 buffer, the entry's base
    pointer at buf[base]; packed: uint8 [NF][rows][cols][cn]; pix: the layout run_u8 takes `packed` as; frame_bytes (named YUV
    layouts: what a stream copies per frame, else 0); planes: the Y, U, V views' (offset, shape, strides) of "three_planes"."""

    def __init__(self, **kw):
        self.frame_bytes = 0
        self.planes = None
        self.__dict__.update(kw)


def build(case):
    name, H, W, dr, dc, scale, form, inp, model, d_in = case
    seed0 = 40 + 7 * IDS.index(name)
    if inp in ("i420", "nv12", "yuyv_padded"):
        lay = inp.split("_")[0]
        sx, sy = ydr.SUB[lay]
        stride = 2 * W + 32 if inp == "yuyv_padded" else 0
        desc, fb = HipDetector.yuv_desc(lay, H, W, stride)
        planes = [yuv_planes(seed0 + f, H, W, sx, sy) for f in range(NF)]
        buf = np.concatenate([ydr.pack(lay, Y, U, V, stride) for Y, U, V in planes])
        assert buf.size == fb * NF
        return Built(kind="yuv", desc=desc, buf=buf, base=0, packed=ydr.desc_to_rgb(buf, desc, H, W, NF), pix=capi.PIX_RGB, frame_bytes=fb)
    if inp == "i444_odd":
        # three full planes of 299 x 401 behind one another, rows 404 bytes apart, 5 bytes in front
        ys = 404
        fb = 3 * ys * H
        buf = np.full(5 + NF * fb, 0x5A, np.uint8)
        for f in range(NF):
            for i, P in enumerate(yuv_planes(seed0 + f, H, W, 0, 0)):
                _place(buf, 5 + f * fb + i * ys * H, P, ys)
        desc = capi.YuvDesc(capi.YuvPlane(0, fb, ys, 1), capi.YuvPlane(ys * H, fb, ys, 1), capi.YuvPlane(2 * ys * H, fb, ys, 1), 0, 0)
        return Built(kind="yuv", desc=desc, buf=buf, base=5, packed=ydr.desc_to_rgb(buf, desc, H, W, NF, 5), pix=capi.PIX_RGB)
    if inp == "three_planes":
        # a software decoder's frame: three allocations wherever they lie — here U, then V, then Y in one arena with gaps, so that both
        # chroma planes lie BELOW the base (negative offsets); 4:2:0 with ceil-sized chroma planes of 121 x 161
        ch, cw = (H + 1) >> 1, (W + 1) >> 1
        u_at, v_at = 3, 3 + NF * ch * cw + 61
        y_at = v_at + NF * ch * cw + 29
        buf = np.full(y_at + NF * H * W, 0x5A, np.uint8)
        for f in range(NF):
            Y, U, V = yuv_planes(seed0 + f, H, W, 1, 1)
            assert U.shape == (ch, cw)
            _place(buf, y_at + f * H * W, Y, W)
            _place(buf, u_at + f * ch * cw, U, cw)
            _place(buf, v_at + f * ch * cw, V, cw)
        desc = capi.YuvDesc(capi.YuvPlane(0, H * W, W, 1), capi.YuvPlane(u_at - y_at, ch * cw, cw, 1), capi.YuvPlane(v_at - y_at, ch * cw, cw, 1), 1, 1)
        planes = [(y_at, (NF, H, W)), (u_at, (NF, ch, cw)), (v_at, (NF, ch, cw))]
        return Built(kind="yuv", desc=desc, buf=buf, base=y_at, packed=ydr.desc_to_rgb(buf, desc, H, W, NF, y_at), pix=capi.PIX_RGB, planes=planes)
    rgb = np.stack([rgb_u8(seed0 + f, H, W) for f in range(NF)])                             # [NF][H][W][3]
    if inp == "nchw":
        buf = np.ascontiguousarray(rgb.transpose(0, 3, 1, 2))
        desc = capi.ImageDesc(capi.T_U8, 3, 3 * H * W, H * W, W, 1)
        return Built(kind="image", desc=desc, buf=buf.ravel(), base=0, packed=rgb, pix=capi.PIX_RGB, shape=buf.shape, layout="nchw")
    if inp == "bgr":
        buf = np.ascontiguousarray(rgb[..., ::-1])                                           # B, G, R in memory
        desc = capi.ImageDesc(capi.T_U8, 3, 3 * H * W, -1, 3 * W, 3)
        return Built(kind="image", desc=desc, buf=buf.ravel(), base=2, packed=rgb, pix=capi.PIX_RGB)
    if inp == "rgba":
        buf = np.concatenate([rgb, np.full((NF, H, W, 1), 0xC3, np.uint8)], axis=3)
        desc = capi.ImageDesc(capi.T_U8, 3, 4 * H * W, 1, 4 * W, 4)
        return Built(kind="image", desc=desc, buf=buf.ravel(), base=0, packed=rgb, pix=capi.PIX_RGB)
    if inp == "gray":
        g = np.ascontiguousarray(rgb[..., 1:2])                                              # [NF][H][W][1]
        desc = capi.ImageDesc(capi.T_U8, 1, H * W, 0, W, 1)
        return Built(kind="image", desc=desc, buf=g.ravel(), base=0, packed=g, pix=capi.PIX_GRAY, shape=(NF, 1, H, W), layout="nchw")
    raise ValueError(inp)


_BUILT, _EXPECT = {}, {}


def built(case):
    if case[0] not in _BUILT:
        _BUILT[case[0]] = build(case)
    return _BUILT[case[0]]


def oracle_planar(oracle, red):
    """The oracle's 8-bit image entry on a tight upright image [rows][cols][cn] (cn 1 or 3) -> planar f32 [cn][cols][rows]."""
    red = np.ascontiguousarray(red)
    rows, cols, cn = red.shape
    out = oracle.aligned((cn, cols, rows))
    ro, go, bo = (0, 1, 2) if cn == 3 else (0, 0, 0)
    oracle.lib().acfo_ingest_u8(red.ctypes.data, rows, cols, cn, ro, go, bo, cols * cn, oracle.F(out), cn)
    return out


def expected(oracle, case, arith=0):
    """Per frame (pyramid, detections, hits) of the oracle chain on `packed`, and the plan; computed once per (case, arith)."""
    key = (case[0], arith)
    if key not in _EXPECT:
        name, H, W, dr, dc, scale, form, inp, model, d_in = case
        b = built(case)
        plan = oracle.Plan(synth.make_model(**model), dr, dc, d_in)
        if arith:
            oracle.set_x86_tables(*oracle.x86_fixture())
            oracle.set_approx(3)
        try:
            out = []
            for f in range(NF):
                red = oracle.resize_u8(b.packed[f], scale)
                assert red.shape == (dr, dc, b.packed.shape[3])
                pyr, _, _ = oracle.chns_pyramid(plan, oracle_planar(oracle, red))
                out.append((pyr,) + oracle.detect(plan, pyr))
        finally:
            if arith:
                oracle.set_approx(0)
        _EXPECT[key] = (plan, out)
    return _EXPECT[key]
