"""Crops of the stored frame on the GPU (include/acf_hip.h: acf_hip_cut_crops / acf_hip_cut_detections; kernel k_cut_crops, staged and
gather).  Every comparison is bit for bit (array_equal on the raw bits) against the numpy restatement of the header's definition
(tests/cut_crops_ref.py) fed with the UPRIGHT frame U, which is built as the oriented tests build it: the addressed tensor elements, or
the R, G, B of the format's arithmetic (tests/video_format_ref.py: what acf_hip_video_to_rgb writes), turned by np.rot90
(tests/orient_ref.py).  tests/test_cut_crops.py holds the preconditions: the restatement's own properties, and that the boxes below take
both forms.

Shapes: stored frames of 37 x 53 (odd) and 48 x 64, two frames (so that stride_n matters); crops of 1 x 1, 7 x 5, 64 x 64 and
112 x 112 (more than one pass of the 256 lanes; at 37 x 53 several bands or one), samples 1, 2, 3.  Sources are allocated exactly to
their extents; the destination is pre-filled with a sentinel and holds one slot more than the call writes."""
import ctypes as C

import numpy as np
import pytest

import cut_crops_ref as ccr
import orient_ref as orf
import oriented_case as oc
import resized_entry_case as rc
import video_format_ref as vfr
import yuv_desc_ref as ydr
from acf_amd import capi, synth
from acf_amd.detector import HipDetector, HipError

pytestmark = pytest.mark.gpu
F = np.float32
NF = 2
ODD, EVEN = (37, 53), (48, 64)
SENTINEL = 0xA5
NP_ELEM = {capi.T_U8: np.uint8, capi.T_F16: np.uint16, capi.T_BF16: np.uint16, capi.T_F32: np.uint32}
BT709_FULL = (8, 0, capi.YUV_MATRIX_BT709, 1)
P010 = (10, 6, capi.YUV_MATRIX_BT709, 0)
P10LE = (10, 0, capi.YUV_MATRIX_BT2020, 0)


class Source:
    """One stored input: the flat host buffer, how to describe it to the library, and S [NF][Hs][Ws][C], its exact float32 code values."""

    def __init__(self, name, buf, base, size, S, unit, codes8, sb, image=None, yuv=None, fmt=None):
        self.name, self.buf, self.base, self.size, self.S, self.unit, self.codes8, self.sb = name, buf, base, size, S, F(unit), codes8, sb
        self.image, self.yuv, self.fmt = image, yuv, fmt
        self.C = S.shape[3]

    def crop_source(self, det, x, code):
        ptr = x.data_ptr() + self.base
        if self.image is not None:
            return det.crop_source_image(ptr, NF, self.image, self.size[0], self.size[1], code)
        return det.crop_source_yuv(ptr, NF, self.yuv, HipDetector.video_format(*self.fmt) if self.fmt else None, self.size[0], self.size[1], code)

    def upright(self, code):
        return np.ascontiguousarray(orf.orient(self.S, code, axes=(1, 2)))


def _elements(seed, dtype, shape):
    """(raw elements, their exact float32 values)"""
    rng = np.random.RandomState(seed)
    if dtype == capi.T_U8:
        e = rng.randint(0, 256, shape).astype(np.uint8)
        return e, e.astype(F)
    v = (rng.rand(*shape) * 1.5 - 0.25).astype(F)
    if dtype == capi.T_F16:
        h = v.astype(np.float16)
        return h.view(np.uint16), h.astype(F)
    if dtype == capi.T_BF16:
        b = (v.view(np.uint32) >> 16).astype(np.uint16)
        return b, (b.astype(np.uint32) << 16).view(F)
    return v.view(np.uint32), v


def image_source(name, dtype, size, variant, seed):
    Hs, Ws = size
    ch = 1 if variant == "gray" else 3
    sn, sc, sy, sx = {
        "nchw": (ch * Hs * Ws, Hs * Ws, Ws, 1), "gray": (Hs * Ws, Hs * Ws, Ws, 1), "nhwc": (Hs * Ws * 3, 1, Ws * 3, 3), "bgr": (Hs * Ws * 3, -1, Ws * 3, 3),
        "padded": (3 * Hs * (Ws + 5) + 7, Hs * (Ws + 5), Ws + 5, 1)}[variant]
    desc = capi.ImageDesc(dtype, ch, sn, sc, sy, sx)
    first, last = HipDetector.image_extent(desc, Hs, Ws, NF)
    E, vals = _elements(seed, dtype, (NF, ch, Hs, Ws))
    flat = np.zeros(last - first + 1, dtype=E.dtype)                                         # exactly the extent
    n, c, y, x = np.meshgrid(np.arange(NF), np.arange(ch), np.arange(Hs), np.arange(Ws), indexing="ij")
    flat[-first + n * sn + c * sc + y * sy + x * sx] = E
    es = flat.dtype.itemsize
    return Source(name, flat.view(np.uint8), -first * es, size, np.ascontiguousarray(vals.transpose(0, 2, 3, 1)), 1 / 255.0 if dtype == capi.T_U8 else 1.0,
                  dtype == capi.T_U8, es, image=desc)


def yuv_source(name, layout, size, fmt, seed):
    Hs, Ws = size
    bits, shift = (fmt[0], fmt[1]) if fmt else (8, 0)
    f = fmt or (8, 0, capi.YUV_MATRIX_BT601, 0)
    sx, sy = ydr.SUB[layout]
    if bits > 8:
        desc, fb = HipDetector.video_desc(layout, Hs, Ws, HipDetector.video_format(*fmt))
        buf = np.concatenate([vfr.pack16(layout, *vfr.random_planes16(seed + i, layout, Hs, Ws, bits), shift) for i in range(NF)])
    elif Hs % 2 or Ws % 2:
        assert layout in ("i420", "i444")                                                    # hand-built: ceil-sized chroma planes, tight
        cw = (Ws + sx) >> sx
        buf, desc, fb = oc.planar_buffer([ydr.random_planes(seed + i, layout, Hs, Ws) for i in range(NF)], Ws, cw, (sx, sy))
    else:
        desc, fb = HipDetector.video_desc(layout, Hs, Ws)
        buf = np.concatenate([ydr.pack(layout, *ydr.random_planes(seed + i, layout, Hs, Ws)) for i in range(NF)])
    assert buf.size == NF * fb
    _, last = vfr.extent(desc, Hs, Ws, bits, NF)
    assert max(last) == buf.size - 1                                                         # nothing behind the last addressed byte
    S = vfr.desc_to_rgb(buf, desc, Hs, Ws, f, NF).astype(F)
    omax = vfr.coeffs(f[0], f[2], f[3])[2]
    return Source(name, buf, 0, size, S, 1 / 255.0 if bits == 8 else 1.0 / omax, bits == 8, 1 if bits == 8 else 2, yuv=desc, fmt=fmt)


# name -> (builder, orientation codes): every source takes a turn of its own; one image and one 4:2:0 layout take all eight
SOURCES = {
    "u8_nchw_odd": (lambda: image_source("u8_nchw_odd", capi.T_U8, ODD, "nchw", 11), range(8)),
    "i420_odd": (lambda: yuv_source("i420_odd", "i420", ODD, None, 12), range(8)),
    "f16_nchw_odd": (lambda: image_source("f16_nchw_odd", capi.T_F16, ODD, "nchw", 13), (3,)),
    "bf16_nhwc_even": (lambda: image_source("bf16_nhwc_even", capi.T_BF16, EVEN, "nhwc", 14), (5,)),
    "f32_nchw_even": (lambda: image_source("f32_nchw_even", capi.T_F32, EVEN, "nchw", 15), (1,)),
    "f32_padded_odd": (lambda: image_source("f32_padded_odd", capi.T_F32, ODD, "padded", 16), (6,)),
    "u8_nhwc_even": (lambda: image_source("u8_nhwc_even", capi.T_U8, EVEN, "nhwc", 17), (7,)),
    "u8_bgr_odd": (lambda: image_source("u8_bgr_odd", capi.T_U8, ODD, "bgr", 18), (2,)),
    "u8_padded_even": (lambda: image_source("u8_padded_even", capi.T_U8, EVEN, "padded", 19), (4,)),
    "u8_gray_odd": (lambda: image_source("u8_gray_odd", capi.T_U8, ODD, "gray", 20), (1,)),
    "f16_gray_even": (lambda: image_source("f16_gray_even", capi.T_F16, EVEN, "gray", 21), (0,)),
    "i420_even_709full": (lambda: yuv_source("i420_even_709full", "i420", EVEN, BT709_FULL, 22), (3,)),
    "nv12_even": (lambda: yuv_source("nv12_even", "nv12", EVEN, None, 23), (1, 6)),
    "nv12_even_709full": (lambda: yuv_source("nv12_even_709full", "nv12", EVEN, BT709_FULL, 24), (0,)),
    "yuyv_even": (lambda: yuv_source("yuyv_even", "yuyv", EVEN, None, 25), (5,)),
    "yuyv_even_709full": (lambda: yuv_source("yuyv_even_709full", "yuyv", EVEN, BT709_FULL, 26), (2,)),
    "i444_odd": (lambda: yuv_source("i444_odd", "i444", ODD, None, 27), (7,)),
    "i444_even_709full": (lambda: yuv_source("i444_even_709full", "i444", EVEN, BT709_FULL, 28), (4,)),
    "p010_even": (lambda: yuv_source("p010_even", "nv12", EVEN, P010, 29), (0, 1)),
    "yuv420p10le_even": (lambda: yuv_source("yuv420p10le_even", "i420", EVEN, P10LE, 30), (6,)),
}


@pytest.fixture(scope="module")
def det():
    d = HipDetector()                                                                        # a context; no model, no plan
    yield d
    d.close()


def dev(buf):
    import torch
    return torch.from_numpy(np.ascontiguousarray(buf)).cuda()


def cut(det, src, boxes, frames, spec, slack=1):
    """acf_hip_cut_crops into a sentinel-filled buffer of n + slack slots -> (raw bits [n][...], the bytes behind them)"""
    import torch
    n = len(frames)
    cb = HipDetector.crop_bytes(spec, src.channels)
    out = torch.full(((n + slack) * cb,), SENTINEL, dtype=torch.uint8, device="cuda")
    b, f = dev(boxes), dev(frames)
    torch.cuda.synchronize()                                                                 # (torch fills on its own stream)
    det._chk(det.lib.acf_hip_cut_crops(det.ctx, C.byref(src), C.c_void_p(b.data_ptr()), C.c_void_p(f.data_ptr()), n, C.byref(spec), C.c_void_p(out.data_ptr())))
    det.synchronize()
    raw = out.cpu().numpy()
    shape = (spec.out_h, spec.out_w, src.channels) if spec.layout == 1 else (src.channels, spec.out_h, spec.out_w)
    return raw[:n * cb].view(NP_ELEM[int(spec.dtype)]).reshape((n,) + shape), raw[n * cb:]


def check(det, s, x, code, spec, tag):
    """every box of the shared list for this source, turn and spec: bits, sentinel, and the forms the boxes take"""
    U = s.upright(code)
    Hu, Wu = U.shape[1:3]
    boxes, frames, what = ccr.boxes_for(Hu, Wu, NF, spec, s.C, s.sb)
    src = s.crop_source(det, x, code)
    got, tail = cut(det, src, boxes, frames, spec)
    want = ccr.crops(U, boxes, frames, spec.out_h, spec.out_w, spec.samples, s.unit, int(spec.dtype), int(spec.layout))
    assert got.shape == want.shape and got.dtype == want.dtype, (tag, got.shape, want.shape)
    for i, w in enumerate(what):
        assert np.array_equal(got[i], want[i]), (tag, w, boxes[i].tolist(), int(frames[i]), int((got[i] != want[i]).sum()))
    assert (tail == SENTINEL).all(), tag
    for w in ("NaN member", "infinite width", "zero width", "negative height", "frame -1", "frame n_frames"):
        assert not got[what.index(w)].any(), (tag, w)
    return {HipDetector.crop_form(spec, b, Hu, Wu, s.C, s.sb) for b in boxes if ccr.box_ok(b)}


@pytest.mark.parametrize("name", list(SOURCES), ids=list(SOURCES))
def test_crops_equal_the_definition_bit_for_bit(det, name):
    build, codes = SOURCES[name]
    s = build()
    x = dev(s.buf)
    forms = set()
    for k, code in enumerate(codes):
        # every spec in float32 planar on the first turn (two of them on the others), then every dtype and both layouts on one spec
        for (oh, ow, smp) in (ccr.SPECS if k == 0 else [ccr.SPECS[2], ccr.SPECS[5 if k & 1 else 4]]):
            forms |= check(det, s, x, code, ccr.spec_of(oh, ow, smp), (name, code, oh, ow, smp))
        if k == 0:
            # the narrow types on enough values to meet the rare ones: val * unit is rounded to float32 and THEN narrowed (an f16
            # conversion fused with the product rounds once, and differs on about one value in 10^4)
            check(det, s, x, code, ccr.spec_of(112, 112, 1, capi.T_F16, 1), (name, code, "f16 112 x 112"))
            check(det, s, x, code, ccr.spec_of(64, 64, 2, capi.T_BF16, 0), (name, code, "bf16 64 x 64"))
        if k == 0 or len(codes) == 8:
            for dt in (capi.T_U8, capi.T_F16, capi.T_BF16, capi.T_F32):
                if dt == capi.T_U8 and not s.codes8:
                    continue
                for layout in (0, 1):
                    if (dt, layout) == (capi.T_F32, 0) or (k and (dt + layout + k) % 3):     # (the other turns: a third of the combinations each)
                        continue
                    oh, ow, smp = ccr.SPECS[1] if (dt + layout) & 1 else ccr.SPECS[2]
                    check(det, s, x, code, ccr.spec_of(oh, ow, smp, dt, layout), (name, code, "dtype", dt, "layout", layout))
    assert forms == {0, 1}, (name, forms)                                                    # both forms ran, on this source


def test_u8_output_rounds_to_even():
    """U8 out against rint: a hand-made frame whose half-way samples are exact — 2 x 2 means of (0, 1, 0, 0) .. are k / 4."""
    import torch
    d = HipDetector()
    S = np.zeros((1, 4, 8, 1), dtype=np.uint8)
    S[0, 0::2, 0::2, 0] = [[1, 2, 3, 255], [5, 0, 254, 7]]                                   # 2 x 2 cells sum to 1, 2, 3, 255, 5, 0, 254, 7
    S[0, 1, 1, 0], S[0, 1, 7, 0] = 1, 255                                                    # -> sums 2 and 510
    x = dev(S)
    src = d.crop_source_tensor(x.permute(0, 3, 1, 2))
    out = d.cut_crops(src, np.array([[0, 0, 8, 4]], dtype=F), np.array([0], dtype=np.int32), (2, 4), samples=2, dtype=torch.uint8)
    d.synchronize()
    U = S[0].astype(F)
    want = ccr.crop(U, [0, 0, 8, 4], 2, 4, 2, 1.0, capi.T_U8, 0)
    val = ccr.sample(U, [0, 0, 8, 4], 2, 4, 2)[..., 0]
    assert val.tolist() == [[0.5, 0.5, 0.75, 127.5], [1.25, 0.0, 63.5, 1.75]]                # s = 2 samples a cell at its pixel centres: the cell's mean
    assert want[0].tolist() == [[0, 0, 1, 128], [1, 0, 64, 2]]
    assert np.array_equal(out.cpu().numpy()[0], want)
    d.close()


def test_tensor_sources_and_defaults(det):
    """crop_source_tensor on torch views (NCHW, channels_last memory, an NHWC tensor), the default spec, n = 0."""
    import torch
    E = np.random.RandomState(5).randint(0, 256, (NF, 3, 37, 53)).astype(np.uint8)
    U = np.ascontiguousarray(E.transpose(0, 2, 3, 1)).astype(F)
    boxes = np.array([[3.3, 2.7, 17.6, 12.2], [-4, -3, 70, 50]], dtype=F)
    frames = np.array([1, 0], dtype=np.int32)
    want = ccr.crops(U, boxes, frames, 7, 5, 1, F(1 / 255.0), capi.T_F32, 0)
    t = dev(E)
    for src in (det.crop_source_tensor(t), det.crop_source_tensor(t.contiguous(memory_format=torch.channels_last)),
                det.crop_source_tensor(dev(E.transpose(0, 2, 3, 1)), layout="nhwc")):
        out = det.cut_crops(src, boxes, frames, (7, 5))
        det.synchronize()
        assert out.dtype == torch.float32 and tuple(out.shape) == (2, 3, 7, 5)
        assert np.array_equal(ccr.raw_bits(out.cpu().numpy()), want)
    packed = det.cut_crops(det.crop_source_tensor(t), boxes, frames, (7, 5), layout="packed", dtype=torch.bfloat16)
    det.synchronize()
    assert tuple(packed.shape) == (2, 7, 5, 3)
    assert np.array_equal(packed.view(torch.int16).cpu().numpy().view(np.uint16), ccr.crops(U, boxes, frames, 7, 5, 1, F(1 / 255.0), capi.T_BF16, 1))
    # n = 0 is accepted and writes nothing
    src = det.crop_source_tensor(t)
    got, tail = cut(det, src, np.zeros((0, 4), F), np.zeros((0,), np.int32), ccr.spec_of(7, 5, 1))
    assert got.shape[0] == 0 and (tail == SENTINEL).all()


def test_profile_names_the_kernel(det):
    s = SOURCES["nv12_even"][0]()
    x = dev(s.buf)
    det.set_option("profile", 1)
    det.profile()
    check(det, s, x, 1, ccr.spec_of(7, 5, 1), "profile")
    names = det.profile()
    det.set_option("profile", 0)
    assert [n for n in names if n != "(end)"] == ["k_cut_crops"], names


# ---------------------------------------------------------------- cut_detections

DH, DW, DSCALE, K = 112, 144, 0.5, 3
CASC_THR = {1: -1.2, 6: -1.4}    # chosen on the CPU oracle: by frame (busy, patch, flat) > K, 1 .. K and no detections, NMS off and on
NMS = dict(type="maxg", overlap=0.65, ovrDnm="min")


def _det_frames():
    out = []
    for kind in ("busy", "patch", "flat"):
        Y, U, V = rc.yuv_planes(77, DH, DW, 1, 1)
        if kind != "busy":
            Y2, U2, V2 = Y.copy(), U.copy(), V.copy()
            Y[:], U[:], V[:] = 100, 128, 128
            if kind == "patch":
                Y[30:70, 40:90], U[15:35, 20:45], V[15:35, 20:45] = Y2[30:70, 40:90], U2[15:35, 20:45], V2[15:35, 20:45]
        out.append((Y, U, V))
    return out


@pytest.mark.parametrize("code", [1, 6])
def test_cut_detections_equals_get_detections_crop_box_reference(code):
    import torch
    planes = _det_frames()
    buf = np.stack([ydr.pack("i420", *p) for p in planes])
    desc, fb = HipDetector.yuv_desc("i420", DH, DW)
    assert buf.shape == (3, fb)
    U = np.ascontiguousarray(orf.orient(np.stack([ydr.planes_to_rgb(Y, Uc, V, 1, 1) for Y, Uc, V in planes]), code, axes=(1, 2))).astype(F)
    h, w = HipDetector.oriented_resized_dims(DH, DW, code, DSCALE)
    det = HipDetector(synth.make_model(seed=3, name="TINY", nTrees=16, cascThr=CASC_THR[code]), h, w, 3, max_batch=3, max_hits=1 << 12)
    x = dev(buf)
    src = det.crop_source_yuv(x, 3, desc, None, DH, DW, code)
    oh, ow, grow = 24, 20, 1.3
    for nms in (None, capi.make_nms(**NMS)):
        det.set_nms(nms)
        det.run_yuv_resized(x, 3, desc, DH, DW, DSCALE, code)
        first = [det.detections(f)[0] for f in range(3)]
        lens = sorted(len(d) for d in first)
        assert lens[0] == 0 and 1 <= lens[1] <= K and lens[2] > K, (code, nms is not None, lens)
        for dt, layout, smp in ((torch.float16, "planar", 2), (torch.uint8, "packed", 1)):
            spec = HipDetector.crop_spec((oh, ow), smp, dt, layout, K, grow)
            cb = HipDetector.crop_bytes(spec, 3)
            out = torch.full((3 * K * cb,), SENTINEL, dtype=torch.uint8, device="cuda")
            boxes = torch.full((3, K, 4), -777.0, dtype=torch.float32, device="cuda")
            counts = torch.full((3,), -99, dtype=torch.int32, device="cuda")
            torch.cuda.synchronize()
            det.run_yuv_resized(x, 3, desc, DH, DW, DSCALE, code)
            got = det.cut_detections(src, (oh, ow), K, det_scale=DSCALE, grow=grow, samples=smp, dtype=dt, layout=layout, out=out, boxes_out=boxes,
                                     counts_out=counts)
            assert got[0] is out and got[1] is boxes and got[2] is counts
            det.run_yuv_resized(x, 3, desc, DH, DW, DSCALE, code)                          # queued behind it: the call did not wait
            det.synchronize()
            again = [det.detections(f)[0] for f in range(3)]
            raw, bx, cnt = out.cpu().numpy().reshape(3, K, cb), boxes.cpu().numpy(), counts.cpu().numpy()
            for f in range(3):
                assert again[f].tobytes() == first[f].tobytes(), (code, f)
                n = min(len(first[f]), K)
                assert cnt[f] == n, (code, f, cnt)
                for i in range(K):
                    if i >= n:
                        assert (raw[f, i] == SENTINEL).all() and (bx[f, i] == -777.0).all(), (code, f, i)    # not written
                        continue
                    d = first[f][i]
                    box = ccr.crop_box([d["x"], d["y"], d["w"], d["h"]], DSCALE, grow)
                    assert np.array_equal(box.view(np.uint32), HipDetector.crop_box([d["x"], d["y"], d["w"], d["h"]], DSCALE, grow).view(np.uint32))
                    assert np.array_equal(bx[f, i].view(np.uint32), box.view(np.uint32)), (code, f, i, bx[f, i], box)
                    code_dt = capi.T_F16 if dt == torch.float16 else capi.T_U8
                    want = ccr.crop(U[f], box, oh, ow, smp, F(1 / 255.0), code_dt, 1 if layout == "packed" else 0)
                    assert np.array_equal(raw[f, i].view(want.dtype).reshape(want.shape), want), (code, nms is not None, f, i, box.tolist())
    det.close()


def test_cut_detections_without_a_resize_and_with_defaults():
    """det_scale None: the plan is for the upright size; outputs allocated by the call."""
    import torch
    code = 6
    planes = _det_frames()[:1]
    buf = np.stack([ydr.pack("nv12", *p) for p in planes])
    desc, fb = HipDetector.yuv_desc("nv12", DH, DW)
    U = np.ascontiguousarray(orf.orient(np.stack([ydr.planes_to_rgb(Y, Uc, V, 1, 1) for Y, Uc, V in planes]), code, axes=(1, 2))).astype(F)
    h, w = HipDetector.oriented_dims(DH, DW, code)
    det = HipDetector(synth.make_model(seed=3, name="TINY", nTrees=16, cascThr=-1.0), h, w, 3, max_batch=1, max_hits=1 << 12)
    x = dev(buf)
    det.run_yuv(x, 1, desc, code, DH, DW)
    crops, boxes, counts = det.cut_detections(det.crop_source_yuv(x, 1, desc, None, DH, DW, code), 16, 4)
    det.synchronize()
    d, _ = det.detections(0)
    assert len(d) > 0 and int(counts[0]) == min(len(d), 4)
    assert tuple(crops.shape) == (1, 4, 3, 16, 16) and crops.dtype == torch.float32
    for i in range(int(counts[0])):
        box = ccr.crop_box([d["x"][i], d["y"][i], d["w"][i], d["h"][i]], 0, 1.0)
        assert np.array_equal(boxes[0, i].cpu().numpy(), box)
        assert np.array_equal(ccr.raw_bits(crops[0, i].cpu().numpy()), ccr.crop(U[0], box, 16, 16, 1, F(1 / 255.0), capi.T_F32, 0))
    det.close()


# ---------------------------------------------------------------- refusals

def test_refusals_each_with_its_code_and_text():
    import torch
    H, W, code, scale = 48, 64, 1, 0.5
    h, w = HipDetector.oriented_resized_dims(H, W, code, scale)
    model = synth.make_model(seed=3, name="TINY", nTrees=16)
    det = HipDetector(model, h, w, 3, max_batch=2)
    lib = det.lib
    x = torch.zeros(2 * H * W * 3 * 4, dtype=torch.uint8, device="cuda")
    ydesc, _ = HipDetector.yuv_desc("i420", H, W)
    idesc = capi.ImageDesc(capi.T_U8, 3, 3 * H * W, H * W, W, 1)
    boxes = dev(np.array([[1, 1, 9, 9]], dtype=F))
    frames = dev(np.array([0], dtype=np.int32))
    out = torch.zeros(1 << 20, dtype=torch.uint8, device="cuda")
    bout = torch.zeros((2, 3, 4), dtype=torch.float32, device="cuda")
    cout = torch.zeros((2,), dtype=torch.int32, device="cuda")
    P = lambda t: C.c_void_p(t.data_ptr())
    ysrc = lambda **kw: _with(det.crop_source_yuv(x, 2, ydesc, None, H, W, code), **kw)
    isrc = lambda **kw: _with(det.crop_source_image(x.data_ptr(), 2, idesc, H, W, code), **kw)
    spec = lambda **kw: _with(HipDetector.crop_spec((7, 5), 1, None, "planar", 3, 1.0), **kw)

    def crops(src, sp, b=boxes, f=frames, n=1, o=out):
        return lib.acf_hip_cut_crops(det.ctx, C.byref(src) if src is not None else None, P(b) if b is not None else None, P(f) if f is not None else None, n,
                                     C.byref(sp) if sp is not None else None, P(o) if o is not None else None)

    def dets(src, sp, sc=scale, o=out, c=cout, ctx=None):
        return lib.acf_hip_cut_detections((ctx or det).ctx, C.byref(src) if src is not None else None, C.c_double(sc), C.byref(sp) if sp is not None else None,
                                          P(o) if o is not None else None, P(bout), P(c) if c is not None else None)

    def refused(rc, want=capi.E_INVALID, ctx=None):
        assert rc == want, (rc, want)
        assert len(lib.acf_hip_last_error((ctx or det).ctx) or b"") > 10

    def accepted():
        assert crops(ysrc(), spec()) == 0 and crops(isrc(), spec()) == 0
        det.synchronize()

    accepted()
    # null pointers
    assert lib.acf_hip_cut_crops(None, C.byref(ysrc()), P(boxes), P(frames), 1, C.byref(spec()), P(out)) == capi.E_INVALID
    for rc in (crops(None, spec()), crops(ysrc(), None), crops(ysrc(), spec(), b=None), crops(ysrc(), spec(), f=None), crops(ysrc(), spec(), o=None),
               crops(ysrc(base_dev=None), spec())):
        refused(rc)
    # both or neither of image / yuv
    both = ysrc()
    both.image = C.pointer(idesc)
    neither = ysrc()
    neither.yuv = None
    refused(crops(both, spec()))
    refused(crops(neither, spec()))
    # what the oriented image / video entry refuses about the description and the format
    bad = capi.YuvDesc.from_buffer_copy(ydesc)
    bad.sub_x = 2
    refused(crops(det.crop_source_yuv(x, 2, bad, None, H, W, code), spec()))
    bad = capi.YuvDesc.from_buffer_copy(ydesc)
    bad.u.stride_px = 0
    refused(crops(det.crop_source_yuv(x, 2, bad, None, H, W, code), spec()))
    badi = capi.ImageDesc.from_buffer_copy(idesc)
    badi.channels = 2
    refused(crops(det.crop_source_image(x.data_ptr(), 2, badi, H, W, code), spec()))
    badi = capi.ImageDesc.from_buffer_copy(idesc)
    badi.stride_x = 0
    refused(crops(det.crop_source_image(x.data_ptr(), 2, badi, H, W, code), spec()))
    badi = capi.ImageDesc.from_buffer_copy(idesc)
    badi.dtype = 4
    refused(crops(det.crop_source_image(x.data_ptr(), 2, badi, H, W, code), spec()))
    refused(crops(det.crop_source_yuv(x, 2, ydesc, HipDetector.video_format(7), H, W, code), spec()))
    refused(crops(det.crop_source_yuv(x, 2, ydesc, HipDetector.video_format(8, 2), H, W, code), spec()))
    refused(crops(det.crop_source_yuv(x, 2, ydesc, HipDetector.video_format(10, 0, 3), H, W, code), spec()))
    refused(crops(det.crop_source_yuv(x.data_ptr() + 1, 2, ydesc, HipDetector.video_format(10), H, W, code), spec()))     # 16-bit words at an odd base
    # orient outside 0 .. 7; sizes < 1
    for kw in (dict(orient=8), dict(orient=-1), dict(src_rows=0), dict(src_cols=-3), dict(n_frames=0)):
        refused(crops(ysrc(**kw), spec()))
        refused(crops(isrc(**kw), spec()))
    # the spec out of range
    for kw in (dict(out_h=0), dict(out_w=513), dict(samples=0), dict(samples=5), dict(dtype=-1), dict(dtype=4), dict(layout=2), dict(reserved=1)):
        refused(crops(ysrc(), spec(**kw)))
        refused(dets(ysrc(), spec(**kw)))
    # n < 0
    refused(crops(ysrc(), spec(), n=-1))
    # UNSUPPORTED: uint8 crops from a floating image or from wide video
    fdesc = capi.ImageDesc(capi.T_F32, 3, 3 * H * W, H * W, W, 1)
    refused(crops(det.crop_source_image(x.data_ptr(), 2, fdesc, H, W, code), spec(dtype=capi.T_U8)), capi.E_UNSUPPORTED)
    wdesc, _ = HipDetector.video_desc("i420", H, W, HipDetector.video_format(10))
    refused(crops(det.crop_source_yuv(x, 2, wdesc, HipDetector.video_format(10), H, W, code), spec(dtype=capi.T_U8)), capi.E_UNSUPPORTED)
    assert crops(det.crop_source_yuv(x, 2, wdesc, HipDetector.video_format(10), H, W, code), spec(dtype=capi.T_F16)) == 0
    # cut_detections: without valid detections
    refused(dets(ysrc(), spec()))
    bare = HipDetector()
    refused(lib.acf_hip_cut_detections(bare.ctx, C.byref(ysrc()), C.c_double(scale), C.byref(spec()), P(out), P(bout), P(cout)), ctx=bare)
    assert lib.acf_hip_cut_crops(bare.ctx, C.byref(ysrc()), P(boxes), P(frames), 1, C.byref(spec()), P(out)) == 0        # no model, no plan needed
    bare.synchronize()
    bare.close()
    det.run_yuv_resized(x, 2, ydesc, H, W, scale, code)
    assert dets(ysrc(), spec()) == 0
    # K and grow out of range; null counts
    for kw in (dict(max_per_frame=0), dict(max_per_frame=2049), dict(grow=0.0), dict(grow=-1.0), dict(grow=float("nan")), dict(grow=float("inf"))):
        refused(dets(ysrc(), spec(**kw)))
        assert crops(ysrc(), spec(**kw)) == 0                                               # (cut_crops does not read them)
    refused(dets(ysrc(), spec(), c=None))
    refused(dets(ysrc(), spec(), o=None))
    # n_frames other than the last batch; a plan of other dimensions; a scale that is no scale
    refused(dets(ysrc(n_frames=1), spec()))
    refused(dets(ysrc(orient=2), spec()))
    refused(dets(ysrc(src_rows=H + 2), spec()))
    refused(dets(ysrc(), spec(), sc=0.75))
    refused(dets(ysrc(), spec(), sc=0.0))
    for s in (-0.5, float("nan"), float("inf")):
        refused(dets(ysrc(), spec(), sc=s))
    # option "streams" > 1
    multi = HipDetector(model, h, w, 3, max_batch=4, streams=2)
    refused(lib.acf_hip_cut_crops(multi.ctx, C.byref(ysrc()), P(boxes), P(frames), 1, C.byref(spec()), P(out)), capi.E_UNSUPPORTED, ctx=multi)
    refused(lib.acf_hip_cut_detections(multi.ctx, C.byref(ysrc()), C.c_double(scale), C.byref(spec()), P(out), P(bout), P(cout)), capi.E_UNSUPPORTED, ctx=multi)
    multi.close()
    # ... and a following valid call still works
    accepted()
    assert dets(ysrc(), spec()) == 0
    det.synchronize()
    with pytest.raises(HipError) as e:
        det.cut_crops(ysrc(), np.zeros((1, 4), F), np.zeros(1, np.int32), (0, 5))
    assert e.value.code == capi.E_INVALID
    det.close()


def _with(obj, **kw):
    for k, v in kw.items():
        setattr(obj, k, v)
    return obj
