"""The video frame entry for three-plane YUV descriptors on the GPU (include/acf_hip.h: acf_hip_pyramid_yuv / run_yuv /
yuv_to_rgb8 / stream_open_yuv).

The expected result of a YUV frame is what the packed RGB entry, run_u8(PIX_RGB), gives for the R, G, B bytes of the numpy
restatement (tests/yuv_desc_ref.py: a gather through the descriptor, then tests/yuv420_ref.py's per-pixel formula); run_u8 itself is
held against the oracle by tests/test_gpu_ingest.py.  Every comparison is an equality of bytes or of uint32 views.
"""
import ctypes as C
import os
import sys

import numpy as np
import pytest

import yuv420_ref as yr
import yuv_desc_ref as ydr
from acf_amd import capi, synth

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

H, W = 130, 174  # three tiles each way, ragged edges, H % 4 == 2
INRIA = dict(name="INRIA", nTrees=64, cascThr=-3.0, nOctUp=0)


def bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def snapshot(det, nF):
    """Per frame (levels, detections bytes, hits bytes) of the last run."""
    out = []
    for f in range(nF):
        d, h = det.detections(f)
        out.append(([bits(det.read_level(f, i)) for i in range(len(det.levels))], d.tobytes(), h.tobytes()))
    return out


def same(got, want, tag):
    assert len(got) == len(want), tag
    for f, ((gl, gd, gh), (wl, wd, wh)) in enumerate(zip(got, want)):
        for i, (a, b) in enumerate(zip(gl, wl)):
            assert np.array_equal(a, b), (tag, f, "level", i)
        assert gd == wd and gh == wh, (tag, f)


def dev(buf):
    import torch
    return torch.from_numpy(np.ascontiguousarray(buf)).cuda()


def rgb_expect(det, rgb):
    """run_u8(PIX_RGB) on uint8 [n][rows][cols][3] -> snapshot."""
    x = dev(rgb)                                                          # (alive until the snapshot has synchronised)
    det.run_u8(x, capi.PIX_RGB)
    return snapshot(det, rgb.shape[0])


def batch(name, planes, stride=0):
    """The frames of `planes` ([(Y, U, V), ...]) in the named layout back to back -> (flat buffer, descriptor, frame bytes)."""
    from acf_amd.detector import HipDetector
    rows, cols = planes[0][0].shape
    d, fb = HipDetector.yuv_desc(name, rows, cols, stride)
    buf = np.concatenate([ydr.pack(name, Y, U, V, stride) for Y, U, V in planes])
    assert buf.size == fb * len(planes)
    return buf, d, fb


@pytest.fixture(scope="module")
def det130():
    from acf_amd.detector import HipDetector
    det = HipDetector(synth.make_model(seed=3, **INRIA), H, W, 3, max_batch=2, max_hits=1 << 16)
    yield det
    det.close()


_REF = {}


def reference(det, sx, sy):
    """Two random frames of the subsampling class (every code value), their RGB by numpy and the RGB entry's result: computed once."""
    if (sx, sy) not in _REF:
        name = {(1, 1): "i420", (1, 0): "i422", (0, 0): "i444"}[(sx, sy)]
        planes = [ydr.random_planes(70 + 10 * sx + sy + 100 * f, name, H, W) for f in range(2)]
        rgb = np.stack([ydr.planes_to_rgb(Y, U, V, sx, sy) for Y, U, V in planes])
        want = rgb_expect(det, rgb)
        assert sum(len(w[1]) for w in want) > 0, "no detections: the cascade comparison would be vacuous"
        _REF[(sx, sy)] = (planes, rgb, want)
    return _REF[(sx, sy)]


# ---------------------------------------------------------------- the conversion alone, every (Y, U, V)

def test_yuv_to_rgb8_on_every_triple():
    """A 4096 x 4096 I444 frame whose pixels enumerate every (Y, U, V) exactly once; neither model nor plan."""
    from acf_amd.detector import HipDetector
    det = HipDetector()
    idx = np.arange(1 << 24, dtype=np.int32).reshape(4096, 4096)
    Y, U, V = (idx >> 16).astype(np.uint8), ((idx >> 8) & 255).astype(np.uint8), (idx & 255).astype(np.uint8)
    d, fb = HipDetector.yuv_desc("i444", 4096, 4096)
    got = det.yuv_to_rgb8(dev(np.concatenate([Y.ravel(), U.ravel(), V.ravel()])), 1, 4096, 4096, d).cpu().numpy()
    assert np.array_equal(got[0], yr.yuv_to_rgb(Y, U, V))
    det.close()


# ---------------------------------------------------------------- the nine named layouts

@pytest.mark.parametrize("padded", [False, True], ids=["tight", "padded"])
@pytest.mark.parametrize("name", ydr.NAMES)
def test_named_layouts_equal_the_rgb_entry(det130, name, padded):
    det = det130
    sx, sy = ydr.SUB[name]
    planes, rgb, want = reference(det, sx, sy)
    # rows padded to a 4-aligned stride whose chroma stride is 4-aligned too
    stride = 0 if not padded else (352 if name in ydr.PACKED_ORDER else 192 if name not in ("nv12", "nv21") else 176)
    buf, d, fb = batch(name, planes, stride)
    assert np.array_equal(ydr.desc_to_rgb(buf, d, H, W, 2), rgb)          # the helper's gather sees the planes that went in
    x = dev(buf)
    assert np.array_equal(det.yuv_to_rgb8(x, 2, H, W, d).cpu().numpy(), rgb), name
    det.run_yuv(x, 2, d)
    got = snapshot(det, 2)
    same(got, want, name)
    if name in ("nv12", "nv21"):
        det.run_u8(x, capi.PIX_NV21 if name == "nv21" else capi.PIX_NV12, stride, n=2)
        same(snapshot(det, 2), got, name + " against run_u8")


# ---------------------------------------------------------------- odd sizes: ceil-sized chroma planes, the scalar rgb2luv body

@pytest.mark.parametrize("layout,ystride,cstride", [("planar", 175, 88), ("planar", 176, 88), ("yuyv", 352, 0)],
                         ids=["byte_loads", "dword_loads_with_tails", "yuyv_half_macropixel"])
def test_odd_sizes_reach_the_scalar_luv_body(layout, ystride, cstride):
    """131 x 175 (h * w % 4 == 1: IG_LUV) as hand-built 4:2:0 planar with 66 x 88 chroma planes, and as hand-packed YUYV (131 x 88 chroma
    samples: every row ends on half a macropixel)."""
    import oriented_case as oc
    from acf_amd.detector import HipDetector
    h, w, nF = 131, 175, 2
    ch, cw = (66, 88) if layout == "planar" else (131, 88)
    sy = 1 if layout == "planar" else 0
    det = HipDetector(synth.make_model(seed=3, name="INRIA", nTrees=64, cascThr=-2.5, nOctUp=0), h, w, 3, max_batch=nF, max_hits=1 << 16)
    rng = np.random.RandomState(9)
    planes = [(rng.randint(0, 256, (h, w)), rng.randint(0, 256, (ch, cw)), rng.randint(0, 256, (ch, cw))) for f in range(nF)]
    rgb = np.stack([ydr.planes_to_rgb(Y, U, V, 1, sy) for Y, U, V in planes])
    if layout == "planar":
        buf, d, fb = oc.planar_buffer(planes, ystride, cstride, (1, 1))
    else:
        buf, d, fb = oc.yuyv_buffer(planes, ystride)
    assert np.array_equal(ydr.desc_to_rgb(buf, d, h, w, nF), rgb)
    want = rgb_expect(det, rgb)
    assert sum(len(x[1]) for x in want) > 0
    x = dev(buf)
    assert np.array_equal(det.yuv_to_rgb8(x, nF, h, w, d).cpu().numpy(), rgb)
    det.set_option("profile", 1)
    det.profile()
    det.run_yuv(x, nF, d)
    names = set(det.profile())
    assert ("k_ingest_yuv_packed422" if layout == "yuyv" else "k_ingest_yuv_generic" if ystride % 4 else "k_ingest_yuv_planar") in names, names
    same(snapshot(det, nF), want, (layout, ystride, cstride))
    det.close()


# ---------------------------------------------------------------- the load forms give identical bits

def _planar_buffer(planes, ystride, cstride, lead):
    """Hand-packed I420 frames with any strides, `lead` bytes in front -> (buffer, descriptor relative to buf[lead])."""
    h, w = planes[0][0].shape
    ch, cw = planes[0][1].shape
    fb = ystride * h + 2 * cstride * ch
    buf = np.full(lead + fb * len(planes), 0x5A, np.uint8)
    for f, (Y, U, V) in enumerate(planes):
        fr = buf[lead + f * fb:lead + (f + 1) * fb]
        fr[:ystride * h].reshape(h, ystride)[:, :w] = Y
        fr[ystride * h:ystride * h + cstride * ch].reshape(ch, cstride)[:, :cw] = U
        fr[ystride * h + cstride * ch:].reshape(ch, cstride)[:, :cw] = V
    d = capi.YuvDesc(capi.YuvPlane(0, fb, ystride, 1), capi.YuvPlane(ystride * h, fb, cstride, 1), capi.YuvPlane(ystride * h + cstride * ch, fb, cstride, 1), 1, 1)
    return buf, d


def test_load_forms_give_identical_pyramids_and_report_their_names(det130):
    det = det130
    i420, _, want420 = reference(det, 1, 1)
    p422, _, want422 = reference(det, 1, 0)
    det.set_option("profile", 1)
    try:
        def run(x, off, d):
            det.profile()
            det.run_yuv(x.data_ptr() + off, 2, d)
            return snapshot(det, 2), set(det.profile())
        # I420: aligned (strides 176 / 88), then one byte further with an odd row stride
        buf, d = _planar_buffer(i420, 176, 88, 0)
        a, names = run(dev(buf), 0, d)
        assert "k_ingest_yuv_planar" in names and "k_ingest_yuv_generic" not in names, names
        buf, d = _planar_buffer(i420, 175, 89, 1)
        b, names = run(dev(buf), 1, d)
        assert "k_ingest_yuv_generic" in names and "k_ingest_yuv_planar" not in names, names
        same(a, want420, "i420 planar form")
        same(b, a, "i420 generic against planar")
        # YUYV: aligned, then the same bytes from a base shifted by one byte
        buf, d, fb = batch("yuyv", p422)
        a, names = run(dev(buf), 0, d)
        assert "k_ingest_yuv_packed422" in names and "k_ingest_yuv_generic" not in names, names
        b, names = run(dev(np.concatenate([np.zeros(1, np.uint8), buf])), 1, d)
        assert "k_ingest_yuv_generic" in names and "k_ingest_yuv_packed422" not in names, names
        same(a, want422, "yuyv packed form")
        same(b, a, "yuyv generic against packed")
    finally:
        det.set_option("profile", 0)


# ---------------------------------------------------------------- three separately allocated planes

def test_three_separate_allocations_one_below_the_base(det130):
    import torch
    det = det130
    planes, _, want = reference(det, 1, 1)
    Y, U, V = (np.stack([p[i] for p in planes]) for i in range(3))       # [2][rows][cols] each
    v, y, u = dev(V), dev(Y), dev(U)
    if min(u.data_ptr(), v.data_ptr()) > y.data_ptr():
        # the allocator put both chroma planes above Y: one arena in V, Y, U order
        arena = torch.empty(V.size + Y.size + U.size + 64, dtype=torch.uint8, device="cuda")
        v = arena[:V.size].view(V.shape)
        y = arena[V.size:V.size + Y.size].view(Y.shape)
        u = arena[V.size + Y.size:V.size + Y.size + U.size].view(U.shape)
        v.copy_(dev(V)), y.copy_(dev(Y)), u.copy_(dev(U))
        torch.cuda.synchronize()
    base, n, d = det.yuv_planes_desc(y, u, v, 1, 1)
    assert n == 2 and min(d.u.offset, d.v.offset) < 0, "a plane below the base: a negative offset"
    lo, hi = det.yuv_extent(d, H, W, 2)
    assert lo == [0, d.u.offset, d.v.offset] and hi[0] == Y.size - 1 and hi[1] == d.u.offset + U.size - 1
    det.run_yuv_planes(y, u, v, 1, 1)
    same(snapshot(det, 2), want, "separate allocations")


# ---------------------------------------------------------------- views: a repeated frame, a view that ends with its allocation

def test_views_repeat_a_frame_and_end_with_the_allocation(det130):
    import torch
    det = det130
    planes, _, want = reference(det, 1, 1)
    buf, d, fb = batch("i420", planes[:1])
    for p in (d.y, d.u, d.v):
        p.stride_n = 0
    x = dev(buf)
    det.run_yuv(x, 2, d)
    same(snapshot(det, 2), [want[0], want[0]], "stride_n = 0")
    # both frames at the end of a larger surface: the last addressed byte is the allocation's last byte
    buf, d, fb = batch("i420", planes)
    lead = 4096 + 3
    x = torch.empty(lead + buf.size, dtype=torch.uint8, device="cuda")
    x[lead:].copy_(dev(buf))
    torch.cuda.synchronize()
    lo, hi = det.yuv_extent(d, H, W, 2)
    assert min(lo) == 0 and lead + max(hi) == x.numel() - 1
    det.run_yuv(x.data_ptr() + lead, 2, d)
    same(snapshot(det, 2), want, "view at the end of its allocation")


# ---------------------------------------------------------------- the other conversions of the store phase

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
    for name in ("i420", "uyvy"):
        sx, sy = ydr.SUB[name]
        # video-like frames, so that the cascade has something to find
        planes = []
        for f in range(2):
            up = np.clip(np.rint(synth.make_frame(40 + f, h, w, "rgb").transpose(2, 1, 0) * 255.0), 0, 255).astype(np.uint8)
            Y, U, V = yr.planes(yr.from_rgb(up), h, w)
            planes.append((Y.copy(), np.repeat(U, 2, axis=0).copy() if sy == 0 else U.copy(), np.repeat(V, 2, axis=0).copy() if sy == 0 else V.copy()))
        rgb = np.stack([ydr.planes_to_rgb(Y, U, V, sx, sy) for Y, U, V in planes])
        want = rgb_expect(det, rgb)
        buf, d, fb = batch(name, planes)
        x = dev(buf)
        det.set_option("profile", 1)
        det.profile()
        det.run_yuv(x, 2, d)
        names = set(det.profile())
        det.set_option("profile", 0)
        # tight rows of w samples: the planar form needs w and w / 2 four-aligned, else the element-wise form; uyvy rows of 2 w bytes are
        assert ("k_ingest_yuv_packed422" if name == "uyvy" else "k_ingest_yuv_planar" if w % 8 == 0 else "k_ingest_yuv_generic") in names, (tag, name, names)
        same(snapshot(det, 2), want, (tag, name))
        total += sum(len(x[1]) for x in want)
    assert total > 0, "no detections: the cascade comparison would be vacuous"
    det.close()


# ---------------------------------------------------------------- streaming

def test_stream_of_i420_frames_matches_blocking_calls():
    """Four I420 batches (one short) from pinned memory at depth 2 give the records of run_yuv + export of each batch."""
    import torch
    from acf_amd.detector import HipDetector, PinnedBuffer
    h, w, cap, nB, depth = 120, 160, 512, 3, 2
    det = HipDetector(synth.make_model(seed=3, **INRIA), h, w, 3, max_batch=nB, max_hits=4096)
    d, fb = HipDetector.yuv_desc("i420", h, w)
    batches = []
    for b in range(4):
        n = nB if b != 2 else 1
        fr = []
        for i in range(n):
            up = np.clip(np.rint(synth.make_frame(100 + 10 * b + i, h, w, "rgb").transpose(2, 1, 0) * 255.0), 0, 255).astype(np.uint8)
            fr.append(ydr.pack("i420", *yr.planes(yr.from_rgb(up), h, w)))
        batches.append(np.stack(fr))
        assert batches[-1].shape[1] == fb
    want = []
    for x in batches:
        xd = dev(x)                                                       # (alive until the synchronise: the call is asynchronous)
        det.run_yuv(xd, x.shape[0], d)
        dst = torch.zeros((x.shape[0], 1 + 6 * cap), dtype=torch.int32, device="cuda")
        torch.cuda.synchronize()                                          # (torch fills dst on its own stream: before the export writes it)
        det.export_detections(dst, cap)
        det.synchronize()
        want.append(dst.cpu().numpy())
    assert sum(int(x[:, 0].sum()) for x in want) > 0
    pins = [PinnedBuffer(nB * fb) for _ in range(depth)]
    det.stream_open_yuv(d, fb, cap, depth)
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
    # a later acf_hip_stream_open replaces it: packed RGB batches of the same context
    det.stream_open(capi.PIX_RGB, 0, cap, depth)
    rgb = ydr.desc_to_rgb(batches[0].ravel(), d, h, w, nB)
    pin = PinnedBuffer(rgb.size)
    pin.array[:] = rgb.ravel()
    rec = det.stream_collect(det.stream_submit(pin.ptr.value, nB))
    for f in range(nB):
        n = want[0][f, 0]
        assert np.array_equal(rec[f, :1 + 6 * n], want[0][f, :1 + 6 * n]), f
    det.stream_close()
    det.close()
    for p in pins + [pin]:
        p.close()


# ---------------------------------------------------------------- what is refused

def test_yuv_entry_argument_checks():
    import torch
    from acf_amd.detector import HipDetector, HipError
    model = synth.make_model(seed=3, name="TINY", nTrees=16)
    h, w = 96, 128
    x = torch.zeros(4 * h * w * 3, dtype=torch.uint8).cuda()             # room for every call below, were it not refused
    good, fb = HipDetector.yuv_desc("i420", h, w)

    def refused(fn, code=capi.E_INVALID):
        with pytest.raises(HipError) as e:
            fn()
        assert e.value.code == code, e.value

    def variant(**kw):
        d = capi.YuvDesc.from_buffer_copy(good)
        for k, v in kw.items():
            plane, _, field = k.partition("_")
            if plane in ("y", "u", "v"):
                setattr(getattr(d, plane), field, v)
            else:
                setattr(d, k, v)
        return d
    det = HipDetector(model, h, w, 3, max_batch=2)
    det.run_yuv(x, 2, good)                                               # accepted as it is
    lib = det.lib
    assert lib.acf_hip_run_yuv(det.ctx, None, 1, C.byref(good)) == capi.E_INVALID
    assert lib.acf_hip_run_yuv(det.ctx, C.c_void_p(x.data_ptr()), 1, None) == capi.E_INVALID
    assert lib.acf_hip_pyramid_yuv(None, C.c_void_p(x.data_ptr()), 1, C.byref(good)) == capi.E_INVALID
    refused(lambda: det.run_yuv(x, 0, good))
    refused(lambda: det.run_yuv(x, 3, good))                              # max_batch is 2
    for bad in (variant(sub_x=2), variant(sub_y=-1), variant(y_stride_px=0), variant(u_stride_row=0), variant(v_stride_n=-4), variant(u_stride_px=-1)):
        refused(lambda: det.run_yuv(x, 1, bad))
        refused(lambda: det.pyramid_yuv(x, 1, bad))
        refused(lambda: det.yuv_to_rgb8(x, 1, h, w, bad))
        refused(lambda: det.stream_open_yuv(bad, fb, 64, 2))
    # the conversion alone: null destination, empty sizes
    assert lib.acf_hip_yuv_to_rgb8(det.ctx, C.c_void_p(x.data_ptr()), 1, h, w, C.byref(good), None) == capi.E_INVALID
    refused(lambda: det.yuv_to_rgb8(x, 1, 0, w, good))
    refused(lambda: det.yuv_to_rgb8(x, 0, h, w, good))
    # the stream: planes outside [0, frame_bytes), stride_n other than frame_bytes, depth, cap
    refused(lambda: det.stream_open_yuv(good, fb - 1, 64, 2))
    refused(lambda: det.stream_open_yuv(variant(v_offset=-8), fb, 64, 2))
    refused(lambda: det.stream_open_yuv(variant(y_stride_n=fb + 4), fb, 64, 2))
    refused(lambda: det.stream_open_yuv(good, fb, 64, 1))
    refused(lambda: det.stream_open_yuv(good, fb, 0, 2))
    # an active input resize
    small = HipDetector(model, *HipDetector.resize_dims(192, 256, 0.5), 3, max_batch=1)
    small.set_input_resize(192, 256, 0.5)
    refused(lambda: small.run_yuv(x, 1, good))
    refused(lambda: small.stream_open_yuv(good, fb, 64, 2))
    small.close()
    # plans of one and of five input planes
    g = HipDetector(synth.make_model(seed=3, name="FACE64", nTrees=16), h, w, 1, max_batch=1)
    refused(lambda: g.run_yuv(x, 1, good))
    refused(lambda: g.stream_open_yuv(good, fb, 64, 2))
    g.close()
    five = HipDetector(model, h, w, 5, max_batch=1)
    refused(lambda: five.run_yuv(x, 1, good))
    five.close()
    # no plan; sub-batch contexts
    bare = HipDetector(model)
    refused(lambda: bare.run_yuv(x, 1, good), capi.E_NOPLAN)
    bare.close()
    multi = HipDetector(model, h, w, 3, max_batch=4, streams=2)
    refused(lambda: multi.run_yuv(x, 2, good), capi.E_UNSUPPORTED)
    refused(lambda: multi.stream_open_yuv(good, fb, 64, 2), capi.E_UNSUPPORTED)
    multi.close()
    # the ACF_HIP_PIX_* enum is untouched: 7 and 9 are still no layouts of the 8-bit entry
    refused(lambda: det.run_u8(x, 7, n=1))
    refused(lambda: det.run_u8(x, 9, n=1))
    det.run_u8(x, capi.PIX_NV12, n=1)
    det.close()


# ---------------------------------------------------------------- the C++ host

@pytest.mark.parametrize("name,mode", [("i420", []), ("yuyv", ["--stream", "2"])], ids=["i420_batch", "yuyv_stream"])
def test_cli_yuv_matches_the_python_path(tmp_path, name, mode):
    """acf::HipDetector::detectYuv and streamOpenYuv / streamSubmit through the CLI print what run_yuv returns."""
    import subprocess
    from acf_amd.detector import HipDetector
    from acf_amd.modelio import write_model
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    from test_host_cpp import parse, run
    host = os.path.join(ROOT, "acf_amd", "host")
    subprocess.check_call(["make", "-s", "-C", host])
    h, w, cnt = 120, 160, 5
    sx, sy = ydr.SUB[name]
    model = synth.make_model(seed=3, **INRIA)
    write_model(str(tmp_path / "m.acfm"), model)
    planes = []
    for i in range(cnt):
        up = np.clip(np.rint(synth.make_frame(60 + i, h, w, "rgb").transpose(2, 1, 0) * 255.0), 0, 255).astype(np.uint8)
        Y, U, V = yr.planes(yr.from_rgb(up), h, w)
        planes.append((Y.copy(), np.repeat(U, 2, axis=0).copy() if sy == 0 else U.copy(), np.repeat(V, 2, axis=0).copy() if sy == 0 else V.copy()))
    buf, d, fb = batch(name, planes)
    (tmp_path / "f.yuv").write_bytes(buf.tobytes())
    p = run(os.path.join(host, "acf_hip_detect"), ["--model", str(tmp_path / "m.acfm"), "--frames", str(tmp_path / "f.yuv"), "--yuv", name,
                                                   "--rows", str(h), "--cols", str(w), "--count", str(cnt)] + mode)
    got = parse(p.stdout)
    det = HipDetector(model, h, w, 3, max_batch=cnt, max_hits=1 << 16)
    x = dev(buf)
    det.run_yuv(x, cnt, d)
    total = 0
    for f in range(cnt):
        dd, _ = det.detections(f)
        py = [(int(r["x"]), int(r["y"]), int(r["w"]), int(r["h"]), int(np.float32(r["score"]).view(np.uint32))) for r in dd]
        assert got[f] == py, f
        total += len(py)
    assert total > 0
    det.close()
