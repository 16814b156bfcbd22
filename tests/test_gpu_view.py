"""Affine views of the stored frame on the GPU (include/acf_hip.h: acf_hip_pyramid_view / acf_hip_run_view; kernel k_ingest_view, staged
and gather).  Every comparison is bit for bit: every level (acf_hip_read_level), detection and hit of a view call against
  1. the existing entry on the same buffer, for the identity view (every source kind, orientation codes 0, 1, 3, 6),
  2. acf_hip_run_image on the strided sub-view, for integer translations,
  3. acf_hip_run_image on the float32 image tests/view_ref.py restates from the header's definition, for general views.
tests/test_view.py holds the preconditions: the restatement's own properties, that the general views detect something and that the
cases take both forms.  Sources end with their last addressed element (tests/image_entry_case.lay_out poisons the rest)."""
import ctypes as C

import numpy as np
import pytest

import image_entry_case as iec
import orient_ref as orf
import oriented_case as oc
import resized_entry_case as rc
import video_format_ref as vfr
import view_ref as vr
import yuv_desc_ref as ydr
from acf_amd import capi, synth
from acf_amd.detector import HipDetector, HipError

pytestmark = pytest.mark.gpu
F = np.float32
TINY = dict(seed=3, name="TINY", nTrees=96, cascThr=-3.0)
TINY_RGB = dict(TINY, isLuv=0)
P010 = (10, 6, capi.YUV_MATRIX_BT709, 0)
P10LE = (10, 0, capi.YUV_MATRIX_BT2020, 0)


def bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def dev(buf):
    import torch
    return torch.from_numpy(np.ascontiguousarray(buf)).cuda()


def snapshot(det, n):
    """[(levels' bits, detections' bytes, hits' bytes)] of the last batch"""
    det.synchronize()
    out = []
    for f in range(n):
        d, h = det.detections(f)
        out.append(([bits(det.read_level(f, i)) for i in range(len(det.levels))], d.tobytes(), h.tobytes(), len(h)))
    return out


def assert_same(got, want, tag):
    assert len(got) == len(want), tag
    for f, (g, w) in enumerate(zip(got, want)):
        for i, (a, b) in enumerate(zip(g[0], w[0])):
            assert np.array_equal(a, b), (tag, "frame", f, "level", i, int((a != b).sum()))
        assert g[3] == w[3], (tag, "frame", f, "hits", g[3], w[3])
        assert g[1] == w[1] and g[2] == w[2], (tag, "frame", f)
    return sum(w[3] for w in want)


def identity(n):
    return np.tile(vr.IDENTITY, (n, 1))


def f32_desc(h, w, ch=3):
    return capi.ImageDesc(capi.T_F32, ch, ch * h * w, h * w, w, 1)


def run_f32_image(det, img):
    """acf_hip_run_image on a tight planar float32 image [n][C][h][w]"""
    x = dev(img)
    n, ch, h, w = img.shape
    det.run_image(x.data_ptr(), n, f32_desc(h, w, ch))
    det.synchronize()
    return x


# ---------------------------------------------------------------- 1. the identity view is the existing entry

IMAGE_IDENTITY = [("u8_nhwc_luv_vec_ragged", 0), ("u8_nhwc_luv_vec_ragged", 1), ("u8_nhwc_luv_vec_ragged", 6), ("f16_stride2_gray_ragged", 0), ("bf16_nchw_isluv_ragged", 0)]


@pytest.mark.parametrize("name,code", IMAGE_IDENTITY, ids=["%s-%d" % c for c in IMAGE_IDENTITY])
def test_identity_view_equals_the_image_entry(name, code):
    b = iec.build(name)
    c, n = b["case"], iec.N_FRAMES
    Hu, Wu = HipDetector.oriented_dims(c["H"], c["W"], code)
    det = HipDetector(b["model"], Hu, Wu, c["d_in"], max_batch=n, max_hits=1 << 16)
    t = iec.to_device(b["buf"], c["dtype"])
    ptr = t.data_ptr() + c["base"] * t.element_size()
    det.run_image_oriented(ptr, n, b["desc"], c["H"], c["W"], code) if code else det.run_image(ptr, n, b["desc"])
    want = snapshot(det, n)
    src = det.crop_source_image(ptr, n, b["desc"], c["H"], c["W"], code)
    det.run_view(src, identity(n))
    assert assert_same(snapshot(det, n), want, (name, code)) > 0
    det.close()


def video_like(layout, size, fmt, seed, n=2):
    """(flat uint8 buffer, descriptor, capi format or None) of n video-like frames (tests/resized_entry_case.yuv_planes) of a named
    layout; sizes with an odd member through a hand-built descriptor of ceil-sized chroma planes."""
    Hs, Ws = size
    sx, sy = ydr.SUB[layout]
    planes = [rc.yuv_planes(seed + i, Hs, Ws, sx, sy) for i in range(n)]
    if fmt is not None:
        up = fmt[0] - 8                                                                       # the 8-bit codes at the wider sample's scale, the low bits filled
        planes = [tuple((np.asarray(p).astype(np.uint16) << up) | (np.asarray(p).astype(np.uint16) >> (8 - up)) for p in pl) for pl in planes]
        f = HipDetector.video_format(*fmt)
        desc, fb = HipDetector.video_desc(layout, Hs, Ws, f)
        buf = np.concatenate([vfr.pack16(layout, *pl, fmt[1]) for pl in planes])
    elif Hs % 2 or Ws % 2:
        f = None
        buf, desc, fb = oc.planar_buffer(planes, Ws, (Ws + sx) >> sx, (sx, sy))
    else:
        f = None
        desc, fb = HipDetector.yuv_desc(layout, Hs, Ws)
        buf = np.concatenate([ydr.pack(layout, *pl) for pl in planes])
    assert buf.size == n * fb
    _, last = vfr.extent(desc, Hs, Ws, fmt[0] if fmt else 8, n)
    assert max(last) == buf.size - 1                                                          # nothing behind the last addressed byte
    return buf, desc, f


YUV_IDENTITY = [("nv12", (96, 128), None, 0, TINY), ("yuyv", (96, 128), None, 0, TINY_RGB), ("yuyv", (96, 128), None, 1, TINY_RGB), ("yuyv", (96, 128), None, 6, TINY),
                ("i420", (97, 129), None, 0, TINY_RGB), ("nv12", (96, 128), P010, 0, TINY), ("i420", (96, 128), P10LE, 0, TINY_RGB)]


@pytest.mark.parametrize("layout,size,fmt,code,mkw", YUV_IDENTITY, ids=["%s-%dx%d-%s-%d" % (c[0], c[1][0], c[1][1], "8" if c[2] is None else "10", c[3]) for c in YUV_IDENTITY])
def test_identity_view_equals_the_video_entry(layout, size, fmt, code, mkw):
    n = 2
    buf, desc, f = video_like(layout, size, fmt, 60, n)
    Hu, Wu = HipDetector.oriented_dims(size[0], size[1], code)
    det = HipDetector(synth.make_model(**mkw), Hu, Wu, 3, max_batch=n, max_hits=1 << 16)
    x = dev(buf)
    if fmt is not None:
        det.run_video(x, n, desc, f)
    elif code:
        det.run_yuv(x, n, desc, code, size[0], size[1])                                       # acf_hip_run_yuv_oriented
    else:
        det.run_yuv(x, n, desc)
    want = snapshot(det, n)
    det.run_view(det.crop_source_yuv(x, n, desc, f, size[0], size[1], code), identity(n))
    assert assert_same(snapshot(det, n), want, (layout, size, fmt, code)) > 0
    det.close()


def test_wide_video_oriented_through_a_view():
    """16-bit video with orientation 3: acf_hip_run_video refuses it; the identity view is acf_hip_run_image on the restated image."""
    n, size, code = 2, (96, 128), 3
    buf, desc, f = video_like("nv12", size, P010, 70, n)
    Hu, Wu = HipDetector.oriented_dims(size[0], size[1], code)
    det = HipDetector(synth.make_model(**TINY_RGB), Hu, Wu, 3, max_batch=n, max_hits=1 << 16)
    x = dev(buf)
    with pytest.raises(HipError) as e:
        det.run_video(x, n, desc, f, size[0], size[1], code)
    assert e.value.code == capi.E_UNSUPPORTED
    S = vfr.desc_to_rgb(buf, desc, size[0], size[1], P010, n).astype(F)
    U = np.ascontiguousarray(orf.orient(S, code, axes=(1, 2)))
    omax = vfr.coeffs(P010[0], P010[2], P010[3])[2]
    views = np.stack([vr.IDENTITY, vr.from_box((20, 10, 60, 80), vr.deg(15), Hu, Wu)])
    img = vr.image(U, views, None, Hu, Wu, 1, F(1.0 / omax))
    keep = run_f32_image(det, img)
    want = snapshot(det, n)
    det.run_view(det.crop_source_yuv(x, n, desc, f, size[0], size[1], code), views)
    assert assert_same(snapshot(det, n), want, "p010 orient 3") > 0
    del keep
    det.close()


# ---------------------------------------------------------------- 2. an integer translation is the strided sub-view

@pytest.mark.parametrize("kind", ["u8", "f32"])
def test_integer_translation_equals_run_image_on_the_sub_view(kind):
    import torch
    E = vr.stored_u8()[0] if kind == "u8" else vr.stored_f32()[0]
    t = dev(E)
    t = t.permute(0, 3, 1, 2) if kind == "u8" else t                                          # [n, 3, HS, WS] either way
    det = HipDetector(vr.model(), vr.H, vr.W, 3, max_batch=vr.NF, max_hits=vr.MAX_HITS)
    src = det.crop_source_tensor(t)
    total = 0
    for (tx, ty) in ((7, 5), (vr.WS - vr.W, vr.HS - vr.H)):
        det.run_tensor(t[:, :, ty:ty + vr.H, tx:tx + vr.W])
        want = snapshot(det, vr.NF)
        det.run_view(src, np.tile(vr.translation(tx, ty), (vr.NF, 1)))
        total += assert_same(snapshot(det, vr.NF), want, (kind, tx, ty))
    assert total > 0
    det.close()


# ---------------------------------------------------------------- 3. general views equal the definition

def nv12_stored():
    """(buffer, descriptor, U [NF][HS][WS][3] float32) of NV12 frames at the general cases' stored size"""
    buf, desc, _ = video_like("nv12", (vr.HS, vr.WS), None, 80, vr.NF)
    return buf, desc, ydr.desc_to_rgb(buf, desc, vr.HS, vr.WS, vr.NF).astype(F)


def general_source(det, kind):
    """-> (acf_hip_crop_source, U, unit, keep-alive)"""
    if kind == "u8":
        E, U = vr.stored_u8()
        x = dev(E)
        return det.crop_source_tensor(x, layout="nhwc"), U, F(1 / 255.0), x
    if kind == "f32":
        E, U = vr.stored_f32()
        x = dev(E)
        return det.crop_source_tensor(x), U, F(1), x
    buf, desc, U = nv12_stored()
    x = dev(buf)
    return det.crop_source_yuv(x, vr.NF, desc, None, vr.HS, vr.WS, 0), U, F(1 / 255.0), x


@pytest.mark.parametrize("kind", ["u8", "f32", "nv12"])
def test_general_views_equal_run_image_on_the_restated_image(oracle, kind):
    """Every view of the shared list, one call a view (its samples) with the frame index given and once more with frame_dev NULL;
    with option "taps" the plane itself is compared first, so that a sampling error shows at the plane and not at a hit.  The u8
    source runs once more under option "arith" = 1."""
    det = HipDetector(vr.model(), vr.H, vr.W, 3, max_batch=vr.NF, max_hits=vr.MAX_HITS, taps=True)
    src, U, unit, keep = general_source(det, kind)
    shape = (3, vr.W, vr.H)
    for arith in ((0, 1) if kind == "u8" else (0,)):
        if arith:
            det.set_x86_tables(*oracle.x86_fixture())
            det.set_option("arith", 1)
        for name, (m, s) in vr.VIEWS.items():
            for frames in ([vr.frame_choice(name)], None, [1, 0]):
                if arith and frames is None:
                    continue
                nv = 1 if frames is None or len(frames) == 1 else 2
                views = np.tile(m, (nv, 1))
                img = vr.image(U, views, frames, vr.H, vr.W, s, unit)
                k2 = run_f32_image(det, img)
                want = snapshot(det, nv)
                tap = [bits(det.read_tap(f, capi.TAP_IMAGE, 0, shape)) for f in range(nv)]
                det.run_view(src, views, None if frames is None else np.array(frames, np.int32), s)
                det.synchronize()
                for f in range(nv):
                    got = bits(det.read_tap(f, capi.TAP_IMAGE, 0, shape))
                    assert np.array_equal(got, tap[f]), (kind, name, frames, "plane", f, int((got != tap[f]).sum()))
                hits = assert_same(snapshot(det, nv), want, (kind, name, frames, arith))
                assert hits > 0 or name not in vr.DETECTING, (kind, name)
                del k2
    del keep
    det.close()


# ---------------------------------------------------------------- 4. one frame at several angles in one batch

def test_four_views_in_one_batch_equal_four_calls():
    det = HipDetector(vr.model(), vr.H, vr.W, 3, max_batch=4, max_hits=vr.MAX_HITS)
    src, U, unit, keep = general_source(det, "u8")
    frames = np.array([0, 0, 0, 1], np.int32)
    box = (20, 20, 128, 96)
    views = np.stack([HipDetector.view_from_box(box, vr.deg(a), vr.H, vr.W) for a in (-40, -20, 20, 40)])
    single = []
    for i in range(4):
        det.run_view(src, views[i:i + 1], frames[i:i + 1], 2)
        single += snapshot(det, 1)
    det.run_view(src, views, frames, 2)
    assert assert_same(snapshot(det, 4), single, "batch of four") > 0
    assert len({s[2] for s in single}) == 4                                                   # (four different pictures)
    del keep
    det.close()


# ---------------------------------------------------------------- 5. bounds: the clamped path on poisoned buffers that end with their extent

def test_far_nan_and_bad_frames_stay_inside_the_extent():
    import torch
    E, U = vr.stored_u8()
    strides = (vr.HS * (vr.WS * 3 + 5) + 11, 1, vr.WS * 3 + 5, 3)                             # padded rows and frames: poison between them
    buf = iec.lay_out(np.ascontiguousarray(E.transpose(0, 3, 1, 2)), capi.T_U8, strides)      # ends with the last addressed byte
    Ef = vr.stored_f32()[0][:, :1]                                                            # one f32 plane, NaN everywhere unaddressed
    fstr = (vr.HS * (vr.WS + 3) + 7, 0, vr.WS + 3, 1)
    fbuf = iec.lay_out(Ef, capi.T_F32, fstr)
    nvbuf, nvdesc, nvU = nv12_stored()                                                        # (tight: ends with its last byte)
    views = np.stack([vr.translation(1e9, 1e9), vr.translation(-1e9, 3), np.array([np.nan] * 6, F), np.array([np.inf, -np.inf, 0, 1, 1, np.nan], F),
                      np.array([1e30, 1e30, -1e30, 0.5, 0.5, 9], F), vr.IDENTITY, vr.VIEWS["tilt 20, s 1"][0], vr.translation(3, 4)])
    frames = np.array([0, 1, 0, 1, 0, -1, vr.NF, 1], np.int32)
    for kind in ("u8", "f32gray", "nv12"):
        ch = 1 if kind == "f32gray" else 3
        model = synth.make_model(**dict(TINY, name="FACE64", nTrees=64, minDs_h=32, minDs_w=32)) if ch == 1 else vr.model()
        det = HipDetector(model, vr.H, vr.W, ch, max_batch=len(views), max_hits=1 << 16)
        if kind == "u8":
            x = dev(buf)
            src, Uk, unit = det.crop_source_image(x.data_ptr(), vr.NF, capi.ImageDesc(capi.T_U8, 3, *strides), vr.HS, vr.WS), U, F(1 / 255.0)
        elif kind == "f32gray":
            x = dev(fbuf)
            src, Uk, unit = det.crop_source_image(x.data_ptr(), vr.NF, capi.ImageDesc(capi.T_F32, 1, *fstr), vr.HS, vr.WS), np.ascontiguousarray(Ef.transpose(0, 2, 3, 1)), F(1)
        else:
            x = dev(nvbuf)
            src, Uk, unit = det.crop_source_yuv(x, vr.NF, nvdesc, None, vr.HS, vr.WS, 0), nvU, F(1 / 255.0)
        for s in (1, 2):
            img = vr.image(Uk, views, frames, vr.H, vr.W, s, unit)
            assert np.isfinite(img).all() and not img[5].any() and not img[6].any()           # the restatement defines every one of them
            keep = run_f32_image(det, img)
            want = snapshot(det, len(views))
            det.run_view(src, views, frames, s)
            assert_same(snapshot(det, len(views)), want, (kind, s))
            del keep
        det.close()


# ---------------------------------------------------------------- 6. profile names; a captured graph survives

def test_profile_names_and_a_graph_still_replays():
    import torch
    det = HipDetector(vr.model(), vr.H, vr.W, 3, max_batch=vr.NF, max_hits=vr.MAX_HITS)
    det.set_option("graph", 1)
    fr = torch.from_numpy(np.stack([synth.make_frame(sd, vr.H, vr.W, "luv") for sd in vr.SEEDS])).cuda()
    for _ in range(3):                                                                        # plain, captured, replayed
        det.run(fr)
    want = snapshot(det, vr.NF)
    for kind, kname in (("u8", "k_ingest_view_image"), ("nv12", "k_ingest_view_yuv")):
        src, U, unit, keep = general_source(det, kind)
        det.set_option("profile", 1)
        det.profile()
        det.run_view(src, np.stack([vr.VIEWS["tilt 20, s 1"][0]] * 2))
        det.synchronize()
        names = det.profile()
        det.set_option("profile", 0)
        assert kname in names and not any(k.startswith("k_ingest") and k != kname for k in names), names
        det.run(fr)                                                                           # the captured graph, replayed
        assert assert_same(snapshot(det, vr.NF), want, "replay after " + kname) > 0
        del keep
    det.close()


# ---------------------------------------------------------------- 7. cut_detections after a view; the refusals that need a device

def test_cut_detections_refuses_after_a_view_and_works_after_a_plain_run():
    import torch
    det = HipDetector(vr.model(), vr.H, vr.W, 3, max_batch=vr.NF, max_hits=vr.MAX_HITS)
    E, U = vr.stored_u8()
    x = dev(E)
    src = det.crop_source_tensor(x, layout="nhwc")
    sub = x[:, 5:5 + vr.H, 7:7 + vr.W, :]                                                     # frames of the plan's size: what a plain run reads
    plain = det.crop_source_tensor(sub, layout="nhwc")
    det.run_view(src, np.tile(vr.translation(7, 5), (vr.NF, 1)))
    with pytest.raises(HipError) as e:
        det.cut_detections(plain, (16, 16), 2)
    assert e.value.code == capi.E_INVALID and "the last run was a view" in str(e.value)
    # the route to crops: view_box, then cut_crops on the stored frame
    d, _ = det.detections(0)
    assert len(d) > 0
    box = HipDetector.view_box(vr.translation(7, 5), [int(d[k][0]) for k in ("x", "y", "w", "h")])
    assert np.array_equal(box, np.array([d["x"][0] + 7, d["y"][0] + 5, d["w"][0], d["h"][0]], F))
    crops = det.cut_crops(src, box[None], np.array([0], np.int32), (16, 16))
    det.synchronize()
    assert tuple(crops.shape) == (1, 3, 16, 16)
    det.run_tensor(sub, layout="nhwc")
    crops, boxes, counts = det.cut_detections(plain, (16, 16), 2)
    det.synchronize()
    assert int(counts.cpu().numpy().sum()) > 0
    det.close()


def test_refusals():
    import torch
    det = HipDetector(vr.model())
    E, _ = vr.stored_u8()
    x = dev(E)
    src = det.crop_source_tensor(x, layout="nhwc")
    v = dev(identity(vr.NF))
    call = lambda d, s, views, frames, n, smp: d.lib.acf_hip_run_view(d.ctx, C.byref(s) if s is not None else None, C.c_void_p(views.data_ptr()) if views is not None else None,
                                                                     C.c_void_p(frames.data_ptr()) if frames is not None else None, n, smp)
    assert call(det, src, v, None, vr.NF, 1) == capi.E_NOPLAN
    det.plan(vr.H, vr.W, 3, max_batch=4, max_hits=vr.MAX_HITS)
    assert call(det, src, v, None, vr.NF, 1) == 0
    det.synchronize()
    for args in ((None, v, None, 1, 1), (src, None, None, 1, 1), (src, v, None, 1, 0), (src, v, None, 1, 5), (src, v, None, 0, 1), (src, v, None, 5, 1),
                 (src, v, None, vr.NF + 1, 1)):                                               # (frame_dev NULL with n_views > n_frames)
        assert call(det, *args) == capi.E_INVALID, args[3:]
    both = det.crop_source_tensor(x, layout="nhwc")
    both.yuv = C.pointer(HipDetector.yuv_desc("nv12", 96, 128)[0])
    neither = det.crop_source_tensor(x, layout="nhwc")
    neither.image = None
    bad_orient = det.crop_source_tensor(x, layout="nhwc", orient=8)
    gray = det.crop_source_tensor(x[..., :1], layout="nhwc")                                  # one channel against a plan for three
    for s in (both, neither, bad_orient, gray):
        assert call(det, s, v, None, 1, 1) == capi.E_INVALID
    det.close()
    # a five-plane plan, an active input resize, option "streams" > 1
    lm = synth.make_model(**TINY)
    det = HipDetector(lm, vr.H, vr.W, 5, max_batch=2, max_hits=vr.MAX_HITS)
    assert call(det, src, v, None, 1, 1) == capi.E_INVALID
    det.close()
    dr, dc = HipDetector.resize_dims(vr.HS, vr.WS, 0.75)
    det = HipDetector(vr.model(), dr, dc, 3, max_batch=2, max_hits=vr.MAX_HITS)
    det.set_input_resize(vr.HS, vr.WS, 0.75)
    assert call(det, src, v, None, 1, 1) == capi.E_INVALID
    det.close()
    det = HipDetector(vr.model(), vr.H, vr.W, 3, max_batch=4, max_hits=vr.MAX_HITS, streams=2)
    assert call(det, src, v, None, 1, 1) == capi.E_UNSUPPORTED
    det.close()
