"""The oriented resized tensor and YUV entries on the GPU (include/acf_hip.h: acf_hip_pyramid_image_oriented_resized /
run_image_oriented_resized / pyramid_yuv_oriented_resized / run_yuv_oriented_resized / stream_open_yuv_oriented_resized; kernel
k_ingest_oriented_resized, staged and generic).

The reference is the definition: the existing acf_hip_run_image_resized on a device tensor holding the numpy-oriented tight upright u8
image (for YUV: the numpy restatement's R, G, B, chroma chosen in source coordinates, oriented) — every level as uint32, the detection
bytes and the hit bytes — and, for the detections, the oracle chain on the same image (tests/oriented_resized_case.py: expected).
tests/test_oriented_resized_entries.py holds the preconditions: every case detects something in every frame, and the other order of
the two steps gives other bytes."""
import ctypes as C
import functools
import os
import subprocess
import sys

import numpy as np
import pytest

import orient_ref as orf
import oriented_resized_case as orc
import resized_entry_case as rc
from acf_amd import capi, synth

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NF = orc.NF

NAME = {("yuv", "staged"): "k_ingest_oriented_resized_yuv", ("yuv", "generic"): "k_ingest_oriented_resized_yuv_generic",
        ("image", "staged"): "k_ingest_oriented_resized_image", ("image", "generic"): "k_ingest_oriented_resized_image_generic"}


def same(got, want, tag):
    assert len(got) == len(want), tag
    for f, ((gl, gd, gh), (wl, wd, wh)) in enumerate(zip(got, want)):
        assert len(gl) == len(wl), (tag, f)
        for i, (a, b) in enumerate(zip(gl, wl)):
            assert np.array_equal(a, b), (tag, f, "level", i)
        assert gd == wd and gh == wh, (tag, f)


def upright_reference(det, case):
    """snapshot of the existing run_image_resized on the tight upright image (NHWC interleaved, `channels` bytes a pixel)"""
    up = orc.upright(case)
    n, h, w, cn = up.shape
    u = orc.dev(up)
    det.run_image_resized(u.data_ptr(), n, capi.ImageDesc(capi.T_U8, cn, h * w * cn, 1, w * cn, cn), h, w, case.scale)
    return orc.snapshot(det)


# ---------------------------------------------------------------- 1. the definition, through run_* and pyramid_*; 3. the form that ran

@pytest.mark.parametrize("case", orc.CASES, ids=orc.IDS)
def test_entry_equals_run_image_resized_on_the_upright_image(oracle, case):
    b = orc.built(case)
    det = orc.detector(case, oracle)
    x = orc.dev(b.buf)
    # the pyramid entry alone, on the fresh context
    orc.run_entry(det, case, x, pyramid_only=True)
    det.synchronize()
    levels = [[orc.bits(det.read_level(f, i)) for i in range(len(det.levels))] for f in range(NF)]
    want = upright_reference(det, case)
    for f in range(NF):
        for i in range(len(det.levels)):
            assert np.array_equal(levels[f][i], want[f][0][i]), (case.id, "pyramid entry", f, i)
    names = orc.ingest_names(det, lambda: orc.run_entry(det, case, x))
    got = orc.snapshot(det)
    same(got, want, case.id)
    assert names == [NAME[(b.kind, case.form)]], (case.id, names)
    # the oracle chain on the same image: the detections and hits
    plan, exp = orc.expected(oracle, case)
    for f, (pyr, wdet, whits) in enumerate(exp):
        assert got[f][1] == wdet.tobytes() and got[f][2] == whits.tobytes(), (case.id, f)
        assert len(wdet) > 0
    det.close()


# ---------------------------------------------------------------- 2. the forced generic form: one fresh child for all cases

@functools.lru_cache(maxsize=None)
def _forced_generic():
    env = dict(os.environ)
    env["ACF_HIP_FORCE_FALLBACK"] = "oriented_resized_generic"
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "oriented_resized_case.py")], cwd=ROOT, env=env, capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    out = {}
    for line in r.stdout.splitlines():
        cid, sha, names = line.split()
        out[cid] = (sha, names.split(","))
    return out


@pytest.mark.parametrize("case", [c for c in orc.CASES if c.form == "staged"], ids=[c.id for c in orc.CASES if c.form == "staged"])
def test_forced_generic_form_gives_the_same_bytes(oracle, case):
    forced = _forced_generic()
    b = orc.built(case)
    sha, names = forced[case.id]
    assert names == [NAME[(b.kind, "generic")]], (case.id, names)
    det = orc.detector(case, oracle)
    assert orc.digest(upright_reference(det, case)) == sha, case.id
    det.close()


def test_the_child_ran_every_case():
    assert sorted(_forced_generic()) == sorted(orc.IDS)


# ---------------------------------------------------------------- 4. code 0 forwards

def test_code_0_is_the_resized_entry(oracle):
    case = orc.by_id("i420_frac_o1")._replace(code=0)
    b = orc.built(case)
    det = orc.detector(case)
    x = orc.dev(b.buf)
    det.run_yuv_resized(x, NF, b.desc, case.H, case.W, case.scale)
    want = orc.snapshot(det)
    sc = C.c_double(case.scale)
    names = orc.ingest_names(det, lambda: det._chk(det.lib.acf_hip_run_yuv_oriented_resized(det.ctx, C.c_void_p(x.data_ptr()), NF, C.byref(b.desc), case.H, case.W, 0, sc)))
    same(orc.snapshot(det), want, "code 0")
    assert names == ["k_ingest_resized_yuv"], names
    same(upright_reference(det, case), want, "code 0 is the upright image")
    assert sum(len(w[1]) for w in want) > 0
    img = orc.by_id("nchw_frac_o1")._replace(code=0)
    bi = orc.built(img)
    di = orc.detector(img)
    xi = orc.dev(bi.buf)
    names = orc.ingest_names(di, lambda: di._chk(di.lib.acf_hip_run_image_oriented_resized(di.ctx, C.c_void_p(xi.data_ptr()), NF, C.byref(bi.desc), img.H, img.W, 0, sc)))
    assert names == ["k_ingest_resized_image"], names
    same(orc.snapshot(di), upright_reference(di, img), "image, code 0")
    di.close()
    det.close()


# ---------------------------------------------------------------- 5. streaming

@pytest.mark.parametrize("code", [1, 6])
def test_stream_matches_blocking_calls(code):
    """Three tickets (the last one short) at depth 2 give the records of run_yuv_resized(orient) + export_detections of each batch."""
    import torch
    import yuv_desc_ref as ydr
    from acf_amd.detector import HipDetector, PinnedBuffer
    H, W, scale = 242, 320, orc.S150
    cap, nB, depth = 512, 2, 2
    dr, dc = HipDetector.oriented_resized_dims(H, W, code, scale)
    det = HipDetector(synth.make_model(**orc.FACE80), dr, dc, 3, max_batch=nB, max_hits=1 << 16)
    d, fb = HipDetector.yuv_desc("i420", H, W)
    batches = [np.stack([ydr.pack("i420", *rc.yuv_planes(500 + 10 * k + i, H, W, 1, 1)) for i in range(nB if k != 2 else 1)]) for k in range(3)]
    want = []
    for x in batches:
        xd = orc.dev(x)
        det.run_yuv_resized(xd, x.shape[0], d, H, W, scale, code)
        dst = torch.zeros((x.shape[0], 1 + 6 * cap), dtype=torch.int32, device="cuda")
        torch.cuda.synchronize()                                          # (torch fills dst on its own stream: before the export writes it)
        det.export_detections(dst, cap)
        det.synchronize()
        want.append(dst.cpu().numpy())
    assert sum(int(x[:, 0].sum()) for x in want) > 0
    pins = [PinnedBuffer(nB * fb) for _ in range(depth)]
    det.stream_open_yuv_resized(d, fb, H, W, scale, cap, depth, orient=code)
    got, inflight = [], []
    for k, x in enumerate(batches):
        if len(inflight) == depth:
            got.append(det.stream_collect(inflight.pop(0)))
        pin = pins[k % depth]
        pin.array[:x.size] = x.ravel()
        inflight.append(det.stream_submit(pin.ptr.value, x.shape[0]))
    while inflight:
        got.append(det.stream_collect(inflight.pop(0)))
    for k in range(3):
        assert got[k].shape == want[k].shape, k
        for f in range(want[k].shape[0]):
            n = want[k][f, 0]
            assert got[k][f, 0] == n
            assert np.array_equal(got[k][f, :1 + 6 * n], want[k][f, :1 + 6 * n]), (k, f)
    det.stream_close()
    det.close()
    for p in pins:
        p.close()


# ---------------------------------------------------------------- 6. what is refused

def test_refusals_one_for_each_code():
    import torch
    from acf_amd.detector import HipDetector, HipError
    model = synth.make_model(seed=3, name="TINY", nTrees=16)
    H, W, scale, code = 192, 256, 0.5, 1
    h, w = HipDetector.oriented_resized_dims(H, W, code, scale)
    assert (h, w) == (128, 96)
    x = torch.zeros(4 * H * W * 4, dtype=torch.uint8).cuda()
    good, fb = HipDetector.yuv_desc("i420", H, W)
    img = capi.ImageDesc(capi.T_U8, 3, 3 * H * W, H * W, W, 1)
    ptr = x.data_ptr()

    def refused(fn, want=capi.E_INVALID):
        with pytest.raises(HipError) as e:
            fn()
        assert e.value.code == want, e.value

    det = HipDetector(model, h, w, 3, max_batch=2)
    lib, sc = det.lib, C.c_double(scale)
    det.run_yuv_resized(x, 2, good, H, W, scale, code)                    # accepted as they are
    det.run_image_resized(ptr, 2, img, H, W, scale, code)
    det.stream_open_yuv_resized(good, fb, H, W, scale, 64, 2, orient=code)
    det.stream_close()
    # what either parent family refuses: null pointers, the batch size, a bad description
    assert lib.acf_hip_run_yuv_oriented_resized(det.ctx, None, 1, C.byref(good), H, W, code, sc) == capi.E_INVALID
    assert lib.acf_hip_run_image_oriented_resized(det.ctx, C.c_void_p(ptr), 1, None, H, W, code, sc) == capi.E_INVALID
    assert lib.acf_hip_pyramid_yuv_oriented_resized(None, C.c_void_p(ptr), 1, C.byref(good), H, W, code, sc) == capi.E_INVALID
    assert lib.acf_hip_stream_open_yuv_oriented_resized(det.ctx, None, fb, H, W, code, sc, 64, 2) == capi.E_INVALID
    refused(lambda: det.run_yuv_resized(x, 3, good, H, W, scale, code))
    bad = capi.YuvDesc.from_buffer_copy(good)
    bad.sub_x = 2
    refused(lambda: det.run_yuv_resized(x, 1, bad, H, W, scale, code))
    badi = capi.ImageDesc.from_buffer_copy(img)
    badi.channels = 2
    refused(lambda: det.run_image_resized(ptr, 1, badi, H, W, scale, code))
    # orient outside 0 .. 7
    for o in (8, -1):
        refused(lambda: det.run_yuv_resized(x, 1, good, H, W, scale, o))
        refused(lambda: det.pyramid_yuv_resized(x, 1, good, H, W, scale, o))
        refused(lambda: det.run_image_resized(ptr, 1, img, H, W, scale, o))
        refused(lambda: det.pyramid_image_resized(ptr, 1, img, H, W, scale, o))
        refused(lambda: det.stream_open_yuv_resized(good, fb, H, W, scale, 64, 2, orient=o))
    # a plan of other dimensions: the un-turned size, another scale, another frame size
    for rows, cols, s, o in ((H, W, scale, 2), (H, W, 0.75, code), (H + 2, W, scale, code), (W, H, scale, code), (0, W, scale, code)):
        refused(lambda: det.run_yuv_resized(x, 1, good, rows, cols, s, o))
        refused(lambda: det.run_image_resized(ptr, 1, img, rows, cols, s, o))
        refused(lambda: det.stream_open_yuv_resized(good, fb, rows, cols, s, 64, 2, orient=o))
    # a scale that is not a positive finite number
    for s in (0.0, -0.5, float("nan"), float("inf")):
        refused(lambda: det.run_yuv_resized(x, 1, good, H, W, s, code))
        refused(lambda: det.run_image_resized(ptr, 1, img, H, W, s, code))
        refused(lambda: det.stream_open_yuv_resized(good, fb, H, W, s, 64, 2, orient=code))
    # an image dtype other than u8
    for dt in (capi.T_F16, capi.T_BF16, capi.T_F32):
        f = capi.ImageDesc.from_buffer_copy(img)
        f.dtype = dt
        refused(lambda: det.run_image_resized(ptr, 1, f, H, W, scale, code), capi.E_UNSUPPORTED)
    # an active input resize
    det.set_input_resize(2 * h, 2 * w, 0.5)
    refused(lambda: det.run_yuv_resized(x, 1, good, H, W, scale, code))
    refused(lambda: det.run_image_resized(ptr, 1, img, H, W, scale, code))
    refused(lambda: det.stream_open_yuv_resized(good, fb, H, W, scale, 64, 2, orient=code))
    det.set_input_resize(0, 0, 1.0)
    det.run_yuv_resized(x, 1, good, H, W, scale, code)                    # ... and the context is usable afterwards
    det.synchronize()
    # a five-plane plan, a one-plane plan for YUV
    five = HipDetector(model, h, w, 5, max_batch=1)
    refused(lambda: five.run_yuv_resized(x, 1, good, H, W, scale, code))
    refused(lambda: five.run_image_resized(ptr, 1, img, H, W, scale, code))
    five.close()
    g = HipDetector(synth.make_model(seed=3, name="FACE64", nTrees=16), h, w, 1, max_batch=1)
    refused(lambda: g.run_yuv_resized(x, 1, good, H, W, scale, code))
    g.close()
    # no plan; option "streams" > 1
    bare = HipDetector(model)
    refused(lambda: bare.run_yuv_resized(x, 1, good, H, W, scale, code), capi.E_NOPLAN)
    refused(lambda: bare.run_image_resized(ptr, 1, img, H, W, scale, code), capi.E_NOPLAN)
    refused(lambda: bare.stream_open_yuv_resized(good, fb, H, W, scale, 64, 2, orient=code), capi.E_NOPLAN)
    bare.close()
    multi = HipDetector(model, h, w, 3, max_batch=4, streams=2)
    refused(lambda: multi.run_yuv_resized(x, 2, good, H, W, scale, code), capi.E_UNSUPPORTED)
    refused(lambda: multi.run_image_resized(ptr, 2, img, H, W, scale, code), capi.E_UNSUPPORTED)
    refused(lambda: multi.stream_open_yuv_resized(good, fb, H, W, scale, 64, 2, orient=code), capi.E_UNSUPPORTED)
    multi.close()
    det.close()


# ---------------------------------------------------------------- 7. run_yuv_planes(scale=, orient=); the boxes back

def test_run_yuv_planes_with_scale_and_orient_equals_the_descriptor_path():
    case = orc.by_id("planes_odd_037_o1")
    b = orc.built(case)
    det = orc.detector(case)
    x = orc.dev(b.buf)
    det.run_yuv_resized(x.data_ptr() + b.base, NF, b.desc, case.H, case.W, case.scale, case.code)
    want = orc.snapshot(det)
    y, u, v = (x[at:at + int(np.prod(shape))].view(shape) for at, shape in b.planes)
    base, n, d = det.yuv_planes_desc(y, u, v, 1, 1)
    assert n == NF and bytes(d) == bytes(b.desc)
    det.run_yuv_planes(y, u, v, 1, 1, scale=case.scale, orient=case.code)
    same(orc.snapshot(det), want, case.id)
    assert sum(len(w[1]) for w in want) > 0
    det.close()


@pytest.mark.parametrize("cid", ["i420_frac_o1", "nchw_third_o6"])
def test_boxes_map_back_into_the_stored_frame(oracle, cid):
    """unscale_boxes, then unorient_boxes: the host-composed mapping, and the boxes lie in the stored frame (the model's padding and the
    rounding of the reduced size allowed for)."""
    from acf_amd.detector import HipDetector
    case = orc.by_id(cid)
    b = orc.built(case)
    det = orc.detector(case)
    x = orc.dev(b.buf)
    orc.run_entry(det, case, x)
    uh, uw = orc.upright_dims(case)
    m = synth.make_model(**case.model)
    slack = int(np.ceil((max(m["modelDsPad_h"] - m["modelDs_h"], m["modelDsPad_w"] - m["modelDs_w"]) + 1) / case.scale)) + 1
    total = 0
    for f in range(NF):
        d, _ = det.detections(f)
        back = HipDetector.unorient_boxes(HipDetector.unscale_boxes(d, case.scale), case.code, case.H, case.W)
        for r, o in zip(d, back):
            up = oracle.unscale_rect(case.scale, [r["x"], r["y"], r["w"], r["h"]])
            assert [int(o[k]) for k in "xywh"] == orf.unorient_box(case.code, case.H, case.W, up)
            assert -slack <= o["x"] and o["x"] + o["w"] <= case.W + slack and -slack <= o["y"] and o["y"] + o["h"] <= case.H + slack, (cid, f, o)
            assert (o["w"], o["h"]) == ((up[3], up[2]) if case.code & 1 else (up[2], up[3]))
        total += len(d)
    assert total > 0
    det.close()
