"""The context's state by lifetime (acf_amd/csrc/acf_hip.hip: ModelState, PlanState with its LastRun, StreamFront): whatever a context
went through before — other plans, other models, refused calls, a stream, sub-batch children, captured graphs, every buffer that is
allocated at its first use — acf_hip_plan and acf_hip_set_model leave it giving what a context fresh from acf_hip_create gives.
Every comparison is against the oracle, bit for bit: the pyramid as uint32, detections and hits as bytes."""
import numpy as np
import pytest

import yuv420_ref as yr
from acf_amd import capi, synth
from acf_amd.dist import detections_to_record

pytestmark = pytest.mark.gpu

GRAY = dict(colorSpace=capi.CS_GRAY, isLuv=0)
LDCF = dict(ldcfK=2, modelDs_h=32, modelDs_w=32, modelDsPad_h=32, modelDsPad_w=32, minDs_h=32, minDs_w=32)
NMS = dict(type="maxg", overlap=0.65, ovrDnm="min", prune=True, maxCount=15, pruneRatio=0.1)
MAX_HITS = 1 << 14


def bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def tiny(**kw):
    return synth.make_model(**dict(dict(seed=3, name="TINY", nTrees=96, cascThr=-2.0), **kw))


def planes_of(kw):
    return 1 if kw.get("colorSpace") == capi.CS_GRAY else 3


def frames_of(kw, H, W, seeds):
    return np.stack([synth.make_frame(s, H, W, "gray" if planes_of(kw) == 1 else "luv") for s in seeds])


def oracle_run(oracle, kw, planar):
    """The oracle on one planar frame [d][W][H] under the model tiny(**kw) -> (pyramid, detections, hits)."""
    d, W, H = planar.shape
    plan = oracle.Plan(tiny(**kw), H, W, d)
    pyr, _, _ = oracle.chns_pyramid(plan, planar)
    if kw.get("ldcfK"):
        lvL, pyrL, _ = oracle.ldcf(plan, pyr)
        return (pyr,) + tuple(oracle.detect_ldcf(plan, lvL, pyrL))
    return (pyr,) + tuple(oracle.detect(plan, pyr))


_WANT = {}


def want_of(oracle, kw, H, W, seeds):
    """oracle_run of the synthetic frames `seeds`, computed once per (model, size, seed) and shared."""
    out = []
    for s in seeds:
        key = (tuple(sorted(kw.items())), H, W, s)
        if key not in _WANT:
            _WANT[key] = oracle_run(oracle, kw, frames_of(kw, H, W, [s])[0])
        out.append(_WANT[key])
    return out


def check(det, want, tag, ldcf=False):
    """The last batch of `det` against `want`; at least one detection in it."""
    for f, (pyr, wdet, whits) in enumerate(want):
        assert np.array_equal(bits(det.read_pyramid(f)), bits(pyr)), (tag, f)
        got, hits = det.detections(f)
        assert got.tobytes() == wdet.tobytes(), (tag, f, len(got), len(wdet))
        if ldcf:   # (as tests/test_gpu_pipeline.py holds the LDCF hits)
            assert all(np.array_equal(hits[k], whits[k]) for k in ("scale", "c", "r")), (tag, f)
        else:
            assert hits.tobytes() == whits.tobytes(), (tag, f)
    assert sum(len(w[1]) for w in want) > 0, tag


def check_nms(oracle, det, want, q, tag):
    """The last batch of `det`, run under acf_hip_set_nms(q): the survivors of the oracle's bbNms of the oracle's detections."""
    for f, (_, wdet, _) in enumerate(want):
        keep = oracle.nms(np.stack([wdet["x"], wdet["y"], wdet["w"], wdet["h"]], axis=1), wdet["score"].astype(np.float64), q)
        assert 1 <= len(keep) < len(wdet), (tag, f)
        assert det.detections(f)[0].tobytes() == wdet[keep].tobytes(), (tag, f)
        assert det.raw_detections(f).tobytes() == wdet.tobytes(), (tag, f)


def run(det, frames):
    import torch
    det.run(torch.from_numpy(frames).cuda())


def fresh_equals(det, kw, H, W, frames, tag, **ctor):
    """A context created for this geometry alone gives the bytes `det` holds for the same batch."""
    from acf_amd.detector import HipDetector
    ref = HipDetector(tiny(**kw), H, W, planes_of(kw), max_batch=len(frames), max_hits=MAX_HITS, **ctor)
    run(ref, frames)
    for f in range(len(frames)):
        assert np.array_equal(bits(ref.read_pyramid(f)), bits(det.read_pyramid(f))), (tag, f)
        assert [a.tobytes() for a in ref.detections(f)] == [a.tobytes() for a in det.detections(f)], (tag, f)
    forms = ref.tri_forms(), ref.level_forms()
    ref.close()
    return forms


def refused(call, code, text):
    from acf_amd.detector import HipError
    with pytest.raises(HipError) as e:
        call()
    assert e.value.code == code and text in str(e.value), (e.value.code, str(e.value))


def rgb_u8(seed, h, w):
    """A video-like upright frame, uint8 [h][w][3]."""
    return np.clip(np.rint(synth.make_frame(seed, h, w, "rgb").transpose(2, 1, 0) * 255.0), 0, 255).astype(np.uint8)


def planar_of(oracle, rgb):
    """The oracle's 8-bit image entry on tight RGB bytes [H][W][3] -> planar f32 [3][W][H]."""
    rgb = np.ascontiguousarray(rgb)
    H, W, _ = rgb.shape
    out = oracle.aligned((3, W, H))
    oracle.lib().acfo_ingest_u8(rgb.ctypes.data, H, W, 3, 0, 1, 2, W * 3, oracle.F(out), 3)
    return out


# ---------------------------------------------------------------- 1. a re-plan equals a fresh context

def test_replan_equals_fresh(oracle):
    """136 x 200 (batch 2) -> 64 x 96 (batch 4) -> 200 x 136 with a grey model, after every buffer that is allocated at its first use
    has been: the NMS buffers, the input resize's tables and reduced frames, the unfused NV12 -> RGB frames, the resized entries'
    tables, run_host's staging.  The settings survive the plan (NMS), what was built against it does not (the input resize)."""
    import torch
    from acf_amd.detector import HipDetector
    kw, q = {}, capi.make_nms(**NMS)
    (H, W), (H2, W2), (H3, W3) = (136, 200), (64, 96), (200, 136)
    fa = frames_of(kw, H, W, [11, 12])
    wa = want_of(oracle, kw, H, W, [11, 12])
    det = HipDetector(tiny(**kw), H, W, 3, max_batch=2, max_hits=MAX_HITS)
    run(det, fa)
    check(det, wa, "first plan")
    det.set_nms(q)
    run(det, fa)
    check_nms(oracle, det, wa, q, "first plan, NMS")
    det.set_nms(None)
    # frames of 68 x 100 enlarged twofold to the plan's size: NV12 through the input resize (k_yuv420_to_rgb8, k_resize_u8) ...
    sh, sw, scale = H // 2, W // 2, 2.0
    assert HipDetector.resize_dims(sh, sw, scale) == (H, W)
    small = [rgb_u8(21 + f, sh, sw) for f in range(2)]
    nv = [yr.from_rgb(s, False, 0, 0, 0) for s in small]
    det.set_input_resize(sh, sw, scale)
    det.run_u8(torch.from_numpy(np.stack(nv)).cuda(), capi.PIX_NV12)
    check(det, [oracle_run(oracle, kw, planar_of(oracle, oracle.resize_u8(yr.nv_to_rgb(b, sh, sw), scale))) for b in nv], "input resize, NV12")
    det.set_input_resize(0, 0, 1.0)
    # ... and as a tensor through the resized entry (its own tables)
    wsmall = [oracle_run(oracle, kw, planar_of(oracle, oracle.resize_u8(s, scale))) for s in small]
    t = torch.from_numpy(np.ascontiguousarray(np.stack(small).transpose(0, 3, 1, 2))).cuda()
    det.run_tensor_resized(t, scale)
    check(det, wsmall, "resized tensor")
    det.run_host(fa)
    check(det, wa, "run_host")
    det.set_input_resize(sh, sw, scale)   # left switched on, and the NMS too: the plan below meets both
    det.set_nms(q)

    fb = frames_of(kw, H2, W2, [31, 32, 33, 34])
    wb = want_of(oracle, kw, H2, W2, [31, 32, 33, 34])
    det.plan(H2, W2, 3, max_batch=4, max_hits=MAX_HITS)
    run(det, fb)
    check_nms(oracle, det, wb, q, "second plan, NMS")      # (the setting survived the plan, its buffers are new ones)
    det.set_nms(None)
    run(det, fb)
    check(det, wb, "second plan")
    fresh_equals(det, kw, H2, W2, fb, "second plan")
    # the input resize is off again: the resized entry (refused beside it) runs, from tables built for this plan
    s2 = [rgb_u8(41 + f, H2 // 2, W2 // 2) for f in range(4)]
    det.run_tensor_resized(torch.from_numpy(np.ascontiguousarray(np.stack(s2).transpose(0, 3, 1, 2))).cuda(), scale)
    check(det, [oracle_run(oracle, kw, planar_of(oracle, oracle.resize_u8(s, scale))) for s in s2], "resized tensor, second plan")
    refused(lambda: det.run_tensor_resized(t, scale), capi.E_INVALID, "the plan must be for the reduced size")   # (the first plan's key)

    det.set_model(tiny(**GRAY))
    det.plan(H3, W3, 1, max_batch=2, max_hits=MAX_HITS)
    fc = frames_of(GRAY, H3, W3, [51, 52])
    run(det, fc)
    check(det, want_of(oracle, GRAY, H3, W3, [51, 52]), "third plan")
    fresh_equals(det, GRAY, H3, W3, fc, "third plan")
    det.close()


# ---------------------------------------------------------------- 2. another model under a plan

def test_model_change_under_a_plan(oracle):
    """acf_hip_set_model drops the plan (depth 2 -> depth 3: other tile sets and tables); the LDCF filters are the model's and
    outlive it, the LDCF stage is the plan's and goes with it."""
    from acf_amd.detector import HipDetector
    H, W = 136, 200
    fr = frames_of({}, H, W, [11, 12])
    det = HipDetector(tiny(), H, W, 3, max_batch=2, max_hits=MAX_HITS)
    run(det, fr)
    check(det, want_of(oracle, {}, H, W, [11, 12]), "depth 2")
    for kw in (dict(treeDepth=3), LDCF, {}):
        det.set_model(tiny(**kw))
        refused(lambda: run(det, fr), capi.E_NOPLAN, "pyramid: plan first")
        refused(lambda: det.read_level(0, 0), capi.E_NOPLAN, "read_level: plan first")
        det.plan(H, W, 3, max_batch=2, max_hits=MAX_HITS)
        run(det, fr)
        check(det, want_of(oracle, kw, H, W, [11, 12]), kw, ldcf="ldcfK" in kw)
    det.close()


# ---------------------------------------------------------------- 3. refused plans and models

def test_refused_plans(oracle):
    """A plan refused for its batch arguments leaves the previous plan in use; one refused later leaves none."""
    import ctypes as C
    from acf_amd.detector import HipDetector
    H, W = 136, 200
    fr = frames_of({}, H, W, [11, 12])
    want = want_of(oracle, {}, H, W, [11, 12])
    det = HipDetector(tiny(), H, W, 3, max_batch=2, max_hits=MAX_HITS)
    refused(lambda: det.plan(H, W, 3, max_batch=0, max_hits=MAX_HITS), capi.E_INVALID, "plan: max_batch/max_hits")
    refused(lambda: det.plan(H, W, 3, max_batch=2, max_hits=0), capi.E_INVALID, "plan: max_batch/max_hits")
    run(det, fr)
    check(det, want, "after the refused batch arguments")

    def unplanned(tag):
        n = C.c_int()
        refused(lambda: run(det, fr), capi.E_NOPLAN, "pyramid: plan first")
        refused(lambda: det.read_level(0, 0), capi.E_NOPLAN, "read_level: plan first")
        refused(lambda: det._chk(det.lib.acf_hip_num_levels(det.ctx, C.byref(n), None)), capi.E_NOPLAN, "num_levels: plan first")

    # refused after the previous plan has gone: a plane count no plan is built for; a smoothing radius the kernels do not implement
    refused(lambda: det.plan(H, W, 2, max_batch=2, max_hits=MAX_HITS), capi.E_INVALID, "plan: bad frame geometry")
    unplanned("geometry")
    det.plan(H, W, 3, max_batch=2, max_hits=MAX_HITS)
    run(det, fr)
    check(det, want, "planned again")
    det.set_model(tiny(smooth=1.5))
    refused(lambda: det.plan(H, W, 3, max_batch=2, max_hits=MAX_HITS), capi.E_UNSUPPORTED, "plan: smoothing radius must be 0 or in (0,1]")
    unplanned("smoothing radius")
    det.set_model(tiny())
    det.plan(H, W, 3, max_batch=2, max_hits=MAX_HITS)
    run(det, fr)
    check(det, want, "a good model and plan")
    det.close()


def test_refusals_on_a_context_with_children(oracle):
    """Sub-batch children hold the plan's buffers, so they stay and go with the plan, never alone: a refused model leaves plan and
    children in use (a planned context without its children would run on buffers it does not have), a refused plan leaves neither
    (children left behind would go on running the plan before it)."""
    from acf_amd.detector import HipDetector
    H, W = 136, 200
    fr = frames_of({}, H, W, [11, 12, 13, 14])
    want = want_of(oracle, {}, H, W, [11, 12, 13, 14])
    det = HipDetector(tiny(), H, W, 3, max_batch=4, max_hits=MAX_HITS, streams=2)
    run(det, fr)
    check(det, want, "children")
    refused(lambda: det.set_model(dict(tiny(), treeDepth=9)), capi.E_INVALID, "set_model: treeDepth must be 0..8")
    run(det, fr)
    check(det, want, "children, after a refused model")
    refused(lambda: det.plan(H, W, 2, max_batch=4, max_hits=MAX_HITS), capi.E_INVALID, "plan: bad frame geometry")
    refused(lambda: run(det, fr), capi.E_NOPLAN, "pyramid: plan first")
    refused(lambda: det.read_level(0, 0), capi.E_NOPLAN, "read_level: plan first")
    det.plan(H, W, 3, max_batch=4, max_hits=MAX_HITS)
    run(det, fr)
    check(det, want, "children, planned again")
    det.close()


# ---------------------------------------------------------------- 4. a stream across a re-plan

def test_stream_across_a_replan(oracle):
    """acf_hip_plan closes the stream; the next one starts from ticket 0 and gives the records of the oracle's detections."""
    from acf_amd.detector import HipDetector, PinnedBuffer
    cap, n = 2048, 2
    det = HipDetector(tiny(), 136, 200, 3, max_batch=n, max_hits=MAX_HITS)
    pin = PinnedBuffer(n * 136 * 200 * 3)

    def one_batch(H, W, seeds):
        x = np.stack([rgb_u8(s, H, W) for s in seeds])
        pin.array[:x.size] = x.ravel()
        ticket = det.stream_submit(pin.ptr.value, n)
        assert ticket == 0                                  # (the first of ITS stream)
        rec = det.stream_collect(ticket)
        want = [oracle_run(oracle, {}, planar_of(oracle, f)) for f in x]
        assert sum(len(w[1]) for w in want) > 0 and max(len(w[1]) for w in want) <= cap
        for f in range(n):
            assert np.array_equal(rec[f], detections_to_record(want[f][1], cap)), (H, W, f)

    det.stream_open(capi.PIX_RGB, 0, cap, 2)
    one_batch(136, 200, [61, 62])
    det.plan(64, 96, 3, max_batch=n, max_hits=MAX_HITS)
    refused(lambda: det.stream_submit(pin.ptr.value, n), capi.E_INVALID, "stream_submit: stream_open first")
    refused(lambda: det.stream_collect(0), capi.E_INVALID, "stream_collect: stream_open first")
    det.stream_open(capi.PIX_RGB, 0, cap, 2)
    one_batch(64, 96, [63, 64])
    det.stream_close()
    refused(lambda: det.stream_submit(pin.ptr.value, n), capi.E_INVALID, "stream_submit: stream_open first")
    det.close()
    pin.close()


# ---------------------------------------------------------------- 5. children <-> own buffers

def test_children_and_own_buffers_alternate(oracle):
    """Option streams 2 -> 1 -> 2 across plans of different sizes: each run is the oracle's, and the forms read back are those of a
    context that only ever had this plan — from the children while there are some, from the context itself while there are none."""
    from acf_amd.detector import HipDetector
    seeds = [11, 12, 13, 14]
    det = HipDetector(streams=2)
    det.set_model(tiny())
    for streams, (H, W) in ((2, (136, 200)), (1, (64, 96)), (2, (200, 136)), (1, (136, 200))):
        det.set_option("streams", streams)
        det.plan(H, W, 3, max_batch=4, max_hits=MAX_HITS)
        fr = frames_of({}, H, W, seeds)
        run(det, fr)
        check(det, want_of(oracle, {}, H, W, seeds), (streams, H, W))
        tri, lev = fresh_equals(det, {}, H, W, fr, (streams, H, W), streams=streams)
        assert det.tri_forms() == tri and len(tri) > 0, (streams, H, W)
        assert det.level_forms() == lev and len(lev["levels"]) == len(det.levels), (streams, H, W)
    det.close()


# ---------------------------------------------------------------- 6. captured graphs across a re-plan

def test_graph_slots_across_a_replan(oracle):
    """Option graph: a plain run, the capturing one and a replay on one input tensor, under two plans; acf_hip_set_nms between replays
    drops the captured run, whose host-side state no longer holds."""
    import torch
    from acf_amd.detector import HipDetector
    q = capi.make_nms(**NMS)
    det = HipDetector(tiny(), 136, 200, 3, max_batch=2, max_hits=MAX_HITS)
    det.set_option("graph", 1)
    for H, W, seeds in ((136, 200, [11, 12]), (64, 96, [31, 32])):
        det.plan(H, W, 3, max_batch=2, max_hits=MAX_HITS)
        want = want_of(oracle, {}, H, W, seeds)
        dev = torch.from_numpy(frames_of({}, H, W, seeds)).cuda()
        for k in range(3):
            det.run(dev)
            check(det, want, (H, W, "run", k))
        det.set_nms(q)
        for k in range(3):
            det.run(dev)
            check_nms(oracle, det, want, q, (H, W, "NMS run", k))
        det.set_nms(None)
        det.run(dev)
        check(det, want, (H, W, "NMS off"))
    det.close()
