"""The views' detections merged into their stored frames on the GPU (include/acf_hip.h: acf_hip_merge_views / acf_hip_op_merge_views;
kernel k_merge_views).  Every comparison is of raw bytes against the numpy restatement of the header's rule (tests/merge_views_ref.py):
  1. every designed case through acf_hip_op_merge_views, on outputs pre-filled with a sentinel byte: records, counts, boxes, frame
     indices and quads, the slots beyond the count included;
  2. the pipeline case: run_view with the device NMS off and with the per-view NMS on, merge_views against the restatement fed with
     get_detections of every view, for types 0, 1 and 2; then acf_hip_cut_crops on boxes_out / frames_out (the device-only route)
     against cut_crops on boxes built on the host with acf_hip_view_box and the restatement's NMS (the route of before);
  3. what the call leaves alone, its refusals, its profile name and a captured graph;
  4. acf_hip_detect --view ... --merge prints the Python path's quads.
tests/test_merge_views.py holds the preconditions: the restatement against the CPU oracle, and that no case is vacuous."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

import merge_views_ref as mr
import view_ref as vr
from acf_amd import capi, synth
from acf_amd.detector import HipDetector, HipError

pytestmark = pytest.mark.gpu
F = np.float32
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("records", "counts", "boxes", "frame indices", "quads")


def dev(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def assert_bytes(got, want, tag):
    for name, g, w in zip(NAMES, got, want):
        g, w = np.ascontiguousarray(g), np.ascontiguousarray(w)
        assert g.shape == w.shape, (tag, name, g.shape, w.shape)
        if g.tobytes() != w.tobytes():
            bad = np.flatnonzero(g.view(np.uint8).ravel() != w.view(np.uint8).ravel())
            raise AssertionError((tag, name, "bytes that differ", len(bad), "first at", int(bad[0]), "counts", list(np.ravel(got[1])), list(np.ravel(want[1]))))


# ---------------------------------------------------------------- 1. the designed cases through the op entry

@pytest.fixture(scope="module")
def bare():
    det = HipDetector()                                                                       # a context: no model, no plan
    yield det
    det.close()


@pytest.mark.parametrize("name", list(mr.cases()))
def test_designed_case_equals_the_restatement(bare, name):
    c = mr.cases()[name]
    got = bare.op_merge_views(c["dets"], c["counts"], c["views"], c.get("frames"), c.get("n_frames"), c["nms"], c.get("k", 8), c.get("grow", 1.0), fill=mr.FILL)
    assert_bytes(got, mr.expected(name), name)


def test_optional_outputs_may_be_null(bare):
    c = mr.cases()["two frames interleaved"]
    want = mr.expected("two frames interleaved")
    dets, counts, views = np.ascontiguousarray(c["dets"]), np.ascontiguousarray(c["counts"], np.int32), np.ascontiguousarray(c["views"], F)
    frames = np.array(c["frames"], np.int32)
    spec = HipDetector.merge_spec(c["nms"], 8, 1.0)
    rec, cnt = np.full((2, 8, 32), mr.FILL, np.uint8), np.zeros(2, np.int32)
    p = lambda a: C.c_void_p(a.ctypes.data)
    rc = bare.lib.acf_hip_op_merge_views(bare.ctx, p(dets), p(counts), dets.shape[1], p(views), p(frames), 5, 2, C.byref(spec), p(rec), p(cnt), None, None, None)
    assert rc == 0 and rec.tobytes() == want[0].tobytes() and cnt.tolist() == want[1].tolist()


def test_argument_refusals_with_a_real_context(bare):
    """what tests/test_merge_views.py sends to a null context, to a real one: the argument checks themselves"""
    import test_merge_views as tm
    c = mr.cases()["two frames interleaved"]
    dets, counts, views = np.ascontiguousarray(c["dets"]), np.ascontiguousarray(c["counts"], np.int32), np.ascontiguousarray(c["views"], F)
    frames = np.array(c["frames"], np.int32)
    rec, cnt = np.zeros((2, 8, 32), np.uint8), np.zeros(2, np.int32)
    p = lambda a: C.c_void_p(a.ctypes.data) if a is not None else None
    good = tm.spec_of(k=8)
    op = lambda d=dets, cn=counts, mh=dets.shape[1], v=views, n=5, nf=2, spec=good, out=rec, co=cnt: bare.lib.acf_hip_op_merge_views(
        bare.ctx, p(d), p(cn), mh, p(v), p(frames), n, nf, C.byref(spec) if spec else None, p(out), p(co), None, None, None)
    pipe = lambda v=views, n=5, nf=2, spec=good, out=rec, co=cnt: bare.lib.acf_hip_merge_views(bare.ctx, p(v), None, n, nf, C.byref(spec) if spec else None, p(out), p(co),
                                                                                                None, None, None)
    assert op() == 0 and cnt.tolist() == mr.expected("two frames interleaved")[1].tolist()
    for fn in (op, pipe):
        for kw in (dict(v=None), dict(out=None), dict(co=None), dict(spec=None), dict(n=0), dict(n=-1), dict(n=capi.MERGE_VIEWS_MAX + 1), dict(nf=0), dict(nf=-3)):
            assert fn(**kw) == capi.E_INVALID, kw
        for kw in tm.BAD_SPECS:
            assert fn(spec=tm.spec_of(**kw)) == capi.E_INVALID, kw
    for kw in (dict(d=None), dict(cn=None), dict(mh=0)):
        assert op(**kw) == capi.E_INVALID, kw
    assert pipe() == capi.E_INVALID and b"acf_hip_run_view first" in bare.lib.acf_hip_last_error(bare.ctx)   # good arguments: only the missing view run is left
    assert op() == 0                                                                          # the context still works


# ---------------------------------------------------------------- 2. the pipeline case

def host_route(det, views, frames, n_frames, q, k, grow):
    """the route of before: get_detections per view, acf_hip_view_box on the host, the restatement's NMS -> (boxes [nF * k][4], frame
    indices [nF * k]) with the merged boxes in the leading slots of every frame, (0, -1) behind them"""
    boxes, fidx = np.zeros((n_frames, k, 4), F), np.full((n_frames, k), -1, np.int32)
    for f in range(n_frames):
        ent = [(v, d) for v in range(len(views)) if frames[v] == f for d in det.detections(v)[0]]
        bx = [HipDetector.view_box(views[v], [int(d[t]) for t in ("x", "y", "w", "h")]) for v, d in ent]
        if q.type == 0:
            keep = list(range(len(ent)))
        else:
            keep, _ = mr.suppress(bx, [d["score"] for _, d in ent], q)
        for s, t in enumerate(keep[:k]):
            boxes[f, s], fidx[f, s] = mr.grown(bx[t], grow), f
    return boxes.reshape(-1, 4), fidx.reshape(-1)


@pytest.mark.parametrize("per_view_nms", [False, True], ids=["raw lists", "per-view NMS"])
def test_pipeline_merge_equals_the_restatement_and_feeds_cut_crops(per_view_nms):
    views, frames, k = mr.pipe_views(), mr.PIPE_FRAMES, mr.PIPE_K
    n = len(views)
    det = HipDetector(vr.model(), vr.H, vr.W, 3, max_batch=n, max_hits=vr.MAX_HITS)
    if per_view_nms:
        det.set_nms(capi.make_nms("maxg", overlap=0.8, ovrDnm="union"))                        # (mild: every view keeps many)
    E, _ = vr.stored_u8()
    x = dev(E)
    src = det.crop_source_tensor(x, layout="nhwc")
    dv, df = dev(views), dev(frames)
    det.run_view(src, dv, df, mr.PIPE_SAMPLES)
    det.synchronize()
    before = [tuple(a.tobytes() for a in det.detections(v)) for v in range(n)]
    lists = [det.detections(v)[0] for v in range(n)]
    assert all(len(l) > 0 for l in lists) and (per_view_nms or [len(l) for l in lists] == [len(l) for l in mr.pipe_oracle_lists()])
    dets, counts = mr.lists_to_arrays(lists, vr.MAX_HITS)
    for q, grow in ((None, 1.0), (mr.nms_of("max", **mr.PIPE_NMS), 1.0), (mr.nms_of("maxg", **mr.PIPE_NMS), 1.25)):
        rec, cnt, boxes, fidx, quads = det.merge_views(dv, df, 2, q, k, grow, quads=True)
        det.synchronize()
        want = list(mr.merge(dets, counts, views, frames, 2, q, k, grow, fill=0))
        got = [rec.cpu().numpy().view(capi.MERGED_DTYPE).reshape(2, k).copy(), cnt.cpu().numpy(), boxes.cpu().numpy(), fidx.cpu().numpy(), quads.cpu().numpy()]
        for f in range(2):                                                                    # record and quad slots beyond the count are undefined here
            m = max(min(int(want[1][f]), k), 0)
            got[0][f, m:], got[4][f, m:] = want[0][f, m:], want[4][f, m:]
        assert_bytes(got, want, (per_view_nms, q.type if q else 0))
        assert (got[1] > 0).all()
        for f in range(2):                                                                    # index points into the list get_detections returns
            for s in range(min(int(got[1][f]), k)):
                r = got[0][f, s]
                d = lists[r["view"]][r["index"]]
                assert frames[r["view"]] == f and d["score"].tobytes() == r["score"].tobytes() and d["scale"] == r["scale"]
                assert np.array_equal(HipDetector.view_box(views[r["view"]], [int(d[t]) for t in ("x", "y", "w", "h")]), np.array([r[t] for t in ("x", "y", "w", "h")], F))
        if q is None:
            continue
        # the device-only route to crops against the route of before
        crops = det.cut_crops(src, boxes.view(-1, 4), fidx.view(-1), (24, 20), samples=2)
        hb, hf = host_route(det, views, frames, 2, q, k, grow)
        assert np.array_equal(hb.view(np.uint32), got[2].reshape(-1, 4).view(np.uint32)) and np.array_equal(hf, got[3].reshape(-1))
        want_crops = det.cut_crops(src, hb, hf, (24, 20), samples=2)
        det.synchronize()
        gc, wc = crops.cpu().numpy(), want_crops.cpu().numpy()
        assert gc.tobytes() == wc.tobytes()
        for f in range(2):
            m = min(int(got[1][f]), k)
            assert gc[f * k:f * k + m].any() and not gc[f * k + m:(f + 1) * k].any()
    # nothing of the context changed
    assert [tuple(a.tobytes() for a in det.detections(v)) for v in range(n)] == before
    plain = det.crop_source_tensor(x[:, :vr.H, :vr.W, :], layout="nhwc")
    with pytest.raises(HipError) as e:
        det.cut_detections(plain, (16, 16), 2)
    assert e.value.code == capi.E_INVALID and "the last run was a view" in str(e.value)
    det.close()


# ---------------------------------------------------------------- 3. refusals, the profile name, a captured graph

def test_refusals_profile_name_and_a_graph_still_replays():
    import torch
    n = 3
    det = HipDetector(vr.model(), vr.H, vr.W, 3, max_batch=n, max_hits=vr.MAX_HITS)
    E, _ = vr.stored_u8()
    x = dev(E)
    src = det.crop_source_tensor(x, layout="nhwc")
    views, frames = dev(mr.pipe_views()[:n]), dev(mr.PIPE_FRAMES[:n])                           # (a few hundred detections a view)
    q = mr.nms_of("maxg", **mr.PIPE_NMS)

    def refused(*a, **kw):
        with pytest.raises(HipError) as e:
            det.merge_views(*a, **kw)
        return e.value.code
    assert refused(views, frames, 2, q) == capi.E_INVALID                                     # no run at all
    det.set_option("graph", 1)
    fr = torch.from_numpy(np.stack([synth.make_frame(sd, vr.H, vr.W, "luv") for sd in (40, 41, 42)])).cuda()
    for _ in range(3):                                                                        # plain, captured, replayed
        det.run(fr)
    det.synchronize()
    want = [tuple(a.tobytes() for a in det.detections(f)) for f in range(n)]
    assert refused(views, frames, 2, q) == capi.E_INVALID                                     # the last run was no view
    det.run_view(src, views, frames, mr.PIPE_SAMPLES)
    assert refused(views[:2], frames[:2], 2, q) == capi.E_INVALID                             # another n_views
    det.set_option("profile", 1)
    det.profile()
    rec, cnt, boxes, fidx = det.merge_views(views, frames, 2, q, 16)
    det.synchronize()
    names = det.profile()
    det.set_option("profile", 0)
    assert "k_merge_views" in names and "k_nms" not in names, names
    assert (cnt.cpu().numpy() > 0).all()
    det.run(fr)                                                                               # the captured graph, replayed
    det.synchronize()
    assert [tuple(a.tobytes() for a in det.detections(f)) for f in range(n)] == want and sum(len(w[0]) for w in want) > 0
    det.close()
    det = HipDetector(vr.model(), vr.H, vr.W, 3, max_batch=4, max_hits=vr.MAX_HITS, streams=2)
    with pytest.raises(HipError) as e:
        det.merge_views(views, frames, 2, q)
    assert e.value.code == capi.E_UNSUPPORTED
    det.close()


# ---------------------------------------------------------------- 4. the CLI prints the Python path's merged quads

def test_cli_merge_prints_the_python_paths_quads(tmp_path):
    import subprocess
    import torch
    import resized_entry_case as rc
    import yuv_desc_ref as ydr
    from acf_amd.modelio import write_model
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    from test_host_cpp import CLI, HOST, run
    subprocess.check_call(["make", "-s", "-C", HOST])
    Hs, Ws, cnt, h, w, smp, k = 150, 170, 2, vr.H, vr.W, 2, 40
    model = vr.model()
    write_model(str(tmp_path / "m.acfm"), model)
    d, fb = HipDetector.yuv_desc("nv12", Hs, Ws)
    buf = np.concatenate([ydr.pack("nv12", *rc.yuv_planes(80 + i, Hs, Ws, 1, 1)) for i in range(cnt)])
    (tmp_path / "f.yuv").write_bytes(buf.tobytes())
    specs = [((50, 40, 32, 24), 0.0, 0), ((120, 100, 128, 96), 6.0, 1), ((50, 40, 32, 24), 6.0, 0), ((50, 40, 32, 24), -6.0, 0)]
    args = ["--model", str(tmp_path / "m.acfm"), "--frames", str(tmp_path / "f.yuv"), "--yuv", "nv12", "--rows", str(Hs), "--cols", str(Ws), "--count", str(cnt), "--luv",
            "--view-size", "%dx%d" % (h, w), "--view-samples", str(smp), "--merge", "0.5:%d" % k, "--nms", "--max-count", "60", "--cut", "20x24", "--cut-prefix", str(tmp_path / "crop")]
    for box, deg, frame in specs:
        args += ["--view", "%g,%g,%g,%g,%g,%d" % (box + (deg, frame))]
    p = run(CLI, args)
    no_merge = [a for i, a in enumerate(args) if a != "--merge" and args[i - 1] != "--merge"]
    bad = run(CLI, no_merge, ok=False)                                                        # --cut with --view needs --merge: said, not ignored
    assert bad.returncode != 0 and "--merge" in bad.stderr and not bad.stdout.strip()
    said, cur, crops_said = [], None, []
    for ln in p.stdout.splitlines():
        t = ln.split()
        if t[0] == "frame":
            cur = []
            said.append((int(t[1]), int(t[2]), cur))
        elif t[0] == "crops":
            crops_said.append((int(t[1]), int(t[2])))
        else:
            cur.append(([float(v) for v in t[:8]], int(t[9], 16), int(t[10]), int(t[11])))
    assert [s[0] for s in said] == [0, 1]
    det = HipDetector(model, h, w, 3, max_batch=len(specs), max_hits=1 << 16)
    x = torch.from_numpy(buf).cuda()
    views = np.stack([HipDetector.view_from_box(box, deg * 3.14159265358979323846 / 180.0, h, w) for box, deg, _ in specs])
    frames = np.array([s[2] for s in specs], np.int32)
    # these frames give over a thousand raw detections a view, more than a stored frame's views may hold together: the per-view NMS
    # first (--nms --max-count 60: HipDetector's default pNms maxg / 0.65 / min + prune(60, 0), on the device)
    det.set_nms(capi.make_nms(type="maxg", overlap=0.65, ovrDnm="min", prune=True, maxCount=60, pruneRatio=0.0))
    src = det.crop_source_yuv(x, cnt, d, None, Hs, Ws, 0)
    det.run_view(src, views, frames, smp)
    # (the CLI's NMS across the views: maxg over the union, as --merge documents)
    rec, counts, boxes, fidx, quads = det.merge_views(views, frames, cnt, capi.make_nms("maxg", overlap=0.5, ovrDnm="union"), k, quads=True)
    crops = det.cut_crops(src, boxes.view(-1, 4), fidx.view(-1), (24, 20), dtype=torch.uint8, layout="packed").cpu().numpy()   # --cut 20x24: W x H
    det.synchronize()
    rec, counts, quads = rec.cpu().numpy().view(capi.MERGED_DTYPE).reshape(cnt, k), counts.cpu().numpy(), quads.cpu().numpy()
    for f in range(cnt):
        assert said[f][1] == counts[f] > 0 and len(said[f][2]) == min(int(counts[f]), k), (f, said[f][1], counts[f])
        for s, (got, score_bits, view, index) in enumerate(said[f][2]):
            assert np.array_equal(np.array(got, F), quads[f, s].ravel()), (f, s)               # %.9g round-trips a float32
            assert score_bits == int(rec[f, s:s + 1]["score"].view(np.uint32)[0]) and (view, index) == (rec[f, s]["view"], rec[f, s]["index"]), (f, s)
    # --cut: the crops of the merged boxes, written from mergeViews' device-side boxes through acf_hip_cut_crops
    assert crops_said == [(f, min(int(counts[f]), k)) for f in range(cnt)]
    for f, m in crops_said:
        for i in range(m):
            ppm = (tmp_path / ("crop_%d_%d.ppm" % (f, i))).read_bytes()
            assert ppm == b"P6\n20 24\n255\n" + crops[f * k + i].tobytes(), (f, i)
    assert len({v for _, _, v, _ in said[0][2]}) >= 2                                         # survivors of more than one view of frame 0
    det.close()
