"""The views' detections merged into their stored frames, without a GPU (include/acf_hip.h: "merging the views' detections into the
stored frame"): the declarations and the refusals that need no device, the numpy restatement (tests/merge_views_ref.py) against the
pinned CPU oracle's bbNms for integer-translation views, and the conditions of the designed cases and of the pipeline case which the
GPU test (tests/test_gpu_merge_views.py) relies on, so that none of them is vacuous."""
import ctypes as C
import fnmatch
import os
import re

import numpy as np
import pytest

import merge_views_ref as mr
import view_ref as vr
from acf_amd import capi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F = np.float32
ENTRIES = ["acf_hip_merge_views", "acf_hip_op_merge_views"]


def test_declarations_sizes_and_the_abi_stays_9():
    text = open(os.path.join(ROOT, "include", "acf_hip.h")).read()
    assert re.search(r"#define ACF_HIP_ABI_VERSION 9\b", text)
    lib = capi.load()
    assert lib.acf_hip_abi_version() == 9
    patterns = re.findall(r"global:\s*([^;]+);", open(os.path.join(ROOT, "acf_amd", "csrc", "exports.map")).read())
    for name in ENTRIES:
        assert re.search(r"ACF_HIP_API int %s\(" % name, text), name
        assert name in capi.DECLARED_SYMBOLS and getattr(lib, name).argtypes is not None
        assert any(fnmatch.fnmatch(name, p.strip()) for p in patterns), name
    for struct in ("acf_hip_merged_detection", "acf_hip_merge_spec"):
        assert re.search(r"typedef struct %s\b" % struct, text), struct
    assert C.sizeof(capi.MergedDetection) == 32 and capi.MERGED_DTYPE.itemsize == 32
    assert [capi.MERGED_DTYPE.fields[n][1] for n in capi.MERGED_DTYPE.names] == [getattr(capi.MergedDetection, n).offset for n in capi.MERGED_DTYPE.names]
    assert C.sizeof(capi.MergeSpec) == C.sizeof(capi.NmsParams) + 16 == 56
    assert capi.MergeSpec.max_per_frame.offset == 40 and capi.MergeSpec.grow.offset == 44 and capi.MergeSpec.reserved.offset == 48


def spec_of(k=4, grow=1.0, typ=2, reserved=(0, 0), overlap=0.5, prune=0, maxCount=0):
    s = capi.MergeSpec()
    s.nms = capi.NmsParams(typ, 1, overlap, -1e300, prune, maxCount, 0.0)
    s.max_per_frame, s.grow = k, grow
    s.reserved[0], s.reserved[1] = reserved
    return s


BAD_SPECS = [dict(k=0), dict(k=capi.NMS_CAP + 1), dict(grow=0.0), dict(grow=-1.0), dict(grow=float("inf")), dict(grow=float("nan")), dict(typ=-1), dict(typ=3),
             dict(reserved=(1, 0)), dict(reserved=(0, 1)), dict(overlap=float("nan")), dict(prune=1, maxCount=-1)]


def test_refusals_that_need_no_device():
    """a null context with good and with bad arguments: ACF_HIP_E_INVALID before anything touches a device"""
    lib = capi.load()
    p = C.c_void_p(256)                                                                       # never dereferenced
    good = spec_of()
    pipe = lambda views=p, frames=None, n=2, nf=1, spec=good, out=p, cnt=p: lib.acf_hip_merge_views(None, views, frames, n, nf, C.byref(spec) if spec else None, out, cnt,
                                                                                                    None, None, None)
    op = lambda dets=p, counts=p, mh=4, views=p, n=2, nf=1, spec=good, out=p, cnt=p: lib.acf_hip_op_merge_views(None, dets, counts, mh, views, None, n, nf,
                                                                                                                 C.byref(spec) if spec else None, out, cnt, None, None, None)
    for fn in (pipe, op):
        assert fn() == capi.E_INVALID                                                         # no context
        for kw in (dict(views=None), dict(out=None), dict(cnt=None), dict(spec=None), dict(n=0), dict(n=-1), dict(n=capi.MERGE_VIEWS_MAX + 1), dict(nf=0), dict(nf=-3)):
            assert fn(**kw) == capi.E_INVALID, kw
        for kw in BAD_SPECS:
            assert fn(spec=spec_of(**kw)) == capi.E_INVALID, kw
    for kw in (dict(dets=None), dict(counts=None), dict(mh=0)):
        assert op(**kw) == capi.E_INVALID, kw


# ---------------------------------------------------------------- the restatement against the pinned oracle

def test_restatement_equals_the_oracles_bbnms_for_integer_translations(oracle):
    r = np.random.RandomState(5)
    checked = suppressed = pruned = 0
    for trial in range(240):
        nv = int(r.randint(1, 6))
        sizes = [int(r.randint(0, 9)) for _ in range(nv)]
        lists = mr.random_lists(1000 + trial, sizes, span=40)
        if trial % 3 == 0:                                                                    # ties, across and within views
            lists = [[e[:4] + (float(int(e[4]) % 3),) for e in l] for l in lists]
        dets, counts = mr.pack(lists)
        shifts = [(int(r.randint(-20, 20)), int(r.randint(-20, 20))) for _ in range(nv)]
        views = np.stack([vr.translation(tx, ty) for tx, ty in shifts])
        typ, ovr = ("max", "maxg")[trial % 2], ("union", "min")[(trial // 2) % 2]
        q = mr.nms_of(typ, ovr, overlap=(0.2, 0.5, 0.65)[trial % 3], thr=(-1e300, 0.0)[(trial // 4) % 2], prune=trial % 5 < 2, maxCount=int(r.randint(0, 8)),
                      pruneRatio=(0.0, 0.5)[(trial // 5) % 2])
        total = sum(sizes)
        rec, cnt, _, _, _ = mr.merge(dets, counts, views, frames=[0] * nv, n_frames=1, nms=q, k=max(total, 1))
        flat = [(v, i) for v in range(nv) for i in range(sizes[v])]
        boxes = np.array([[dets[v, i]["x"] + shifts[v][0], dets[v, i]["y"] + shifts[v][1], dets[v, i]["w"], dets[v, i]["h"]] for v, i in flat], np.int32).reshape(-1, 4)
        scores = np.array([dets[v, i]["score"] for v, i in flat], np.float64)
        keep = oracle.nms(boxes, scores, q)
        assert cnt[0] == len(keep), (trial, cnt[0], len(keep))
        got = [(int(rec[0, s]["view"]), int(rec[0, s]["index"])) for s in range(cnt[0])]
        assert got == [flat[t] for t in keep], trial
        for s, t in enumerate(keep):                                                          # ... and the mapped box is the translated int box
            assert [rec[0, s][n] for n in ("x", "y", "w", "h")] == [F(v) for v in boxes[t]], trial
        checked += 1
        suppressed += total - len(keep)
        pruned += bool(q.prune)
    assert checked == 240 and suppressed > 200 and pruned > 50


# ---------------------------------------------------------------- the designed cases are what they claim to be

def detail_of(name, **over):
    d = []
    mr.merge(**dict(mr.cases()[name], **over), detail=d)
    return d


def total_of(name):
    c = mr.cases()[name]
    return int(c["counts"].sum())


def test_count_cases_sum_to_what_they_say():
    for n in (0, 1, 64, 65, 128, 129, 2048, 2049):
        assert total_of("total %d" % n) == n
    assert mr.expected("total 2048")[1][0] > 64 and mr.expected("total 2049")[1][0] == -1      # (more survivors than K, too)
    assert mr.expected("total 0")[1][0] == 0 and mr.expected("total 1")[1][0] == 1
    for n in (65, 128, 129):
        assert 0 < mr.expected("total %d" % n)[1][0] < n                                      # something is suppressed


def test_many_view_cases_reach_past_the_first_wave():
    for nv in mr.MANY:
        c = mr.cases()["%d views" % nv]
        assert len(c["views"]) == nv > 128 and (c["counts"] == 0).sum() >= nv // 4 and (c["counts"][64:] > 0).sum() > 32
        assert 0 < int(c["counts"].sum()) <= capi.NMS_CAP and -1 in c["frames"]
        rec, cnt = mr.expected("%d views" % nv)[:2]
        assert (cnt > 0).all() and max(int(r["view"]) for f in range(3) for r in rec[f, :min(int(cnt[f]), 40)]) >= 64
    assert mr.MANY[-1] == capi.MERGE_VIEWS_MAX


def test_threshold_pair_sits_on_the_parameter_bit_for_bit():
    for ovr in ("union", "min"):
        c = mr.cases()["at the threshold, " + ovr]
        b = [vr.box(c["views"][v], [c["dets"][v, 0][t] for t in ("x", "y", "w", "h")]).astype(np.float64) for v in (0, 1)]
        assert [list(x) for x in b] == [[0, 0, 10, 10], [5, 0, 10, 10]]
        iw = min(b[0][0] + b[0][2], b[1][0] + b[1][2]) - max(b[0][0], b[1][0])
        ih = min(b[0][1] + b[0][3], b[1][1] + b[1][3]) - max(b[0][1], b[1][1])
        o = iw * ih
        u = (b[0][2] * b[0][3] + b[1][2] * b[1][3]) - o if ovr == "union" else min(b[0][2] * b[0][3], b[1][2] * b[1][3])
        ratio = np.float64(o / u)
        assert ratio.view(np.uint64) == np.float64(c["nms"].overlap).view(np.uint64)
        under = mr.cases()["an ulp under the threshold, " + ovr]["nms"].overlap
        assert np.float64(under).view(np.uint64) + 1 == ratio.view(np.uint64)
        assert mr.expected("at the threshold, " + ovr)[1][0] == 2 and mr.expected("an ulp under the threshold, " + ovr)[1][0] == 1


def test_tie_and_chain_cases():
    for typ in ("max", "maxg"):
        c = mr.cases()["equal scores, " + typ]
        sc = [c["dets"][v, i]["score"] for v in range(3) for i in range(c["counts"][v])]
        assert len(set(sc)) == 1 and len(sc) == 7
        rec, cnt = mr.expected("equal scores, " + typ)[:2]
        order = [(int(rec[0, s]["view"]), int(rec[0, s]["index"])) for s in range(cnt[0])]
        assert order == sorted(order) and 0 < cnt[0] < 7                                      # view, then index; and ties do suppress
    keep = {typ: [tuple(int(x) for x in (r["view"], r["index"])) for r in mr.expected("chain, " + typ)[0][0][:mr.expected("chain, " + typ)[1][0]]] for typ in ("max", "maxg")}
    assert keep["max"] == [(0, 0)] and keep["maxg"] == [(0, 0), (2, 0)]
    by = detail_of("chain, max")[0][2]
    assert by == {(1, 0): (0, 0), (2, 0): (1, 0)}                                             # A suppresses B, B suppresses C, A does not


def test_prune_thr_k_and_view_cases():
    n = lambda name: int(mr.expected(name)[1][0])
    unpruned = n("K above the survivors")
    assert unpruned == 5
    c = mr.cases()["prune: one past the first below the ratio"]
    sc = sorted((float(c["dets"][v, i]["score"]) for v in range(3) for i in range(c["counts"][v])), reverse=True)
    first_below = next(i for i, s in enumerate(sc) if s < sc[0] * c["nms"].pruneRatio)
    assert n("prune: one past the first below the ratio") == first_below + 1 < unpruned
    assert n("prune: maxCount below the survivors") == 2 and n("prune: maxCount 1") == 1 and n("prune: one survivor") == 1
    assert n("thr drops everything") == 0 and 0 < n("thr drops some") < unpruned
    assert n("K below the survivors") == 5 > mr.cases()["K below the survivors"]["k"]
    assert n("type 0, prune and thr ignored") == 5
    # the odd views: the zero and the NaN view lose all their entries, the mirroring and the tilted view keep theirs
    ok = detail_of("zero, NaN, mirroring and tilted views, type 0")[0][0]
    c = mr.cases()["zero, NaN, mirroring and tilted views"]
    assert {v for v, _ in ok} == {2, 3} and len(ok) == int(c["counts"][2] + c["counts"][3]) and c["counts"][0] > 0 and c["counts"][1] > 0
    m = c["views"][2]
    assert m[0] * m[4] - m[1] * m[3] < 0                                                      # (it mirrors)
    # grow: 1.5 changes the boxes and nothing else
    a, b = mr.expected("grow 1.5"), mr.merge(**dict(mr.cases()["grow 1.5"], grow=1.0))
    assert a[0].tobytes() == b[0].tobytes() and not np.array_equal(a[2], b[2])
    # frames: the bad counts make their own frame unknowable only; views of no frame contribute nothing
    assert list(mr.expected("a count of -1")[1]) == [5, -1] and list(mr.expected("a count of max_hits + 1")[1]) == [5, -1]
    assert list(mr.expected("a bad count in no frame")[1]) == [5, 5]
    assert list(mr.expected("frame index -1 and n_frames")[1]) == [8, 0]
    assert list(mr.expected("frame_dev NULL, three frames")[1]) == list(mr.expected("frame_dev NULL, five frames")[1][:3])


def test_unwritten_slots_keep_the_sentinel_and_the_rest_is_zeros_and_minus_one():
    for name in mr.cases():
        rec, cnt, boxes, fidx, quads = mr.expected(name)
        k = rec.shape[1]
        for f in range(len(cnt)):
            n = max(min(int(cnt[f]), k), 0)
            assert (rec[f, n:].view(np.uint8) == mr.FILL).all() and (quads[f, n:].view(np.uint8) == mr.FILL).all(), name
            assert not boxes[f, n:].view(np.uint32).any() and (fidx[f, n:] == -1).all() and (fidx[f, :n] == f).all(), name


# ---------------------------------------------------------------- the precondition of the pipeline case

def test_pipeline_case_merges_across_views(oracle):
    lists = mr.pipe_oracle_lists()
    frames = mr.PIPE_FRAMES
    assert sorted(set(frames.tolist())) == [0, 1] and (frames == 0).sum() == len(mr.PIPE_ANGLES) and (frames == 1).sum() == 2
    assert frames.tolist() != sorted(frames.tolist())                                         # interleaved
    for f in (0, 1):
        assert 0 < sum(len(l) for l, g in zip(lists, frames) if g == f) < capi.NMS_CAP
    assert all(0 < len(l) <= vr.MAX_HITS for l in lists)
    dets, counts = mr.lists_to_arrays(lists, vr.MAX_HITS)
    for typ in ("max", "maxg"):
        d = []
        rec, cnt, _, _, _ = mr.merge(dets, counts, mr.pipe_views(), frames, 2, mr.nms_of(typ, **mr.PIPE_NMS), mr.PIPE_K, detail=d)
        ok, keep, by = d[0]
        assert sum(1 for j, i in by.items() if j[0] != i[0]) > 0                              # a detection suppressed by one of ANOTHER view
        assert len({v for v, _ in keep}) >= 2 and all(frames[v] == 0 for v, _ in keep)
        assert 0 < cnt[0] < len(ok) and 0 < cnt[1]
