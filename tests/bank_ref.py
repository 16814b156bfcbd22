"""A bank of classifiers on one pyramid (include/acf_hip.h: acf_hip_detect_bank / acf_hip_join_bank / acf_hip_op_join_bank; kernel
k_join_bank): the header's join rule restated in numpy, the designed cases and the pipeline case the CPU and GPU tests share.
Helper of tests/test_bank.py, tests/test_gpu_bank.py and tests/test_host_cpp_bank.py.

Boxes are ints and every product of the designed and pipeline cases stays far below 2^31, so k_nms's int arithmetic is exact in the f64
of merge_views_ref.suppress; the quotient o / u is one f64 division on both sides.  join() returns what acf_hip_op_join_bank leaves in
outputs that held the byte `fill` everywhere before the call."""
import functools

import numpy as np

import merge_views_ref as mr
from acf_amd import capi, synth

F = np.float32
CAP = capi.NMS_CAP
FILL = mr.FILL
NONE = mr.NONE
nms_of = mr.nms_of


def crop_box(d, det_scale, grow):
    """acf_hip_crop_box's f32 steps on an int box"""
    inv = F(1.0) if not det_scale else F(1.0) / F(det_scale)
    return mr.grown([F(int(d[t])) * inv for t in ("x", "y", "w", "h")], grow)


def concatenate(counts, max_hits, f):
    """Step 1 for frame f: counts [n_models][n_frames] -> [(model, index)] in concatenation order, or None: unknowable"""
    ent = []
    for m in range(len(counts)):
        c = int(counts[m][f])
        if c < 0 or c > max_hits:
            return None
        ent += [(m, i) for i in range(c)]
    return ent if len(ent) <= CAP else None


def survivors(ent, dets, f, q, separate):
    """Steps 2 and 3 on the concatenated entries of frame f -> positions in `ent`, in output order"""
    if q.type == 0:
        return list(range(len(ent)))
    boxes = [[int(dets[m, f, i][t]) for t in ("x", "y", "w", "h")] for m, i in ent]
    scores = [dets[m, f, i]["score"] for m, i in ent]
    if not separate:
        return mr.suppress(boxes, scores, q)[0]
    # only pairs of one model suppress each other: each model's survivors under the rule without prune, then the joint score order
    # (equal scores keep concatenation order) and the joint prune
    noprune = capi.NmsParams(q.type, q.ovrDnmUnion, q.overlap, q.thr, 0, q.maxCount, q.pruneRatio)
    keep = []
    for m in sorted({m for m, _ in ent}):
        pos = [p for p, e in enumerate(ent) if e[0] == m]
        keep += [pos[t] for t in mr.suppress([boxes[p] for p in pos], [scores[p] for p in pos], noprune)[0]]
    sc = np.asarray(scores, dtype=F).astype(np.float64)
    keep.sort(key=lambda p: (-sc[p], p))
    if q.prune and len(keep) > 1:
        cutoff, L = 1, min(q.maxCount, len(keep))
        for i in range(1, L):
            cutoff = i + 1
            if sc[keep[i]] < sc[keep[0]] * q.pruneRatio:
                break
        keep = keep[:cutoff]
    return keep


def join(dets, counts, nms=None, separate=0, k=8, grow=1.0, det_scale=None, fill=FILL):
    """dets DET_DTYPE [n_models][n_frames][max_hits], counts int32 [n_models][n_frames] -> (records BANK_DTYPE [nF][k], counts int32
    [nF], boxes float32 [nF][k][4], frame_index int32 [nF][k])"""
    q = NONE if nms is None else nms
    dets = np.asarray(dets)
    nM, nF, mh = dets.shape
    counts = np.asarray(counts, np.int32).reshape(nM, nF)
    rec = np.full((nF, k, 32), fill, np.uint8).view(capi.BANK_DTYPE).reshape(nF, k)
    cnt = np.full((nF, 4), fill, np.uint8).view(np.int32).reshape(nF)
    boxes = np.zeros((nF, k, 4), F)
    fidx = np.full((nF, k), -1, np.int32)
    for f in range(nF):
        ent = concatenate(counts, mh, f)
        if ent is None:
            cnt[f] = -1
            continue
        keep = survivors(ent, dets, f, q, separate)
        cnt[f] = len(keep)
        for s, p in enumerate(keep[:k]):
            m, i = ent[p]
            d = dets[m, f, i]
            rec[f, s] = (d["x"], d["y"], d["w"], d["h"], d["score"], d["scale"], m, i)
            boxes[f, s] = crop_box(d, det_scale, grow)
            fidx[f, s] = f
    return rec, cnt, boxes, fidx


# ---------------------------------------------------------------- the designed cases

def pack(models, max_hits=None):
    """[[[(x, y, w, h, score[, scale]), ...] per frame] per model] -> (dets [nM][nF][max_hits], counts [nM][nF])"""
    nM, nF = len(models), len(models[0])
    mh = max(1, max(len(l) for m in models for l in m)) if max_hits is None else max_hits
    dets = np.zeros((nM, nF, mh), dtype=capi.DET_DTYPE)
    for m, frames in enumerate(models):
        assert len(frames) == nF
        for f, l in enumerate(frames):
            for i, e in enumerate(l[:mh]):
                dets[m, f, i] = tuple(int(t) for t in e[:4]) + (F(e[4]), int(e[5]) if len(e) > 5 else m + i)
    return dets, np.array([[len(l) for l in frames] for frames in models], np.int32)


def one_frame(lists):
    return [[l] for l in lists]


TWIN = one_frame([[(10, 10, 20, 20, 2.0)], [(10, 10, 20, 20, 1.0)]])                       # the same box from two models
NINE = one_frame(mr.random_lists(9, [3, 0, 4, 2, 0, 5, 1, 3, 2], span=70))                  # nine models, two without a detection
EDGES = [mr.random_lists(21, [0, 4, 0, 5, 0], span=60), mr.random_lists(22, [3, 0, 0, 2, 4], span=60)]   # empty lists in front, in the middle, at the end
EDGES = [[EDGES[0][m], EDGES[1][m]] for m in range(5)]                                     # -> [model][frame]


def _case(models, max_hits=None, counts=None, **kw):
    dets, cnt = pack(models, max_hits)
    kw.setdefault("nms", nms_of())
    return dict(dets=dets, counts=cnt if counts is None else np.array(counts, np.int32).reshape(cnt.shape), **kw)


@functools.lru_cache(maxsize=None)
def cases():
    c = {}
    c["one model"] = _case(one_frame(mr.random_lists(1, [12], span=50)))
    c["one model, nothing"] = _case(one_frame([[]]))
    c["two models"] = _case(one_frame(mr.random_lists(2, [7, 9], span=50)), k=16)
    for sep in (0, 1):
        c["nine models, separate %d" % sep] = _case(NINE, separate=sep, k=24)
        c["empty lists at every place, two frames, separate %d" % sep] = _case(EDGES, separate=sep, k=12)
        c["the same box from two models, separate %d" % sep] = _case(TWIN, separate=sep, nms=nms_of(overlap=0.5))
        for typ in ("max", "maxg"):
            c["equal scores, %s, separate %d" % (typ, sep)] = _case(one_frame(mr.TIES), separate=sep, nms=nms_of(typ, overlap=0.3))
            c["chain, %s, separate %d" % (typ, sep)] = _case(one_frame(mr.CHAIN), separate=sep, nms=nms_of(typ, overlap=0.3))
    c["chain in one model, maxg"] = _case(one_frame([mr.CHAIN[0] + mr.CHAIN[1] + mr.CHAIN[2], []]), separate=1, nms=nms_of("maxg", overlap=0.3))
    for total in (64, 65, 129):                                                            # the thread-count fork
        c["total %d" % total] = _case(one_frame(mr.random_lists(total, mr.split(total, 3), span=110)), k=48)
    c["total 2048"] = _case(one_frame(mr.random_lists(2048, mr.split(2048, 8), span=250)), k=64)
    c["total 2048, separate"] = _case(one_frame(mr.random_lists(2048, mr.split(2048, 8), span=250)), k=64, separate=1)
    c["total 2049"] = _case(one_frame(mr.random_lists(2049, mr.split(2049, 8))), k=4)
    c["a list over max_hits"] = _case([[mr.FIVE[0], mr.FIVE[1]], [mr.FIVE[2], mr.FIVE[3]]], counts=[[3, 4], [2, 6]], max_hits=5)
    c["a count of -1"] = _case([[mr.FIVE[0], mr.FIVE[1]], [mr.FIVE[2], mr.FIVE[3]]], counts=[[-1, 4], [2, 5]])
    c["K 1 below the survivors"] = _case(one_frame(mr.APART), k=1)
    c["K above the survivors"] = _case(one_frame(mr.APART), k=9)
    c["thr removes a whole model"] = _case(one_frame(mr.APART), nms=nms_of(thr=3.5))          # model 2's only score is 3.0
    c["thr removes model 1 and model 2"] = _case(one_frame(mr.APART), nms=nms_of(thr=9.0))
    c["thr drops everything"] = _case(one_frame(mr.APART), nms=nms_of(thr=1e9))
    c["prune maxCount 0"] = _case(one_frame(mr.APART), nms=nms_of(prune=True, maxCount=0, pruneRatio=0.0))
    c["prune maxCount 3"] = _case(one_frame(mr.APART), nms=nms_of(prune=True, maxCount=3, pruneRatio=0.0))
    c["prune maxCount 3, separate"] = _case(one_frame(mr.APART), separate=1, nms=nms_of(prune=True, maxCount=3, pruneRatio=0.0))
    c["prune: one past the first below the ratio"] = _case(one_frame(mr.APART), nms=nms_of(prune=True, maxCount=10, pruneRatio=0.5))
    c["type 0"] = _case(EDGES, nms=NONE, k=6)
    c["type 0, separate, prune and thr ignored"] = _case(one_frame(mr.APART), separate=1, nms=capi.make_nms("none", thr=1e9, prune=True, maxCount=1))
    c["grow 1.5, det_scale 0.5"] = _case(EDGES, grow=1.5, det_scale=0.5, k=12)
    c["det_scale 1.37"] = _case(NINE, det_scale=1.37, k=24)
    return c


@functools.lru_cache(maxsize=None)
def expected(name):
    return join(**cases()[name])


BAD_SPECS = (dict(k=0), dict(k=CAP + 1), dict(grow=0.0), dict(grow=float("nan")), dict(grow=float("inf")), dict(reserved=1),
             dict(nms=capi.make_nms("maxg", overlap=float("nan"))), dict(nms=capi.NmsParams(3, 0, 0.5, 0.0, 0, 0, 0.0)),
             dict(nms=capi.NmsParams(-1, 0, 0.5, 0.0, 0, 0, 0.0)), dict(nms=capi.make_nms("maxg", prune=True, maxCount=-1)),
             dict(separate=2), dict(separate=-1), dict(det_scale=-1.0), dict(det_scale=float("nan")), dict(det_scale=float("inf")))


def spec_of(nms=None, separate=0, k=8, grow=1.0, det_scale=0.0, reserved=0):
    s = capi.BankSpec()
    s.nms = nms if nms is not None else nms_of()
    s.separate, s.max_per_frame, s.grow, s.det_scale = separate, k, grow, det_scale
    s.reserved[1] = reserved
    return s


# ---------------------------------------------------------------- the pipeline case

H, W, D = 96, 128, 3
MAX_HITS = 4096
FRAME_SEEDS = (40, 41)
MODEL_ARGS = (
    ("primary", dict(seed=3, nTrees=96, cascThr=-2.0)),
    ("tall", dict(seed=5, nTrees=96, cascThr=-1.5, modelDs_h=28, modelDs_w=12, modelDsPad_h=32, modelDsPad_w=16)),
    ("walk", dict(seed=6, nTrees=96, cascThr=-1.5, treeDepth=0, modelDs_h=24, modelDs_w=24, modelDsPad_h=24, modelDsPad_w=24, stride=8)),
    ("deep", dict(seed=7, nTrees=40, cascThr=-1.5, treeDepth=3, stride=2)),
    ("wide", dict(seed=8, nTrees=160, cascThr=-2.0, modelDs_h=16, modelDs_w=40, modelDsPad_h=24, modelDsPad_w=48)),
)
NAMES = tuple(n for n, _ in MODEL_ARGS)
RAW_COUNTS = ((192, 319), (216, 42), (46, 76), (246, 80), (15, 112))                       # [model][frame], from the CPU oracle
JOINT_KEPT = {("maxg", "union", 0.5): ((154, 128), (181, 149)), ("max", "min", 0.65): ((21, 20), (56, 51))}   # (joint, separate) per frame


@functools.lru_cache(maxsize=None)
def models():
    return tuple(synth.make_model(name="TINY", **kw) for _, kw in MODEL_ARGS)


@functools.lru_cache(maxsize=None)
def frames(seeds=FRAME_SEEDS):
    return np.stack([synth.make_frame(s, H, W, "luv") for s in seeds])


@functools.lru_cache(maxsize=None)
def oracle_lists(seeds=FRAME_SEEDS):
    """[model][frame] -> (detections, hits) of the CPU oracle: every model's plan on the PRIMARY's pyramid of the frame"""
    from oracle import binding as ob
    plans = [ob.Plan(m, H, W, D) for m in models()]
    out = [[] for _ in plans]
    for fr in frames(seeds):
        pyr, _, _ = ob.chns_pyramid(plans[0], fr)
        for m, plan in enumerate(plans):
            out[m].append(ob.detect(plan, pyr))
    return out


def lists_to_arrays(lists, max_hits):
    """[model][frame] arrays of DET_DTYPE -> (dets [nM][nF][max_hits], counts [nM][nF])"""
    nM, nF = len(lists), len(lists[0])
    dets = np.zeros((nM, nF, max_hits), dtype=capi.DET_DTYPE)
    for m in range(nM):
        for f in range(nF):
            dets[m, f, :len(lists[m][f])] = lists[m][f][:max_hits]
    return dets, np.array([[len(lists[m][f]) for f in range(nF)] for m in range(nM)], np.int32)
