"""The views' detections merged into their stored frames (include/acf_hip.h: acf_hip_merge_views / acf_hip_op_merge_views; kernel
k_merge_views): the header's rule restated in numpy, the designed cases and the pipeline case the CPU and GPU tests share.
Helper of tests/test_merge_views.py and tests/test_gpu_merge_views.py.

Every f64 / f32 operation is rounded once (numpy's and Python's arithmetic is exactly that), so the GPU tests compare raw bytes.
merge() returns what acf_hip_op_merge_views leaves in outputs that held the byte `fill` everywhere before the call."""
import functools

import numpy as np

import view_ref as vr
from acf_amd import capi

F = np.float32
CAP = capi.NMS_CAP
FILL = 0xA5                       # the sentinel byte the tests pre-fill the outputs with
NONE = capi.make_nms("none")


def nms_of(type="maxg", ovr="union", overlap=0.5, thr=-1.7976931348623157e308, prune=False, maxCount=10, pruneRatio=0.0):
    return capi.make_nms(type=type, overlap=overlap, ovrDnm=ovr, thr=thr, prune=prune, maxCount=maxCount, pruneRatio=pruneRatio)


def pack(lists, max_hits=None):
    """[[(x, y, w, h, score[, scale]), ...] per view] -> (dets DET_DTYPE [n_views][max_hits], counts int32 [n_views])"""
    mh = max(1, max(len(l) for l in lists)) if max_hits is None else max_hits
    dets = np.zeros((len(lists), mh), dtype=capi.DET_DTYPE)
    for v, l in enumerate(lists):
        for i, e in enumerate(l):
            dets[v, i] = tuple(int(t) for t in e[:4]) + (F(e[4]), int(e[5]) if len(e) > 5 else v + i)
    return dets, np.array([len(l) for l in lists], np.int32)


def grown(b, grow):
    """acf_hip_crop_box's f32 steps on a float box"""
    b, g = np.asarray(b, dtype=F), F(grow)
    with np.errstate(all="ignore"):
        cx, cy = b[0] + b[2] * F(0.5), b[1] + b[3] * F(0.5)
        w2, h2 = b[2] * g, b[3] * g
        out = np.array([cx - w2 * F(0.5), cy - h2 * F(0.5), w2, h2])
    assert out.dtype == F
    return out


def suppress(boxes, scores, q):
    """Steps 4 of the rule on float32 boxes [n][4] and float32 scores [n] in concatenation order -> (survivors in output order,
    {suppressed entry: the entry that suppressed it})"""
    sc = np.asarray(scores, dtype=F).astype(np.float64)
    b = np.asarray(boxes, dtype=F).astype(np.float64).reshape(-1, 4)
    order = [i for i in range(len(sc)) if not sc[i] < q.thr]
    order.sort(key=lambda i: -sc[i])                                                      # stable: equal scores keep concatenation order
    o = np.array(order, dtype=np.int64)
    xs, ys = b[o, 0], b[o, 1]
    xe, ye, area = xs + b[o, 2], ys + b[o, 3], b[o, 2] * b[o, 3]
    kp, by = np.ones(len(o), bool), {}
    for i in range(len(o)):
        if q.type == 2 and not kp[i]:
            continue
        j = np.arange(i + 1, len(o))
        iw = np.minimum(xe[i], xe[j]) - np.maximum(xs[i], xs[j])
        ih = np.minimum(ye[i], ye[j]) - np.maximum(ys[i], ys[j])
        with np.errstate(all="ignore"):
            ov = iw * ih
            u = (area[i] + area[j]) - ov if q.ovrDnmUnion else np.minimum(area[i], area[j])
            hit = kp[j] & (iw > 0) & (ih > 0) & (ov / u > q.overlap)
        for t in j[hit]:
            by[order[t]] = order[i]
        kp[j[hit]] = False
    keep = [order[i] for i in range(len(o)) if kp[i]]
    if q.prune and len(keep) > 1:                                                         # ObjectDetector.cpp:30-42
        cutoff, L = 1, min(q.maxCount, len(keep))
        for i in range(1, L):
            cutoff = i + 1
            if sc[keep[i]] < sc[keep[0]] * q.pruneRatio:
                break
        keep = keep[:cutoff]
    return keep, by


def concatenate(counts, max_hits, frames, n_views, f):
    """Step 1 for stored frame f -> [(view, index)] in concatenation order, or None: unknowable"""
    ent = []
    for v in range(n_views):
        if (v if frames is None else int(frames[v])) != f:
            continue
        c = int(counts[v])
        if c < 0 or c > max_hits:
            return None
        ent += [(v, i) for i in range(c)]
    return ent if len(ent) <= CAP else None


def merge(dets, counts, views, frames=None, n_frames=None, nms=None, k=8, grow=1.0, fill=FILL, detail=None):
    """-> (records MERGED_DTYPE [nF][k], counts int32 [nF], boxes float32 [nF][k][4], frame_index int32 [nF][k], quads float32
    [nF][k][4][2]).  detail: a list that receives, per stored frame, (entries after step 2, survivors, suppressed-by map) as
    (view, index) pairs."""
    q = NONE if nms is None else nms
    views = np.asarray(views, dtype=F).reshape(-1, 6)
    n, nF = len(views), len(views) if n_frames is None else n_frames
    dets = np.asarray(dets).reshape(n, -1)
    rec = np.full((nF, k, 32), fill, np.uint8).view(capi.MERGED_DTYPE).reshape(nF, k)
    cnt = np.full((nF, 4), fill, np.uint8).view(np.int32).reshape(nF)
    boxes = np.zeros((nF, k, 4), F)
    fidx = np.full((nF, k), -1, np.int32)
    quads = np.full((nF, k, 32), fill, np.uint8).view(F).reshape(nF, k, 4, 2)
    for f in range(nF):
        ent = concatenate(counts, dets.shape[1], frames, n, f)
        if ent is None:
            cnt[f] = -1
            if detail is not None:
                detail.append(None)
            continue
        with np.errstate(all="ignore"):
            bx = [vr.box(views[v], [dets[v, i][t] for t in ("x", "y", "w", "h")]) for v, i in ent]
        ok = [e for e, b in zip(ent, bx) if np.isfinite(b).all() and b[2] > 0 and b[3] > 0]
        bmap = {e: b for e, b in zip(ent, bx)}
        if q.type == 0:
            keep, by = list(range(len(ok))), {}
        else:
            keep, by = suppress([bmap[e] for e in ok], [dets[v, i]["score"] for v, i in ok], q)
        cnt[f] = len(keep)
        for s, t in enumerate(keep[:k]):
            v, i = ok[t]
            d, b = dets[v, i], bmap[ok[t]]
            rec[f, s] = (b[0], b[1], b[2], b[3], d["score"], v, i, d["scale"])
            quads[f, s] = vr.quad(views[v], [d[t2] for t2 in ("x", "y", "w", "h")]).astype(F)
            boxes[f, s] = grown(b, grow)
            fidx[f, s] = f
        if detail is not None:
            detail.append((ok, [ok[t] for t in keep], {ok[j]: ok[i] for j, i in by.items()}))
    return rec, cnt, boxes, fidx, quads


# ---------------------------------------------------------------- the designed cases

def random_lists(seed, sizes, span=400):
    """lists of random int boxes with distinct float32 scores"""
    r = np.random.RandomState(seed)
    total = sum(sizes)
    scores = (r.permutation(total).astype(F) * F(0.125) - F(7)).tolist()
    out, at = [], 0
    for n in sizes:
        out.append([(int(r.randint(0, span)), int(r.randint(0, span)), int(r.randint(8, 40)), int(r.randint(8, 40)), scores[at + i]) for i in range(n)])
        at += n
    return out


def shifts(n):
    """n integer-translation views"""
    return np.stack([vr.translation(3 * i, 2 * i + 1) for i in range(n)])


def split(total, n):
    return [total // n + (1 if i < total % n else 0) for i in range(n)]


PAIR = [[(0, 0, 10, 10, 2.0)], [(0, 0, 10, 10, 1.0)]]                                     # in U: (0, 0, 10, 10) and (5, 0, 10, 10)
PAIR_VIEWS = np.stack([vr.translation(0, 0), vr.translation(5, 0)])
PAIR_RATIO = {"union": 50.0 / 150.0, "min": 50.0 / 100.0}
CHAIN = [[(0, 0, 10, 10, 3.0)], [(4, 0, 10, 10, 2.0)], [(8, 0, 10, 10, 1.0)]]              # A suppresses B, B would suppress C, A does not
CHAIN_VIEWS = np.tile(vr.IDENTITY, (3, 1))
APART = [[(0, 0, 10, 10, 10.0), (20, 0, 10, 10, 4.0)], [(40, 0, 10, 10, 8.0), (60, 0, 10, 10, 2.0)], [(80, 0, 10, 10, 3.0)]]   # no two overlap
TIES = [[(0, 0, 10, 10, 1.0), (30, 0, 10, 10, 1.0), (2, 0, 10, 10, 1.0)], [(31, 1, 10, 10, 1.0), (60, 0, 10, 10, 1.0)], [(61, 0, 10, 10, 1.0), (0, 30, 9, 9, 1.0)]]
FIVE = random_lists(11, [3, 4, 2, 5, 3], span=60)
ODD_VIEWS = np.stack([np.zeros(6, F), np.full(6, np.nan, F), vr.VIEWS["mirror and shear, s 1"][0], vr.from_box((10, 10, 150, 112.5), vr.deg(20), vr.H, vr.W)])


MANY = (170, 1024)


def many_views(nv):
    """nv views of 0 .. 3 boxes each (every fourth view empty), integer translations -> (lists, views)"""
    sizes = [0 if i % 4 == 1 else 1 + (i * 7) % 3 for i in range(nv)]
    return random_lists(nv, sizes, span=150), np.stack([vr.translation(i % 17, (3 * i) % 13) for i in range(nv)])


def _case(lists, views=None, max_hits=None, counts=None, **kw):
    dets, cnt = pack(lists, max_hits)
    kw.setdefault("nms", nms_of())
    return dict(dets=dets, counts=cnt if counts is None else np.array(counts, np.int32), views=shifts(len(lists)) if views is None else views, **kw)


@functools.lru_cache(maxsize=None)
def cases():
    c = {}
    c["total 0"] = _case([[], [], []], n_frames=1, frames=[0, 0, 0])
    c["total 1"] = _case([[], [(5, 6, 20, 30, 1.5)], []], n_frames=1, frames=[0, 0, 0])
    for total in (64, 65, 128, 129):                                                      # the thread-count fork
        c["total %d" % total] = _case(random_lists(total, split(total, 3), span=110), n_frames=1, frames=[0] * 3, k=48)
    c["total 2048"] = _case(random_lists(2048, split(2048, 8), span=250), n_frames=1, frames=[0] * 8, k=64)
    c["total 2049"] = _case(random_lists(2049, split(2049, 8)), n_frames=1, frames=[0] * 8, k=4)
    c["two frames interleaved"] = _case(FIVE, frames=[1, 0, 1, 0, 1], n_frames=2)
    c["frame_dev NULL, five frames"] = _case(FIVE, n_frames=5)
    c["frame_dev NULL, three frames"] = _case(FIVE, n_frames=3)
    c["frame index -1 and n_frames"] = _case(FIVE[:4], frames=[0, -1, 2, 0], n_frames=2)
    c["a count of -1"] = _case(FIVE[:4], frames=[0, 1, 0, 1], n_frames=2, counts=[3, -1, 2, 5])
    c["a count of max_hits + 1"] = _case(FIVE[:4], frames=[0, 1, 0, 1], n_frames=2, counts=[3, 4, 2, 6], max_hits=5)
    c["a bad count in no frame"] = _case(FIVE[:4], frames=[0, 7, 0, 1], n_frames=2, counts=[3, -1, 2, 5])
    for typ in ("max", "maxg"):
        c["equal scores, " + typ] = _case(TIES, frames=[0, 0, 0], n_frames=1, nms=nms_of(typ, overlap=0.3))
        c["chain, " + typ] = _case(CHAIN, views=CHAIN_VIEWS, frames=[0, 0, 0], n_frames=1, nms=nms_of(typ, overlap=0.3))
    for ovr in ("union", "min"):
        c["at the threshold, " + ovr] = _case(PAIR, views=PAIR_VIEWS, frames=[0, 0], n_frames=1, nms=nms_of(ovr=ovr, overlap=PAIR_RATIO[ovr]))
        c["an ulp under the threshold, " + ovr] = _case(PAIR, views=PAIR_VIEWS, frames=[0, 0], n_frames=1,
                                                        nms=nms_of(ovr=ovr, overlap=float(np.nextafter(PAIR_RATIO[ovr], 0.0))))
    c["prune: one past the first below the ratio"] = _case(APART, frames=[0, 0, 0], n_frames=1, nms=nms_of(prune=True, maxCount=10, pruneRatio=0.5))
    c["prune: maxCount below the survivors"] = _case(APART, frames=[0, 0, 0], n_frames=1, nms=nms_of(prune=True, maxCount=2, pruneRatio=0.0))
    c["prune: maxCount 1"] = _case(APART, frames=[0, 0, 0], n_frames=1, nms=nms_of(prune=True, maxCount=1, pruneRatio=0.0))
    c["prune: one survivor"] = _case([[], [(5, 6, 20, 30, 1.5)]], frames=[0, 0], n_frames=1, nms=nms_of(prune=True, maxCount=10, pruneRatio=0.5))
    c["thr drops everything"] = _case(APART, frames=[0, 0, 0], n_frames=1, nms=nms_of(thr=1e9))
    c["thr drops some"] = _case(APART, frames=[0, 0, 0], n_frames=1, nms=nms_of(thr=3.5))
    c["K below the survivors"] = _case(APART, frames=[0, 0, 0], n_frames=1, k=2)
    c["K above the survivors"] = _case(APART, frames=[0, 0, 0], n_frames=1, k=9)
    c["zero, NaN, mirroring and tilted views"] = _case(FIVE[:4], views=ODD_VIEWS, frames=[0, 0, 0, 0], n_frames=1)
    c["zero, NaN, mirroring and tilted views, type 0"] = _case(FIVE[:4], views=ODD_VIEWS, frames=[0, 0, 0, 0], n_frames=1, nms=NONE)
    c["grow 1.5"] = _case(FIVE, frames=[1, 0, 1, 0, 1], n_frames=2, grow=1.5, views=np.stack([ODD_VIEWS[3], ODD_VIEWS[2]] + list(shifts(3))))
    c["type 0"] = _case(FIVE, frames=[1, 0, 1, 0, 1], n_frames=2, nms=NONE, k=6)
    for nv in MANY:                                                                       # counts beyond the first wave of the offsets scan, a deep binary search
        c["%d views" % nv] = _case(*many_views(nv), frames=[(-1 if i % 11 == 5 else i % 3) for i in range(nv)], n_frames=3, k=40)
    c["type 0, prune and thr ignored"] = _case(APART, frames=[0, 0, 0], n_frames=1, nms=capi.make_nms("none", thr=1e9, prune=True, maxCount=1))
    return c


@functools.lru_cache(maxsize=None)
def expected(name):
    return merge(**cases()[name])


# ---------------------------------------------------------------- the pipeline case

PIPE_BOX = (50, 40, 32, 24)                                                               # of stored frame 0, 4 : 3 like the plan: a strong zoom, a few hundred hits a view
PIPE_ANGLES = (0, 6, -6, 12, -12)
PIPE_BOX1 = (120, 100, 128, 96)                                                            # of stored frame 1 (reaches over its border), at 0 and 6 degrees
PIPE_FRAMES = np.array([0, 1, 0, 0, 1, 0, 0], np.int32)
PIPE_SAMPLES = 2
PIPE_K = 48
PIPE_NMS = dict(ovr="union", overlap=0.5)


@functools.lru_cache(maxsize=None)
def pipe_views():
    a = iter(PIPE_ANGLES)
    other = iter([vr.from_box(PIPE_BOX1, a, vr.H, vr.W) for a in (0.0, vr.deg(6))])
    return np.stack([vr.from_box(PIPE_BOX, vr.deg(next(a)), vr.H, vr.W) if f == 0 else next(other) for f in PIPE_FRAMES])


@functools.lru_cache(maxsize=None)
def pipe_oracle_lists():
    """the CPU oracle's detections of the restatement's images of the pipeline case's views (uint8 stored frames), as view_ref.oracle_hits
    finds them: per view a DET_DTYPE array, raw (scale, column, row) order"""
    from oracle import binding as ob
    U = vr.stored_u8()[1]
    img = vr.image(U, pipe_views(), PIPE_FRAMES, vr.H, vr.W, PIPE_SAMPLES, F(1 / 255.0))
    plan = ob.Plan(vr.model(), vr.H, vr.W, 3)
    out = []
    for i in range(len(img)):
        pyr, _, _ = ob.chns_pyramid(plan, np.ascontiguousarray(img[i].transpose(0, 2, 1)))
        out.append(ob.detect(plan, pyr)[0])
    return out


def lists_to_arrays(lists, max_hits):
    dets = np.zeros((len(lists), max_hits), dtype=capi.DET_DTYPE)
    for v, l in enumerate(lists):
        dets[v, :len(l)] = l
    return dets, np.array([len(l) for l in lists], np.int32)
