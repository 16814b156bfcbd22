"""Shared by tests/test_tree_topology.py (CPU) and tests/test_gpu_tree_topology.py: variable-depth trees (treeDepth 0, the child-pointer
walk `while (child[k])`, acfDetect1.cpp:146-166) of every shape, built on synth.make_model(.., treeDepth=0) by replacing fids / thrs /
hs / child with [nTrees][nTreeNodes] arrays.  Everything is drawn from synth.uniform, so every machine builds identical bytes.

The reference's convention: child[k] == 0 marks a leaf; otherwise the walk goes on at node child[k] - (ftr < thr) of the same tree, so
the pair sits at child[k] - 1 and child[k], both after k.  Where the walk must not look there is garbage: leaves carry fids 0xFFFFFFFF
and thrs NaN, nodes with a test carry hs NaN, unused slots carry child 0 and garbage in all three — a read of the wrong node becomes a
NaN score (which is no hit and no equal bit pattern) or a refusal.

The leaf ranges and cascThr of the detect cases (CASES) were tuned against the oracle alone, on this module's buffers; the hit fractions
recorded there are asserted by tests/test_tree_topology.py."""
import ctypes as C
import functools

import numpy as np

from acf_amd import capi, synth

SHAPES = ("mixed", "chain", "sparse", "scattered", "bare", "one_node", "heap2", "heap3")
# shape -> (deepest leaf, nTreeNodes)
GEOMETRY = {"mixed": (4, 31), "chain": (8, 17), "sparse": (3, 511), "scattered": (3, 40), "bare": (4, 31), "one_node": (0, 1),
            "heap2": (2, 7), "heap3": (3, 15)}
P_LEAF = 0.35                          # a node below the root of a mixed / bare / scattered / sparse tree is a leaf with this probability
BARE_AT = (0, 15, 16, 31, 32, 127, 128)  # and the last tree: the staged path's stages end at 16 / 32 / 128 trees
BAD_FID = 0xFFFFFFFF
UNUSED, TEST, LEAF = 0, 1, 2

NC, WP, HP = 10, 60, 44                # the operator entries' channel buffer (tests/test_gpu_ops.py test_acf_detect1's)
TREE_COUNTS = (12, 16, 17, 40, 129, 193, 300)  # one stage, exact stage ends, a one-tree tail, a partial 64-tree tail batch


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def rnd(seed, shape, lo=0.0, hi=1.0):
    n = int(np.prod(shape))
    return (lo + (hi - lo) * synth.uniform(seed, n, 3)).astype(np.float32).reshape(shape)


# ------------------------------------------------------------------ topology

def _tree(shape, maxDepth, nNodes, bare, draws):
    """One tree: (child row, role row).  draws: an iterator of uniforms in [0, 1)."""
    child = np.zeros(nNodes, np.uint32)
    role = np.zeros(nNodes, np.uint8)
    if bare or nNodes == 1 or maxDepth == 0:
        role[0] = LEAF
        return child, role
    role[0] = TEST
    depth_first = shape in ("scattered", "sparse")
    gap_max = {"scattered": 3, "sparse": 60}.get(shape, 0)
    todo = [(0, 0)]
    nxt = 1
    last_pair = None
    while todo:
        k, dep = todo.pop() if depth_first else todo.pop(0)
        a = nxt + (int(next(draws) * gap_max) if gap_max else 0)
        assert a > k and a + 1 < nNodes, (shape, k, a, nNodes)
        child[k] = a + 1
        nxt = a + 2
        last_pair = (k, a)
        keep = int(next(draws) < 0.5) if shape == "chain" else -1
        for side in (0, 1):
            s = a + side
            if dep + 1 >= maxDepth:
                leaf = True
            elif shape in ("heap2", "heap3"):
                leaf = False
            elif shape == "chain":
                leaf = side != keep
            else:
                leaf = next(draws) < P_LEAF
            role[s] = LEAF if leaf else TEST
            if not leaf:
                todo.append((s, dep + 1))
    if shape == "sparse":
        # the pair placed last has two leaves (a test's pair would lie after it): move it to the end of the row, so that child reaches
        # its largest legal value nTreeNodes - 1
        k, a = last_pair
        assert role[a] == LEAF and role[a + 1] == LEAF
        role[a] = role[a + 1] = UNUSED
        child[k] = nNodes - 1
        role[nNodes - 2] = role[nNodes - 1] = LEAF
    return child, role


def grow(shape, maxDepth, nTreeNodes, nTrees, fid_val, thr_val, hs_val, seed=17):
    """Parent-first trees of one shape.  fid_val / thr_val / hs_val: [nTrees][nTreeNodes] values a slot takes if it is a test (fid, thr)
    or a leaf (hs); every other field of a slot is garbage.  -> fids, thrs, hs, child, role."""
    assert shape in SHAPES
    per = 96
    u = synth.uniform(seed, nTrees * per, 41).reshape(nTrees, per)
    child = np.zeros((nTrees, nTreeNodes), np.uint32)
    role = np.zeros((nTrees, nTreeNodes), np.uint8)
    for t in range(nTrees):
        bare = shape == "bare" and (t in BARE_AT or t == nTrees - 1)
        child[t], role[t] = _tree(shape, maxDepth, nTreeNodes, bare, iter(u[t]))
    fid_val = np.asarray(fid_val).astype(np.uint64)
    junk = synth.splitmix64(seed, nTrees * nTreeNodes, 43).reshape(nTrees, nTreeNodes)
    # unused slots: a feature id far outside any window, an infinite threshold, a NaN leaf
    fids = np.where(role == TEST, fid_val, np.where(role == LEAF, np.uint64(BAD_FID), (junk >> np.uint64(32)) | np.uint64(0x80000000))).astype(np.uint32)
    thrs = np.where(role == TEST, thr_val, np.where(role == LEAF, np.nan, np.inf)).astype(np.float32)
    hs = np.where(role == LEAF, hs_val, np.nan).astype(np.float32)
    return fids, thrs, hs, child, role


def model(shape, nTrees, cascThr=-1.0, hs_range=(-0.2, 0.2), maxDepth=None, nTreeNodes=None, seed=17, channel_thrs=False, **kw):
    """synth.make_model(name="TINY", treeDepth=0) with trees of `shape`.  channel_thrs: the (feature, threshold) pairs are synth's own,
    thresholds between the quartiles of the feature's channel (for real frames); else features uniform over the window and thresholds in
    (0.1, 0.5) (for the random buffers in (0, 0.6))."""
    d0, n0 = GEOMETRY[shape]
    maxDepth = d0 if maxDepth is None else maxDepth
    if nTreeNodes is None:
        nTreeNodes = max(n0, (1 << (maxDepth + 1)) - 1) if shape in ("mixed", "bare") else n0
    kw.setdefault("name", "TINY")
    m = synth.make_model(seed=seed, nTrees=nTrees, treeDepth=0, cascThr=cascThr, **kw)
    nF = synth.n_channels(m) * (m["modelDsPad_h"] // m["shrink"]) * (m["modelDsPad_w"] // m["shrink"])
    n = nTrees * nTreeNodes
    if channel_thrs:
        rows = (nTreeNodes + 6) // 7
        pool = synth.make_model(seed=seed + 1, nTrees=nTrees * rows, treeDepth=0, **kw)
        fid_val = pool["fids"].reshape(nTrees, rows * 7)[:, :nTreeNodes]
        thr_val = pool["thrs"].reshape(nTrees, rows * 7)[:, :nTreeNodes]
    else:
        fid_val = np.minimum((synth.uniform(seed, n, 45) * nF).astype(np.int64), nF - 1).reshape(nTrees, nTreeNodes)
        thr_val = (0.1 + 0.4 * synth.uniform(seed, n, 46)).reshape(nTrees, nTreeNodes)
    lo, hi = hs_range
    hs_val = (lo + (hi - lo) * synth.uniform(seed, n, 47)).reshape(nTrees, nTreeNodes)
    fids, thrs, hs, child, role = grow(shape, maxDepth, nTreeNodes, nTrees, fid_val, thr_val, hs_val, seed)
    m.update(fids=fids, thrs=thrs, hs=hs, child=child)
    return m


def roles(m):
    """Which slots a walk from the root can reach, and as what: [nTrees][nTreeNodes] of UNUSED / TEST / LEAF."""
    child = np.asarray(m["child"])
    role = np.zeros(child.shape, np.uint8)
    for t in range(child.shape[0]):
        todo = [0]
        while todo:
            k = todo.pop()
            if child[t, k]:
                role[t, k] = TEST
                todo += [int(child[t, k]) - 1, int(child[t, k])]
            else:
                role[t, k] = LEAF
    return role


def depth_of(m):
    """The deepest leaf of any tree (0: every root is a leaf)."""
    child = np.asarray(m["child"])
    deepest = 0
    for t in range(child.shape[0]):
        todo = [(0, 0)]
        while todo:
            k, d = todo.pop()
            if child[t, k]:
                todo += [(int(child[t, k]) - 1, d + 1), (int(child[t, k]), d + 1)]
            else:
                deepest = max(deepest, d)
    return deepest


def pad_full(m, D):
    """The equivalent full depth-D heap model (treeDepth D, nTreeNodes 2^(D+1) - 1; heap node i's children are 2i + 1 for ftr < thr and
    2i + 2 otherwise, getChild acfDetect1.cpp:100-107).  A leaf above depth D becomes a subtree of one in-range test whose leaves all
    carry the leaf's value: every tree contributes the same value in the same tree order."""
    child, fids, thrs, hs = (np.asarray(m[k]) for k in ("child", "fids", "thrs", "hs"))
    nTrees = child.shape[0]
    nNodes = (1 << (D + 1)) - 1
    nInternal = (1 << D) - 1
    F = np.zeros((nTrees, nNodes), np.uint32)
    T = np.zeros((nTrees, nNodes), np.float32)
    Hs = np.zeros((nTrees, nNodes), np.float32)
    for t in range(nTrees):
        todo = [(0, 0)]  # (heap node, the variable tree's node it stands for)
        while todo:
            i, k = todo.pop()
            if i >= nInternal:
                if child[t, k]:
                    raise ValueError("tree %d is deeper than %d" % (t, D))
                Hs[t, i] = hs[t, k]
            elif child[t, k]:
                F[t, i], T[t, i] = fids[t, k], thrs[t, k]
                todo += [(2 * i + 1, int(child[t, k]) - 1), (2 * i + 2, int(child[t, k]))]
            else:
                F[t, i], T[t, i] = 0, 0.3
                todo += [(2 * i + 1, k), (2 * i + 2, k)]
    out = dict(m)
    out.update(treeDepth=D, fids=F, thrs=T, hs=Hs, child=np.zeros((nTrees, nNodes), np.uint32))
    return out


# ------------------------------------------------------------------ the plain walker (the oracle's independent reference)

def window_geometry(m):
    return m["modelDsPad_h"] // m["shrink"], m["modelDsPad_w"] // m["shrink"]


def walk(chns_window, m, t, thrs=None):
    """The leaf value tree t reaches on one window's cells [nC][mW][mH], walking from the root."""
    mH, mW = window_geometry(m)
    thrs = m["thrs"] if thrs is None else thrs
    k = 0
    while m["child"][t, k]:
        f = int(m["fids"][t, k])
        z, cc, rr = f // (mW * mH), (f // mH) % mW, f % mH   # cids[], acfDetect1.cpp:390-406
        k = int(m["child"][t, k]) - (1 if np.float32(chns_window[z, cc, rr]) < np.float32(thrs[t, k]) else 0)
    return np.float32(m["hs"][t, k])


def score_window(chns_window, m, cascThr, thrs=None):
    """Detector::evaluate: leaves added in f32 in tree order until h <= cascThr (acfDetect1.cpp:123-138)."""
    h = np.float32(0.0)
    for t in range(m["fids"].shape[0]):
        h = np.float32(h + walk(chns_window, m, t, thrs))
        if h <= np.float32(cascThr):
            break
    return h


def walk_hits(chns, m, thrs=None):
    """acfDetect1 on one buffer [nC][wP][hP] (float, or bytes with byte thresholds) with the walker, all windows of a tree at a time:
    -> hits (capi.HIT_DTYPE) in the reference's order (column, then row)."""
    nC, wP, hP = chns.shape
    mH, mW = window_geometry(m)
    shrink, stride = m["shrink"], m["stride"]
    nR = max(0, -(-(hP * shrink - m["modelDsPad_h"] + 1) // stride))
    nCc = max(0, -(-(wP * shrink - m["modelDsPad_w"] + 1) // stride))
    cc, rr = np.meshgrid(np.arange(nCc), np.arange(nR), indexing="ij")
    c, r = cc.ravel(), rr.ravel()                               # column-major: c outer, r inner
    c0, r0 = c * stride // shrink, r * stride // shrink
    data = np.asarray(chns, np.float32)
    th = np.asarray(m["thrs"] if thrs is None else thrs, np.float32)
    child, fids, hs = (np.asarray(m[k]) for k in ("child", "fids", "hs"))
    h = np.zeros(len(c), np.float32)
    alive = np.ones(len(c), bool)
    for t in range(child.shape[0]):
        idx = np.nonzero(alive)[0]
        if not len(idx):
            break
        k = np.zeros(len(idx), np.int64)
        while True:
            go = child[t, k] != 0
            if not go.any():
                break
            kk = k[go]
            f = fids[t, kk].astype(np.int64)
            ftr = data[f // (mW * mH), c0[idx[go]] + (f // mH) % mW, r0[idx[go]] + f % mH]
            k[go] = child[t, kk].astype(np.int64) - (ftr < th[t, kk])
        h[idx] = h[idx] + hs[t, k]
        alive[idx] = h[idx] > np.float32(m["cascThr"])
    out = np.zeros(int(alive.sum()), capi.HIT_DTYPE)
    out["c"], out["r"], out["score"] = c[alive], r[alive], h[alive]
    return out


# ------------------------------------------------------------------ oracle calls

def oracle_detect1(oracle, m, chns, thrs_u8=None):
    """acfo_acf_detect1 on float planes [nC][wP][hP], or on byte planes with byte thresholds."""
    nC, wP, hP = chns.shape
    params, keep = capi.make_params(m)
    thrs = keep["thrs"] if thrs_u8 is None else np.ascontiguousarray(thrs_u8, np.uint8)
    want = np.zeros(1 << 16, dtype=capi.HIT_DTYPE)
    n = oracle.lib().acfo_acf_detect1(chns.ctypes.data_as(C.c_void_p), 0 if thrs_u8 is None else 1, thrs.ctypes.data_as(C.c_void_p), hP, wP, nC,
                                      C.byref(params), want.ctypes.data_as(C.POINTER(capi.Hit)), 1 << 16, 0)
    assert 0 <= n <= 1 << 16
    return want[:n].copy()


def oracle_evaluate(oracle, m, chns, cascThr):
    params, keep = capi.make_params(m)
    nC, wP, hP = chns.shape
    return np.float32(oracle.lib().acfo_evaluate(oracle.F(np.ascontiguousarray(chns, np.float32)), hP, wP, nC, C.byref(params), np.float32(cascThr)))


def n_windows(m, wP, hP):
    s, st = m["shrink"], m["stride"]
    return max(0, -(-(hP * s - m["modelDsPad_h"] + 1) // st)) * max(0, -(-(wP * s - m["modelDsPad_w"] + 1) // st))


def check_model(m, nChns):
    """acf_hip_check_model (host only) -> (code, reason)"""
    params, keep = capi.make_params(m)
    why = C.create_string_buffer(256)
    rc = capi.load().acf_hip_check_model(C.byref(params), nChns, why, 256)
    return rc, why.value.decode()


# ------------------------------------------------------------------ the detect cases of the operator entries

@functools.lru_cache(maxsize=None)
def buffer_f32():
    a = rnd(99, (NC, WP, HP), 0.0, 0.6)
    a.setflags(write=False)
    return a


@functools.lru_cache(maxsize=None)
def buffer_u8():
    a = (rnd(77, (NC, WP, HP), 0.0, 0.6) * 255.0).astype(np.uint8)
    a.setflags(write=False)
    return a


# Leaves uniform in (-0.2, 0.2): a zero-mean walk of step deviation 0.4 / sqrt(12).  The score of a window after n trees is then about
# 0.115 sqrt(n) wide, so cascThr = -CASC_K * 0.115 sqrt(n) keeps a fraction of the windows that depends little on n (the chance that a
# random walk stays above -B for n steps is erf(B / (sigma sqrt(2 n)))): the threshold moves with the tree count.
HS_RANGE = (-0.2, 0.2)
CASC_K = 0.5


def casc_thr(nTrees):
    return -float(np.float32(CASC_K * (0.4 / np.sqrt(12.0)) * np.sqrt(float(nTrees))))


def detect_model(shape, nTrees, maxDepth=None):
    if shape == "one_node":
        # every tree is one leaf: all windows score alike, so a case keeps either all or none of them.  Positive leaves: all, with the
        # early exit never taken, and every window's score compared.
        return model(shape, nTrees, cascThr=-1.0, hs_range=(0.0, 0.2))
    return model(shape, nTrees, cascThr=casc_thr(nTrees), hs_range=HS_RANGE, maxDepth=maxDepth)


# tests/fuzz_parity.py: random frames of any size and stride.  The leaves also drift down, by `drift` step deviations over the whole
# model; the script takes the strongest drift of FUZZ_DRIFTS that leaves the oracle a hit on the case's first frame, so that few
# windows are hits (a frame with more hits than the buffers hold is not compared at all).  one_node is left out there: its windows
# are all hits or all none.
FUZZ_SHAPES = tuple(s for s in SHAPES if s != "one_node")
FUZZ_DRIFTS = (3.0, 2.0, 1.0, 0.0)


def fuzz_model(shape, nTrees, seed, drift, **kw):
    d = drift * (0.4 / np.sqrt(12.0)) / np.sqrt(float(nTrees))
    return model(shape, nTrees, cascThr=casc_thr(nTrees), hs_range=(HS_RANGE[0] - d, HS_RANGE[1] - d), seed=seed, channel_thrs=True, **kw)


# (shape, nTrees) -> (hit fraction on buffer_f32, on buffer_u8 with the model's thresholds as bytes), the oracle's, to three places.
# Asserted by tests/test_tree_topology.py, which also asserts 0.01 <= fraction <= 0.90 for every shape but one_node (1.0 by construction).
CASES = {
    ("mixed", 12): (0.337, 0.362),
    ("mixed", 16): (0.369, 0.392),
    ("mixed", 17): (0.374, 0.394),
    ("mixed", 40): (0.520, 0.523),
    ("mixed", 129): (0.466, 0.452),
    ("mixed", 193): (0.511, 0.503),
    ("mixed", 300): (0.552, 0.525),
    ("chain", 12): (0.091, 0.087),
    ("chain", 16): (0.093, 0.097),
    ("chain", 17): (0.097, 0.100),
    ("chain", 40): (0.049, 0.048),
    ("chain", 129): (0.056, 0.053),
    ("chain", 193): (0.041, 0.039),
    ("chain", 300): (0.069, 0.062),
    ("sparse", 12): (0.175, 0.185),
    ("sparse", 16): (0.187, 0.196),
    ("sparse", 17): (0.193, 0.201),
    ("sparse", 40): (0.102, 0.106),
    ("sparse", 129): (0.130, 0.124),
    ("sparse", 193): (0.162, 0.171),
    ("sparse", 300): (0.202, 0.208),
    ("scattered", 12): (0.264, 0.295),
    ("scattered", 16): (0.240, 0.261),
    ("scattered", 17): (0.236, 0.258),
    ("scattered", 40): (0.181, 0.205),
    ("scattered", 129): (0.169, 0.186),
    ("scattered", 193): (0.236, 0.261),
    ("scattered", 300): (0.321, 0.345),
    ("bare", 12): (0.458, 0.467),
    ("bare", 16): (0.493, 0.504),
    ("bare", 17): (0.499, 0.511),
    ("bare", 40): (0.716, 0.716),
    ("bare", 129): (0.610, 0.609),
    ("bare", 193): (0.680, 0.665),
    ("bare", 300): (0.711, 0.688),
    ("one_node", 12): (1.000, 1.000),
    ("one_node", 16): (1.000, 1.000),
    ("one_node", 17): (1.000, 1.000),
    ("one_node", 40): (1.000, 1.000),
    ("one_node", 129): (1.000, 1.000),
    ("one_node", 193): (1.000, 1.000),
    ("one_node", 300): (1.000, 1.000),
    ("heap2", 12): (0.749, 0.744),
    ("heap2", 16): (0.782, 0.774),
    ("heap2", 17): (0.786, 0.779),
    ("heap2", 40): (0.820, 0.796),
    ("heap2", 129): (0.315, 0.331),
    ("heap2", 193): (0.292, 0.313),
    ("heap2", 300): (0.263, 0.283),
    ("heap3", 12): (0.530, 0.530),
    ("heap3", 16): (0.506, 0.505),
    ("heap3", 17): (0.496, 0.490),
    ("heap3", 40): (0.303, 0.285),
    ("heap3", 129): (0.195, 0.196),
    ("heap3", 193): (0.215, 0.211),
    ("heap3", 300): (0.247, 0.241),
}

# device(variable) against device(pad_full(.., D)): mixed trees no deeper than D, at tree counts that end in the tile kernels' stages
# and behind them
PAD_DEPTHS = (1, 2, 3, 4)
PAD_TREES = (17, 40, 193)

# ------------------------------------------------------------------ op_evaluate: the (10, 9, 7) buffer of test_evaluate_single_window
EVAL_SHAPES = ("mixed", "chain", "scattered", "sparse", "bare", "one_node", "heap2", "heap3")
EVAL_TREES = 128
EVAL_LEAVES = [(-0.25, 0.2), (-0.05, 0.3), (0.0, 0.3), (-0.3, 0.0)]


def eval_buffer(k):
    return rnd(50 + k, (NC, 9, 7), 0.0, 0.6)


def eval_model(shape, k):
    return model(shape, EVAL_TREES, cascThr=-1.0, hs_range=EVAL_LEAVES[k], seed=11 + k)


# ------------------------------------------------------------------ evaluate_crops: 16 crops of 16 x 16
CROP_SHAPES = ("mixed", "chain", "scattered")
CROP_TREES = 128


def crop_model(shape, early):
    """early: leaves with which cascThr = 0 stops some crops and lets others pass"""
    return model(shape, CROP_TREES, hs_range=(-0.10, 0.30) if early else (-0.2, 0.2), seed=3, channel_thrs=True, isLuv=1)


# ------------------------------------------------------------------ the planned pipeline: TINY on 200 x 264 frames
PIPE_H, PIPE_W, PIPE_FRAMES = 200, 264, 3
PIPE_MODELS = {"mixed193": ("mixed", 193), "chain40": ("chain", 40)}
# name -> (cascThr, leaf range), tuned on the oracle's hit fraction over all levels of the three frames (recorded in PIPE_FRACTIONS)
PIPE_TUNING = {"mixed193": (-1.0, (-0.23, 0.2)), "chain40": (-0.5, (-0.25, 0.2))}
PIPE_FRACTIONS = {"mixed193": (0.050, 0.088, 0.085), "chain40": (0.021, 0.029, 0.029)}  # per frame, stride 4, to three places


def pipe_model(name, **over):
    shape, nTrees = PIPE_MODELS[name]
    thr, hs_range = PIPE_TUNING[name]
    return model(shape, nTrees, cascThr=thr, hs_range=hs_range, seed=5, channel_thrs=True, **over)


@functools.lru_cache(maxsize=None)
def pipe_frames():
    a = np.stack([synth.make_frame(300 + i, PIPE_H, PIPE_W, "luv") for i in range(PIPE_FRAMES)])
    a.setflags(write=False)
    return a


@functools.lru_cache(maxsize=None)
def pipe_expected(name, stride=4):
    """-> (oracle plan, [per frame dict(pyr, det, hits)], windows over all levels)"""
    from oracle import binding as ob
    m = pipe_model(name, stride=stride)
    plan = ob.Plan(m, PIPE_H, PIPE_W, 3)
    out = []
    for f in pipe_frames():
        pyr, _, _ = ob.chns_pyramid(plan, f)
        det, hits = ob.detect(plan, pyr)
        out.append(dict(pyr=pyr, det=det, hits=hits))
    nwin = sum(int(plan.levels[i].nWinR) * int(plan.levels[i].nWinC) for i in range(plan.nScales))
    return plan, out, nwin


# ------------------------------------------------------------------ evaluate_crops_u8: 16 packed RGB crops of 16 x 16
@functools.lru_cache(maxsize=None)
def crop_bytes(n=16):
    """uint8 [n][16][16][3], noise averaged with its right-hand neighbour (so that the walks do not all end alike)"""
    a = (synth.splitmix64(77, n * 16 * 16 * 3) >> np.uint64(56)).astype(np.uint8).reshape(n, 16, 16, 3)
    a = ((a.astype(np.uint16) + np.roll(a, 1, axis=2)) // 2).astype(np.uint8)
    a.setflags(write=False)
    return a


def crop_model_u8(shape, early):
    """the byte crops are RGB: the model converts (isLuv 0)"""
    return model(shape, CROP_TREES, hs_range=(-0.20, 0.30) if early else (-0.2, 0.2), seed=3, channel_thrs=True, isLuv=0)


# ------------------------------------------------------------------ the C++ host: a scattered model from a .cpb, 96 x 128 frames
CPP_H, CPP_W, CPP_FRAMES = 96, 128, 2


def cpp_model():
    return model("scattered", 96, cascThr=-1.0, hs_range=(-0.23, 0.2), seed=3, channel_thrs=True)


@functools.lru_cache(maxsize=None)
def cpp_frames():
    a = np.stack([synth.make_frame(40 + i, CPP_H, CPP_W, "luv") for i in range(CPP_FRAMES)])
    a.setflags(write=False)
    return a
