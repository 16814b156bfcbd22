"""Shared by tests/test_cascade_edges.py (CPU) and tests/test_gpu_cascade_edges.py: designed models on a designed buffer that hold the
cascade's rule — a window leaves at the FIRST tree t with h <= cascThr and never comes back (acfDetect1.cpp:123-138) — at every tree
position, at the tie h == cascThr and at model lengths on every stage end.  The random models of the other cascade tests check the
score bits of the survivors; their leaf amplitudes decay, so a window that dips below cascThr and would be lifted back does not occur.

Buffer (tests/test_gpu_ops.py::test_acf_detect1's): 10 channels of 60 x 44 cells uniform in [0, 0.6), the TINY window of 4 x 4 cells:
57 x 41 = 2337 windows in eight tiles that are partial in both axes, more windows than the 1024 leaf-code rows of a tail.  TALL: the
same 60 columns with 88 rows (twelve tiles: a grid of 8 persistent workgroups draws more than one tile each).

Base model: random feature ids, thresholds in [0.1, 0.5], leaves uniform in [-0.01, 0.02] (nothing leaves by itself), cascThr -1.
Families, each a list of tree positions T per model (positions(), split(): over the models of one (depth, length) every tree of
[0, min(nTrees, 193)) and the last tree is a position; at most 8 per model, at least 2 apart):
  dip   tree T: root f < 0.12 (the 20 % quantile), every leaf of the left subtree -8.  Tree T + 1: the same root, left subtree +8.
        The oracle rejects the left class at T; a kernel that does not test h after exactly tree T resurrects it.
  bump  tree T: the same root, left subtree -8 (a plain rejection, so that the hit share stays below 0.9 — with nothing rejected every
        window of a bump model would be a hit), right subtree +8.  Tree T + 1: right subtree -8.  The oracle keeps the right class; a
        kernel that adds the pair in the other order, or tests between the two halves of a sum it formed out of order, loses it.
  tie   every leaf of the model is 2^-6 (every sum exact in any order; the common score before tree T is T * 2^-6).  Tree T: root
        f < 0.12, its left child g < 0.36 (depth 1: the root alone): left-left lands on exactly -1.0 and must go, left-right lands on
        -1.0 + 2^-6 and stays.  Positions: tie_positions().
  A position that is the model's last tree has no T + 1: the tree at T alone.
Mutants (evaluate()'s arguments; CPU only): skip = the h <= cascThr test left out after tree T; swap = trees T and T + 1 exchanged;
strict = `<` in place of `<=` at tree T (at the last tree the hit test h > cascThr becomes >= with it: a kernel that folds the
last test into the hit decision).
"""
import functools
import os
import sys

import numpy as np

if __name__ == "__main__":
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from acf_amd import capi, synth  # noqa: E402

NC, WP, HP, HP_TALL = 10, 60, 44, 88
CASC_THR = -1.0
TAU, TAU2 = 0.12, 0.36
BIG, Q = 8.0, 2.0 ** -6
CODES_CAP = 1024          # leafCodeBuffer: max(nWin / 64, 1024) rows for a buffer of fewer than 65536 windows
HIT_LO, HIT_HI = 0.05, 0.9
MIN_CHANGE = 32
LENGTHS2 = (1, 2, 3, 4, 5, 15, 16, 17, 19, 20, 31, 32, 33, 47, 48, 49, 64, 65, 96, 97, 127, 128, 129, 160, 161, 191, 192, 193, 257)
LENGTHS_D = (20, 30, 32, 33, 128, 129, 160)      # depths 1, 3, 4
LENGTHS_0 = (33, 129)                            # depth 0: the child walk
OVERFLOW = (129, 193, 257)
CHILD_LENGTHS = (33, 129, 193)
CHILD_ENVS = ("ACF_HIP_FORCE_FALLBACK=tail3", "ACF_HIP_FORCE_FALLBACK=no_tail_codes", "ACF_HIP_FORCE_FALLBACK=tiled_staged", "ACF_HIP_CASC_BOUNDS=8,24,24,96")
GROUPS = [(2, n) for n in LENGTHS2] + [(d, n) for d in (1, 3, 4) for n in LENGTHS_D] + [(0, n) for n in LENGTHS_0]


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def rnd(seed, shape, lo=0.0, hi=1.0):
    n = int(np.prod(shape))
    return (lo + (hi - lo) * synth.uniform(seed, n, 3)).astype(np.float32).reshape(shape)


@functools.lru_cache(maxsize=None)
def buffer(tall=False):
    a = rnd(4242 + int(tall), (NC, WP, HP_TALL if tall else HP), 0.0, 0.6)
    a.setflags(write=False)
    return a


# ------------------------------------------------------------------ positions

def positions(n):
    return list(range(min(n, 193))) + ([n - 1] if n > 193 else [])


def split(pos, per=8):
    """the positions dealt round-robin to the fewest models of at most `per` each; two models at least, so that neighbours part"""
    if len(pos) < 2:
        return [list(pos)]
    m = max(2, -(-len(pos) // per))
    out = [pos[j::m] for j in range(m)]
    assert all(b - a >= 2 for p in out for a, b in zip(p, p[1:]))
    return out


def tie_positions(n):
    """first and last tree of each stage, one interior tree of each dense batch of four, the four trees of one chain quad (and the
    tree on each side of a group of 16) of the sparse stage, one tree in each 64-tree code row of the tail"""
    want = [0, 15, 16, 31, 32, 127, 128, n - 1] + [4 * k + 2 for k in range(8)] + [36, 37, 38, 39, 47, 48] + list(range(128 + 37, n, 64))
    return sorted({t for t in want if 0 <= t < n})


def overflow_positions(n):
    """no position before tree 128: every window reaches the tail"""
    a = [t for t in (128, 190, 192, 256) if t < n]
    b = [t for t in (129, 191, 193) if t < n]
    if n - 1 not in a + b:
        a.append(n - 1)
    return [sorted(set(p)) for p in (a, b) if p]


@functools.lru_cache(maxsize=None)
def group_cases(depth, n):
    """-> [(family, positions)] of one (depth, length): the models that one GPU test runs"""
    out = [(fam, tuple(p)) for fam in ("dip", "bump") for p in split(positions(n))]
    out += [("tie", tuple(p)) for p in split(tie_positions(n), 6)]
    return out


@functools.lru_cache(maxsize=None)
def overflow_cases(n):
    return [(fam, tuple(p)) for fam in ("dip", "bump", "tie") for p in overflow_positions(n)]


# ------------------------------------------------------------------ models

def leaves_under(k, depth):
    """leaf nodes (heap order) below node k of a full tree of `depth` levels"""
    lo = hi = k
    while lo < (1 << depth) - 1:
        lo, hi = 2 * lo + 1, 2 * hi + 2
    return list(range(lo, hi + 1))


def make_model(family, depth, n, pos, window=4, nC=NC, seed=0, quantile=None):
    """the base model with the family's trees at the positions `pos`; quantile(feature id, q): the threshold that a share q of the
    feature's cells lies below (None: the buffer's uniform [0, 0.6))"""
    quantile = quantile or (lambda f, q: q * 0.6)
    px = 4 * window
    m = synth.make_model(seed=17, name="TINY", nTrees=n, cascThr=CASC_THR, treeDepth=depth, modelDs_h=px, modelDs_w=px, modelDsPad_h=px, modelDsPad_w=px,
                         minDs_h=px, minDs_w=px, **({"gradHistEnabled": 1, "nOrients": nC - 4} if nC != NC else {}))
    wd = depth if depth > 0 else 2                     # (depth 0: synth's child[] spells the depth-2 topology)
    nInt = (1 << wd) - 1
    nF = nC * window * window
    s = 1000 * n + 10 * depth + seed + sum(pos) * 7 + {"dip": 1, "bump": 2, "tie": 3}[family]
    shape = m["fids"].shape
    fids = np.minimum((synth.uniform(s, shape[0] * shape[1], 1) * nF).astype(np.int64), nF - 1).astype(np.uint32).reshape(shape)
    thrs = rnd(s + 1, shape, 0.1, 0.5)
    hs = rnd(s + 2, shape, -0.01, 0.02) if family != "tie" else np.full(shape, Q, np.float32)
    fids[:, nInt:] = 0
    thrs[:, nInt:] = 0
    hs[:, :nInt] = 0
    # one feature per position, all distinct, so that the classes of one model are independent
    feat = (np.argsort(synth.uniform(s + 3, nF, 2))[:2 * len(pos)]).astype(np.uint32).reshape(2, -1)
    L, R = leaves_under(1, wd), leaves_under(2, wd)
    for i, T in enumerate(pos):
        assert 0 <= T < n
        pair = [T, T + 1] if T + 1 < n and family != "tie" else [T]   # (a tie is one tree)
        for t in pair:
            fids[t, 0], thrs[t, 0] = feat[0, i], quantile(feat[0, i], TAU / 0.6)
        if family == "dip":
            hs[T, L] = -BIG
            if len(pair) > 1:
                hs[T + 1, L] = BIG
        elif family == "bump":
            hs[T, L], hs[T, R] = -BIG, BIG
            if len(pair) > 1:
                hs[T + 1, R] = -BIG
        else:
            if wd > 1:
                fids[T, 1], thrs[T, 1] = feat[1, i], quantile(feat[1, i], TAU2 / 0.6)
                hs[T, leaves_under(3, wd)] = CASC_THR - T * Q
                hs[T, leaves_under(4, wd)] = CASC_THR + Q - T * Q
            else:
                hs[T, L] = CASC_THR - T * Q
    m.update(fids=fids, thrs=thrs, hs=np.ascontiguousarray(hs, np.float32))
    return m


# ------------------------------------------------------------------ evaluate(), restated in numpy (acfDetect1.cpp:84-138)

def features(chns, window=4):
    """-> [feature id][window] of every window of the buffer, windows column by column (the order of the hit list); stride == shrink"""
    nC, wP, hP = chns.shape
    nWc, nWr = wP - window + 1, hP - window + 1
    out = np.empty((nC * window * window, nWc * nWr), np.float32)
    for z in range(nC):
        for cc in range(window):
            for rr in range(window):
                out[(z * window + cc) * window + rr] = chns[z, cc:cc + nWc, rr:rr + nWr].reshape(-1)
    return out, nWr


def leaf_values(m, F):
    """-> [tree][window] the leaf value hs[k] each window's walk ends on (getChild :100-107; depth 0: the child walk :146-155)"""
    fids, thrs, hs, child, depth = m["fids"], m["thrs"], m["hs"], m["child"], m["treeDepth"]
    nT, nN = fids.shape
    ar = np.arange(F.shape[1])
    out = np.empty((nT, F.shape[1]), np.float32)
    for t in range(nT):
        k = np.zeros(F.shape[1], np.int64)
        if depth > 0:
            for _ in range(depth):
                k = 2 * k + np.where(F[fids[t, k], ar] < thrs[t, k], 1, 2)
        else:
            for _ in range(nN):
                ch = child[t, k].astype(np.int64)
                if not ch.any():
                    break
                k = np.where(ch != 0, ch - (F[fids[t, k], ar] < thrs[t, k]), k)
        out[t] = hs[t, k]
    return out


def evaluate(lv, thr=CASC_THR, skip=(), strict=(), swap=None, cols=None):
    """h += hs[k]; if (h <= cascThr) break; over the trees in order, for every window (or the windows `cols`).  -> (hit mask, h, the
    tree each window left at, or nTrees).  skip / strict / swap: the mutants of the module's docstring."""
    thr = np.float32(thr)
    lv = lv if cols is None else lv[:, cols]
    nT = lv.shape[0]
    order = list(range(nT))
    if swap is not None:
        order[swap], order[swap + 1] = order[swap + 1], order[swap]
    h = np.zeros(lv.shape[1], np.float32)
    alive = np.ones(lv.shape[1], bool)
    left = np.full(lv.shape[1], nT, np.int64)
    for i, t in enumerate(order):
        h = np.where(alive, h + lv[t], h)
        if i in skip:
            continue
        rej = alive & ((h < thr) if i in strict else (h <= thr))
        left[rej] = i
        alive &= ~rej
    hit = alive & ((h >= thr) if nT - 1 in strict else (h > thr))
    return hit, h, left


def hit_list(hit, h, nWr, scale=0):
    idx = np.flatnonzero(hit)
    out = np.zeros(len(idx), dtype=capi.HIT_DTYPE)
    out["scale"], out["c"], out["r"], out["score"] = scale, idx // nWr, idx % nWr, h[idx]
    return out


def oracle_hits(m, chns):
    import ctypes as C
    from oracle import binding as ob
    params, keep = capi.make_params(m)
    nC, wP, hP = chns.shape
    want = np.zeros(1 << 14, dtype=capi.HIT_DTYPE)
    n = ob.lib().acfo_acf_detect1(chns.ctypes.data_as(C.c_void_p), 0, keep["thrs"].ctypes.data_as(C.c_void_p), hP, wP, nC, C.byref(params),
                                  want.ctypes.data_as(C.POINTER(capi.Hit)), 1 << 14, 0)
    assert n <= 1 << 14
    return want[:n].copy()


def same_hits(got, want):
    return len(got) == len(want) and all(np.array_equal(got[k], want[k]) for k in ("scale", "c", "r")) and np.array_equal(bits(got["score"]), bits(want["score"]))


@functools.lru_cache(maxsize=None)
def buffer_features(tall=False):
    return features(buffer(tall))


def check_conditions(family, depth, n, pos, overflow=False):
    """the conditions of the inputs, with the oracle alone.  -> dict(hits, changes = {position: windows the mutant changes})"""
    m = make_model(family, depth, n, pos)
    F, nWr = buffer_features()
    lv = leaf_values(m, F)
    hit, h, left = evaluate(lv)
    where = (family, depth, n, pos)
    assert same_hits(hit_list(hit, h, nWr), oracle_hits(m, buffer())), where + ("the restatement differs from the oracle",)
    share = hit.sum() / float(len(hit))
    assert HIT_LO < share < HIT_HI, where + ("hit share", share)
    changes = {}
    for T in pos:
        if family == "tie":
            cols = np.flatnonzero((left == T) & (h == np.float32(CASC_THR)))   # (windows that an earlier tie left one step up fall further)
            changed = evaluate(lv, strict=(T,), cols=cols)[0].sum()       # (only windows that left at T on the threshold can change)
            if depth != 1:   # (a stump has one left leaf: no second class)
                run = np.cumsum(lv[:T + 1], axis=0, dtype=np.float32)[T]   # (exact: multiples of 2^-6; == h for the windows still in)
                assert np.sum((left > T) & (run == np.float32(CASC_THR + Q))) >= MIN_CHANGE, where + (T, "no class one step above cascThr")
        elif T == n - 1:
            continue
        elif family == "dip":
            changed = evaluate(lv, skip=(T,), cols=np.flatnonzero(left == T))[0].sum()
        else:
            changed = (evaluate(lv, swap=T)[0] != hit).sum()
        changes[T] = int(changed)
        assert changed >= MIN_CHANGE, where + ("position", T, "its mutant changes", int(changed), "windows")
    if overflow:
        assert (left >= 128).sum() > CODES_CAP, where + ("windows past tree 127", int((left >= 128).sum()))
    return dict(hits=int(hit.sum()), changes=changes)


# ------------------------------------------------------------------ the forms a launch must report (cascade_run.hip.h, restated)

def tile_bounds(n, env=""):
    b = (0, 8, 24, 24, 96) if "CASC_BOUNDS" in env else (0, 16, 32, 32, 128)
    return tuple(min(v, n) for v in b)


def staged_bounds(n):
    return tuple([v for v in (16, 32, 128) if v < n] + [n])


def rank_supported(depth, n, env=""):
    """a rank tile set exists: depth 2 always; depths 1, 3, 4 from 32 trees on (k_cascade_tile3D), unless tiled_staged forbids it"""
    return depth == 2 or (depth in (1, 3, 4) and n >= 32 and "tiled_staged" not in env)


def expect_forms(depth, n, form, env=""):
    """what cascade_forms() must say of one launch; form: dict(rank, tiles, persist = option tile_persist, tall)"""
    rank, tiles = form["rank"], form["tiles"]
    e = dict(rank=rank, frames=1)
    if depth == 2 and tiles:
        b = tile_bounds(n, env)
        tail = b[4] < n
        codes = tail and "tail3" not in env
        e.update(path="tiled2", kernel="tile3", b=b, pooled=True, codeScan=codes, waveTail=tail, pooledTail=False, nStages=0,
                 codes_cap=CODES_CAP if codes else 0, persist=bool(form["persist"] == 8 and form["tall"]))
        return e
    sb = staged_bounds(n)
    last = len(sb) - 1
    e.update(path="staged", nStages=len(sb), bounds=sb + (0,) * (4 - len(sb)), mode=2 if depth == 2 else 1 if depth > 0 else 0)
    wave = last > 0 and sb[last - 1] >= 128
    codes = wave and e["mode"] == 1 and depth <= 4 and "no_tail_codes" not in env
    # (the leaf-code rows are the tables': a depth-2 model past its tile stages has them whether or not the call runs tiles)
    e.update(waveTail=wave, codeScan=codes, codes_cap=CODES_CAP if codes or (depth == 2 and tile_bounds(n, env)[4] < n and "tail3" not in env) else 0)
    kernel, end = None, None
    if tiles and depth in (1, 3, 4):
        pooled = (depth in (3, 4) or rank) and n >= 32 and "tiled_staged" not in env
        tb = {1: 4, 3: 2, 4: 1}[depth]
        if pooled:
            kernel, end = "tile3D", tile_bounds(n, env)[4]
        elif min(32, n) // tb * tb in (n, 32):
            kernel, end = "tileD", min(32, n) // tb * tb
        if kernel and end not in sb:
            kernel = None
    e.update(kernel=kernel, firstStage=sb.index(end) + 1 if kernel else 0, pooledTail=bool(kernel == "tile3D" and sb.index(end) < last and codes))
    if kernel == "tile3D":
        e.update(b=tile_bounds(n, env), pooled=True, persist=bool(form["persist"] == 8 and form["tall"]))
    elif kernel == "tileD":
        e.update(pooled=False, persist=False)
    return e


def forms_of(depth, n):
    """the option combinations a (depth, length) runs under: float tiles, rank tiles, no tiles, tile_persist 0 and 8 (8 on the tall
    buffer, where twelve tiles meet a grid of eight) on both tile sets"""
    out = [dict(rank=False, tiles=1, persist=1, tall=False), dict(rank=False, tiles=0, persist=1, tall=False)]
    if depth != 0:
        out += [dict(rank=False, tiles=1, persist=0, tall=False), dict(rank=False, tiles=1, persist=8, tall=True)]
    if rank_supported(depth, n):
        out += [dict(rank=True, tiles=1, persist=p, tall=t) for p, t in ((1, False), (0, False), (8, True))]
    return out


# ------------------------------------------------------------------ the GPU side (tests/test_gpu_cascade_edges.py; a child process for the environment's forms)

@functools.lru_cache(maxsize=None)
def expected_hits(family, depth, n, pos, tall):
    m = make_model(family, depth, n, pos)
    want = oracle_hits(m, buffer(tall))
    want.setflags(write=False)
    return want


def launch(dev, m, chns, form):
    dev.set_option("cascade_tiles", form["tiles"])
    dev.set_option("tile_persist", form["persist"])
    try:
        dev.set_model(m)
        got = (dev.op_acf_detect1_rank if form["rank"] else dev.op_acf_detect1)(chns)
        return got, dev.cascade_forms()
    finally:
        dev.set_option("cascade_tiles", 1)
        dev.set_option("tile_persist", 1)


def check_forms(got, want, where):
    bad = {k: (got.get(k), v) for k, v in want.items() if got.get(k) != v}
    assert not bad, where + ("cascade_forms() (reported, wanted)", bad)


def run_group(dev, depth, n, cases, env="", forms=None):
    """every model of the group under every form: hits equal to the oracle's in number, order, position and score bits, then the
    form.  -> the reported records.  Every mismatch of the group is collected before it fails."""
    reported, errs = [], []
    for family, pos in cases:
        m = make_model(family, depth, n, pos)
        for form in forms or forms_of(depth, n):
            where = (family, depth, n, pos, tuple(sorted(form.items())), env)
            got, rec = launch(dev, m, np.array(buffer(form["tall"])), form)
            reported.append(rec)
            try:
                want = expected_hits(family, depth, n, pos, form["tall"])
                assert len(want) > 0, where
                assert len(got) == len(want), where + ("hits", len(got), "oracle", len(want))
                assert same_hits(got, want), where + ("hits differ",)
                check_forms(rec, expect_forms(depth, n, form, env), where)
            except AssertionError as e:
                errs.append(e)
    assert not errs, (len(errs), errs[:6])
    return reported


# ------------------------------------------------------------------ big windows over 16 channels on 40 x 36 cells: the tile plan's waves per workgroup
# buildTileSet takes the largest NW of 8 / 4 / 2 / 1 whose footprint + lists fit 80 KiB on float cells (a third of the LDS on rank
# cells), then 159 KiB; NW * 64 must reach the sparse stage's 128 threads.  Restated here per shape (float cells, 4 bytes):
#   "20x20"  rows 32 - 1 + 20 = 51 -> 52.  NW 2: 16 x 52 x 23 cells = 76544 bytes, + 6400 + 1024 bytes of lists + the leaf table: over
#            80 KiB; NW 1 is below 128 threads.  So the 159 KiB pass takes NW 8 (16 x 52 x 35 cells = 116480 bytes): one workgroup per CU.
#            On rank cells (2 bytes) NW 2 fits a third of the LDS.
#   "12x12"  rows 43 -> 44.  NW 8: 16 x 44 x 27 cells = 76032 bytes + 6400 + 4096 of lists: over 80 KiB; NW 4: 16 x 44 x 19 = 53504 bytes fits.
BIG_WINDOWS = {"20x20": dict(window=20, float_nw=8), "12x12": dict(window=12, float_nw=4)}
BIG_WINDOW = dict(family="dip", depth=2, n=129, pos=(15, 128), nC=16, wP=40, hP=36)


@functools.lru_cache(maxsize=None)
def big_window_case(name):
    """-> (model, buffer, the oracle's hits)"""
    c = BIG_WINDOW
    m = make_model(c["family"], c["depth"], c["n"], c["pos"], window=BIG_WINDOWS[name]["window"], nC=c["nC"])
    chns = rnd(4250, (c["nC"], c["wP"], c["hP"]), 0.0, 0.6)
    chns.setflags(write=False)
    return m, chns, oracle_hits(m, chns)


def big_window_conditions(name):
    m, chns, want = big_window_case(name)
    F, nWr = features(chns, BIG_WINDOWS[name]["window"])
    lv = leaf_values(m, F)
    hit, h, left = evaluate(lv)
    assert same_hits(hit_list(hit, h, nWr), want), name
    assert HIT_LO < hit.sum() / float(len(hit)) < HIT_HI, (name, hit.sum(), len(hit))
    changed = int(evaluate(lv, skip=(15,))[0].sum() - hit.sum())
    assert changed >= MIN_CHANGE, (name, changed)
    return int(hit.sum()), len(hit), changed


# ------------------------------------------------------------------ the pipeline: many levels, many frames, rank cells from the level kernel

PIPE_TREES = 129
PIPE_SIZES = ((96, 128), (96, 96))      # the second: its smallest level is a single window
PIPE_MODELS = (("dip", (0, 16, 32, 47, 64, 96, 127)), ("dip", (15, 31, 48, 63, 95, 128)), ("bump", (0, 16, 32, 47, 64, 96, 127)), ("bump", (15, 31, 48, 63, 95, 128)),
               ("tie", (0, 15, 31, 32, 127, 128)))
PIPE_RUNS = ((1, 1, 0), (1, 1, 8), (2, 0, 8), (2, 1, 0), (5, 0, 0), (5, 1, 8))   # (frames, keep_pyramid, tile_persist)
PIPE_MIN_CHANGE = 8
FRAME_SEED = 71


@functools.lru_cache(maxsize=None)
def pipe_frames(H, W, n=5):
    a = np.stack([synth.make_frame(FRAME_SEED + f, H, W, "luv") for f in range(n)])
    a.setflags(write=False)
    return a


@functools.lru_cache(maxsize=None)
def pipe_case(family, pos, H, W):
    """-> (model, plan, [per frame: dict(pyr, det, hits)]): the family's thresholds are quantiles of the feature's channel in the
    oracle's level 0 of frame 0"""
    from oracle import binding as ob
    base = make_model(family, 2, PIPE_TREES, pos)
    plan0 = ob.Plan(base, H, W, 3)
    pyr0, _, _ = ob.chns_pyramid(plan0, pipe_frames(H, W)[0])
    lvl0 = plan0.level_view(pyr0, 0)
    m = make_model(family, 2, PIPE_TREES, pos, quantile=lambda f, q: float(np.quantile(lvl0[int(f) // 16], q)))
    plan = ob.Plan(m, H, W, 3)
    out = []
    for frame in pipe_frames(H, W):
        pyr, _, _ = ob.chns_pyramid(plan, frame)
        pyr.setflags(write=False)
        det, hits = ob.detect(plan, pyr, cap=1 << 15)
        out.append(dict(pyr=pyr, det=det, hits=hits))
    return m, plan, out


def pipe_leaf_values(m, plan, pyr):
    """-> ([tree][window] over the windows of every level, level by level; per window its (level, rows of windows of the level))"""
    parts, scale, nwr = [], [], []
    for i in range(plan.nScales):
        l = plan.levels[i]
        if l.nWinR <= 0 or l.nWinC <= 0:
            continue
        F, nWr = features(plan.level_view(pyr, i))
        assert nWr == l.nWinR and F.shape[1] == l.nWinR * l.nWinC
        parts.append(leaf_values(m, F))
        scale.append(np.full(F.shape[1], i))
        nwr.append(np.full(F.shape[1], nWr))
    return np.concatenate(parts, axis=1), np.concatenate(scale), np.concatenate(nwr)


def pipe_check_conditions(family, pos, H, W):
    """the restatement equals the oracle's hits on every frame; every position's mutant changes at least PIPE_MIN_CHANGE hits in some frame"""
    m, plan, exp = pipe_case(family, pos, H, W)
    best = {T: 0 for T in pos if family == "tie" or T != PIPE_TREES - 1}   # (a dip or bump on the last tree has no second half)
    for f, e in enumerate(exp):
        lv, scale, nwr = pipe_leaf_values(m, plan, e["pyr"])
        hit, h, left = evaluate(lv)
        idx = np.flatnonzero(hit)
        first = np.concatenate([[0], np.cumsum([(scale == i).sum() for i in range(plan.nScales)])])
        want = e["hits"]
        assert len(idx) == len(want) and len(want) > 0, (family, pos, f, len(idx), len(want))
        loc = idx - first[scale[idx]]
        assert np.array_equal(want["scale"], scale[idx]) and np.array_equal(want["c"], loc // nwr[idx]) and np.array_equal(want["r"], loc % nwr[idx])
        assert np.array_equal(bits(want["score"]), bits(h[idx])), (family, pos, f)
        for T in best:
            if family == "tie":
                ch = evaluate(lv, strict=(T,))[0]
            elif family == "dip":
                ch = evaluate(lv, skip=(T,))[0]
            else:
                ch = evaluate(lv, swap=T)[0]
            best[T] = max(best[T], int((ch != hit).sum()))
    assert all(v >= PIPE_MIN_CHANGE for v in best.values()), (family, pos, H, W, best)
    return best


def pipe_run(family, pos, H, W, n, keep, persist):
    """one pipeline launch on a context, plan and frames of its own: hits and boxes against the oracle as bits.  -> cascade_forms()"""
    import torch
    from acf_amd.detector import HipDetector
    m, plan, exp = pipe_case(family, pos, H, W)
    where = (family, pos, H, W, n, keep, persist)
    pool = torch.from_numpy(np.array(pipe_frames(H, W)[:n])).cuda()
    det = HipDetector()
    try:
        det.set_option("keep_pyramid", keep)
        det.set_option("tile_persist", persist)
        det.set_model(m)
        det.plan(H, W, 3, max_batch=n, max_hits=1 << 14)
        det.run(pool.contiguous(), n)
        rec = det.cascade_forms()
        for f in range(n):
            got, got_hits = det.detections(f)
            want, want_hits = exp[f]["det"], exp[f]["hits"]
            assert len(want_hits) > 0 and len(got_hits) == len(want_hits), where + ("frame", f, len(got_hits), len(want_hits))
            assert same_hits(got_hits, want_hits), where + ("frame", f, "hits differ")
            assert all(np.array_equal(got[k], want[k]) for k in ("x", "y", "w", "h", "scale")) and np.array_equal(bits(got["score"]), bits(want["score"])), where + (f,)
        want_rec = dict(path="tiled2", kernel="tile3", rank=True, frames=n, b=(0, 16, 32, 32, 128), codeScan=True, waveTail=True,
                        persist=bool(persist == 8 and rec["nTiles"] * n > 8))
        check_forms(rec, want_rec, where)
    finally:
        det.close()
    return rec


def record_token(r):
    return "%s:%s:r%d:p%d:NW%d:pw%d:b%s:s%s:f%d:%d%d%d:cap%d" % (r["path"], r["kernel"], r["rank"], r["persist"], r["NW"], r["passW"], ",".join(map(str, r["b"])),
                                                           ",".join(map(str, r["bounds"])), r["firstStage"], r["codeScan"], r["pooledTail"], r["waveTail"], r["codes_cap"])


if __name__ == "__main__":
    # one (depth, length) under the environment the parent set: dips, bumps, ties and the overflow models, every form
    from acf_amd.detector import HipDetector
    depth, n = int(sys.argv[1]), int(sys.argv[2])
    env = " ".join("%s=%s" % (k, os.environ[k]) for k in ("ACF_HIP_FORCE_FALLBACK", "ACF_HIP_CASC_BOUNDS") if k in os.environ)
    dev = HipDetector()
    try:
        cases = group_cases(depth, n) + (overflow_cases(n) if n in OVERFLOW and depth == 2 else [])
        forms = [f for f in forms_of(depth, n) if not f["rank"] or rank_supported(depth, n, env)]
        recs = run_group(dev, depth, n, cases, env, forms)
    finally:
        dev.close()
    print("forms", " ".join(sorted({record_token(r) for r in recs})))
    print("ok", depth, n)
