"""Cases of tests/test_gpu_rank_diet.py: the level kernels' rank cells (record encoding, clamp, negative cells with and without a
zero threshold) and their first / last column, on inputs chosen for them.  Expected values: the oracle's chns_pyramid + detect.

Rank cases (RANK_CASES): a model x a frame size x a frame set, each a batch of 5 (one full group of four frames per workgroup and a
partial one), run with keep_pyramid 1 and 0.
  models   tiny   synth TINY, 256 trees
           zero   tiny with the threshold 0.0 on the first twelve nodes of channel 0 (colour L) and of channel 5 (a histogram bin):
                  the forms that put a negative cell below a zero threshold (RankTables::hasZero)
           cells  TINY, 2304 trees (every channel has at least 600 nodes), every threshold one of the oracle's own cells of the
                  size's synthetic frames or one of its two float neighbours: equality and neighbouring floats on the device,
                  records with six and seven slots in use.  The cells are drawn per channel between its positive cells' median and
                  twice the median, at most two per 2^13 consecutive float patterns (two triples of thresholds: a table of at most
                  1027 buckets always exists)
  sizes    128 x 192 (levels of 32 .. 8 rows, 48 .. 12 columns), 130 x 175 (odd sizes: 43 columns)
  frames   a   synth.make_frame(61 + k, H, W, "luv"), k = 0 .. 4
           b   the same minus 0.5: every colour cell is negative
           c   an all-zero frame, a frame of -0.0, a[0], b[1], the frame of -0.0 again (the zero frames alone would have no window or
               every window as a hit: the set has both kinds of frame so that its hit fraction says something)
Hit fractions over the set's five frames at the model's cascThr (oracle; asserted inside (0.05, 0.9) by the CPU test, which prints
them): see test_gpu_rank_diet.py's docstring.

Edge cases (EDGE_SIZES): frames of 128 x 64, 120 x 72 and 128 x 96, TINY with 32 trees (tests/level_forms_case.py's model), batch 1, keep_pyramid 1, with
the default options and with level_segments 3 + level_warm 4 (every level of 16 columns and more is cut in two or three).  The sizes
are chosen (W from 64 .. 96) so that every level of each plan can be fused (no reason of tests/level_forms_case.py's level_reasons)
and the real levels' widths in cells and the approximated levels' are each 0, 1, 2 and 3 modulo 4 (the main loop takes four columns
per trip: every tail length, on both kinds of level); the CPU test asserts both from the plan.
"""
import functools

import numpy as np

from acf_amd import synth

import level_forms_case as lf

HIT_LO, HIT_HI = lf.HIT_LO, lf.HIT_HI
SIZES = ((128, 192), (130, 175))
SETS = ("a", "b", "c")
MODELS = ("tiny", "zero", "cells")
# cascThr per (model, frame set), chosen on the oracle among -2, -2.5, -3, -3.5, -4 as the value whose hit fraction lies nearest 0.3
# with both sizes inside the window
CASC_THR = {("tiny", "a"): -2.0, ("tiny", "b"): -2.5, ("tiny", "c"): -2.5, ("zero", "a"): -2.0, ("zero", "b"): -3.0, ("zero", "c"): -2.5,
            ("cells", "a"): -3.0, ("cells", "b"): -3.5, ("cells", "c"): -4.0}
RANK_CASES = [(m, H, W, s) for m in MODELS for (H, W) in SIZES for s in SETS]
EDGE_SIZES = ((128, 64), (120, 72), (128, 96))   # real levels of 16 and 7, 18 and 9, 24, 12 and 4 columns
EDGE_RUNS = ({}, {"level_segments": 3, "level_warm": 4})
N_CHNS = 10
CAP = 1 << 17


@functools.lru_cache(maxsize=None)
def frame_set(H, W, s):
    a = [synth.make_frame(61 + k, H, W, "luv") for k in range(5)]
    if s == "a":
        out = a
    elif s == "b":
        out = [(f - np.float32(0.5)).astype(np.float32) for f in a]
    else:
        zero = np.zeros_like(a[0])
        out = [zero, -zero, a[0], (a[1] - np.float32(0.5)).astype(np.float32), -zero]
        assert np.signbit(out[1]).all() and not np.signbit(out[0]).any()
    out = np.stack(out)
    out.setflags(write=False)
    return out


def _chn_of_nodes(m):
    mH, mW = m["modelDsPad_h"] // m["shrink"], m["modelDsPad_w"] // m["shrink"]
    return m["fids"][:, :3] // (mH * mW)


def model(name, H, W, s):
    """the case's model: base_model with the case's cascThr"""
    return dict(base_model(name, H, W), cascThr=CASC_THR[name, s])


@functools.lru_cache(maxsize=None)
def base_model(name, H, W):
    if name == "tiny":
        return synth.make_model(seed=3, name="TINY", nTrees=256)
    if name == "zero":
        m = synth.make_model(seed=3, name="TINY", nTrees=256)
        thrs = m["thrs"].copy()
        ch = _chn_of_nodes(m)
        for z in (0, 5):
            t, k = np.nonzero(ch == z)
            thrs[t[:12], k[:12]] = 0.0
        return dict(m, thrs=thrs)
    # cells: thresholds from the oracle's own cells of the size's synthetic frames
    from oracle import binding as ob
    m = synth.make_model(seed=3, name="TINY", nTrees=2304)
    plan = ob.Plan(m, H, W, 3)
    pyrs = [ob.chns_pyramid(plan, f)[0] for f in frame_set(H, W, "a")]
    thrs = m["thrs"].copy()
    ch = _chn_of_nodes(m)
    f32 = np.float32
    for z in range(N_CHNS):
        cells = np.concatenate([plan.level_view(p, i)[z].ravel() for p in pyrs for i in range(plan.nScales)])
        cells = np.unique(cells[cells > 0])
        med = cells[len(cells) // 2]
        cells = cells[(cells >= med) & (cells < 2 * med)]
        cells = cells[np.r_[True, np.diff(cells.view(np.uint32).astype(np.int64)) > 2]]  # no two triples share a float
        # at most two cells per 2^13 float patterns, spread over the range
        bucket = cells.view(np.uint32) >> 13
        first = np.nonzero(np.r_[True, bucket[1:] != bucket[:-1]])[0]
        second = first + 1
        second = second[(second < len(cells))]
        second = second[bucket[second] == bucket[second - 1]]
        pick = np.sort(np.r_[first, second])
        cells = cells[pick]
        t, k = np.nonzero(ch == z)
        assert len(t) >= 600, (z, len(t))
        n = -(-len(t) // 3)
        assert len(cells) >= n, (z, len(cells), n)
        cells = cells[(np.arange(n) * len(cells)) // n]
        tri = np.stack([np.nextafter(cells, f32(-np.inf)), cells, np.nextafter(cells, f32(np.inf))], axis=1).ravel()[:len(t)]
        assert (tri > 0).all()
        thrs[t, k] = tri.astype(np.float32)
    return dict(m, thrs=thrs)


@functools.lru_cache(maxsize=None)
def expected(name, H, W, s):
    """-> (plan, [per frame: dict(pyr, det, hits)]).  Read-only, shared."""
    from oracle import binding as ob
    plan = ob.Plan(model(name, H, W, s), H, W, 3)
    out = []
    for frame in frame_set(H, W, s):
        pyr, _, _ = ob.chns_pyramid(plan, frame)
        pyr.setflags(write=False)
        det, hits = ob.detect(plan, pyr, cap=CAP)
        out.append(dict(pyr=pyr, det=det, hits=hits))
    return plan, out


def n_windows(plan):
    return sum(max(plan.levels[i].nWinR, 0) * max(plan.levels[i].nWinC, 0) for i in range(plan.nScales))


def hit_fraction(plan, exp):
    return sum(len(e["hits"]) for e in exp) / float(len(exp) * n_windows(plan))


# ---- edge columns

@functools.lru_cache(maxsize=None)
def edge_model():
    return synth.make_model(**dict(lf.TINY, cascThr=-2.0))


@functools.lru_cache(maxsize=None)
def edge_expected(H, W):
    from oracle import binding as ob
    plan = ob.Plan(edge_model(), H, W, 3)
    frame = synth.make_frame(lf.FRAME_SEED, H, W, "luv")
    pyr, _, _ = ob.chns_pyramid(plan, frame)
    pyr.setflags(write=False)
    det, hits = ob.detect(plan, pyr, cap=CAP)
    return plan, frame, dict(pyr=pyr, det=det, hits=hits)


# ---- the GPU side

def compare(det, m, plan, e, f, where, floats):
    """slot f of the last run against the oracle: rank cells of every level (padded border included), floats where kept, hits, scores, boxes"""
    for i in range(plan.nScales):
        want = plan.level_view(e["pyr"], i)
        assert np.array_equal(det.read_rank_level(f, i), lf.ranks_of(m, plan.nChns, want)), where + ("rank level", i)
        if floats:
            assert np.array_equal(lf.bits(det.read_level(f, i)), lf.bits(want)), where + ("pyramid level", i)
    got, got_hits = det.detections(f)
    want, want_hits = e["det"], e["hits"]
    assert len(got_hits) == len(want_hits) and len(got) == len(want), where + (len(got_hits), len(want_hits))
    for key in ("scale", "c", "r"):
        assert np.array_equal(got_hits[key], want_hits[key]), where + ("hits", key)
    assert np.array_equal(lf.bits(got_hits["score"]), lf.bits(want_hits["score"])), where + ("hit scores",)
    for key in ("x", "y", "w", "h", "scale"):
        assert np.array_equal(got[key], want[key]), where + ("detections", key)
    assert np.array_equal(lf.bits(got["score"]), lf.bits(want["score"])), where + ("detection scores",)
