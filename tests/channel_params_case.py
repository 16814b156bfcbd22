"""Shared by tests/test_channel_params.py (CPU) and tests/test_gpu_channel_params.py: the planned pipeline away from the default
channel parameters.  Every case is one departure (or one small group) from normRad 5 / normConst 0.005 / nOrients 6 / smooth 1 /
colorSmooth 1 / all three channel kinds enabled, on synth.make_model(seed=3, name="TINY", nTrees=64, cascThr=-2.0) and the frames
synth.make_frame(17 + f, H, W, "luv").  Expected value everywhere: the oracle's chns_pyramid + detect (ldcf + detect_ldcf for the
LDCF case), compared as bits.

The three sizes: 128 x 192 (every real scale takes the vector forms), 130 x 175 (the image is resampled first; scalar forms) and
240 x 320 (scales at least 48 wide and tall, which the fused y pass and the x pass on the smoothing chain require).

A cascade comparison checks something only if a fair share of the windows passes and a fair share is rejected: the fraction of
windows (all levels, nWinR x nWinC each) that the oracle reports as hits must lie strictly inside (0.05, 0.9) for every case at
every size (asserted by tests/test_channel_params.py).  Measured with the oracle, frames 17 and 18 together:
0.093 (normRad=0 at 240 x 320) .. 0.709 (nOrients=1 at 130 x 175) over the TINY cases, 0.415 .. 0.517 for the LDCF case and 0.293
for FACE80 (cascThr of the last two: see LDCF_CASCTHR, FACE80_CASCTHR).
"""
import functools

import numpy as np

from acf_amd import synth

SIZES = [(128, 192), (130, 175), (240, 320)]
N_FRAMES = 2
HIT_LO, HIT_HI = 0.05, 0.9

TINY = dict(seed=3, name="TINY", nTrees=64, cascThr=-2.0)
# cascThr of the two cases that are not TINY's window: chosen on the oracle so that the hit fraction lies inside (0.05, 0.9)
# (LDCF: 0.42 .. 0.52 at -2, 0.99 at -3; FACE80 with 300 trees: 0.016 at -3, 0.29 at -4, 0.87 at -5)
LDCF_CASCTHR, FACE80_CASCTHR = -2.0, -4.0
CAP = 1 << 18   # hits per frame the oracle's lists and the plan hold (nOctUp=2 at 240 x 320: 66 k per frame)
_LDCF32 = dict(modelDs_h=32, modelDs_w=32, modelDsPad_h=32, modelDsPad_w=32, minDs_h=32, minDs_w=32)

# id -> (make_model keywords over TINY, sizes)
CASES = {"baseline": ({}, SIZES)}
for _r in (0, 2, 3, 4, 6, 7):
    CASES["normRad%d" % _r] = (dict(normRad=_r), SIZES)
CASES.update({
    "normRad15": (dict(normRad=15, minDs_h=48, minDs_w=48), SIZES),   # (2 * 15 + 1 pixels: a smaller minDs is refused)
    "normConst0.02": (dict(normConst=0.02), SIZES),
    "smooth0": (dict(smooth=0), SIZES),
    "smooth0.5": (dict(smooth=0.5), SIZES),
    "colorSmooth0": (dict(colorSmooth=0), SIZES),
    "colorSmooth0.5": (dict(colorSmooth=0.5), SIZES),
    "smooth0_colorSmooth0": (dict(smooth=0, colorSmooth=0), SIZES),
    "nOrients1": (dict(nOrients=1), SIZES),
    "nOrients4": (dict(nOrients=4), SIZES),
    "nOrients7": (dict(nOrients=7), SIZES),
    "nOrients12": (dict(nOrients=12), SIZES),
    "nOrients5_full": (dict(nOrients=5, full=1), SIZES),
    "nOrients9_full": (dict(nOrients=9, full=1), SIZES),
    "nOrients12_hardbin": (dict(nOrients=12, softBin=-2), SIZES),
    "no_color": (dict(colorEnabled=0), SIZES),
    "no_mag": (dict(gradMagEnabled=0), SIZES),
    "no_hist": (dict(gradHistEnabled=0), SIZES),
    "color_only": (dict(gradMagEnabled=0, gradHistEnabled=0), SIZES),
    "hist_only": (dict(colorEnabled=0, gradMagEnabled=0), SIZES),
    "mag_only": (dict(colorEnabled=0, gradHistEnabled=0), SIZES),
    "shrink2_normRad3_nOrients9": (dict(shrink=2, stride=2, normRad=3, nOrients=9), SIZES),
    "nOctUp2": (dict(nOctUp=2), SIZES),
    "colorChn2_normRad3": (dict(colorChn=2, normRad=3), SIZES),
    # the LDCF post-stage on 13 channels x 2 filters
    "ldcf_k2_nOrients9": (dict(ldcfK=2, nOrients=9, cascThr=LDCF_CASCTHR, **_LDCF32), SIZES),
    # a 20 x 20 x 16 window in the tile kernel
    "face80_nOrients12": (dict(name="FACE80", nOrients=12, nTrees=300, cascThr=FACE80_CASCTHR), [(240, 320)]),
})

# the cases option set 7 (the reference's rcpps / rsqrtps bits, option arith) runs
ARITH_CASES = ("normRad3", "nOrients12", "normConst0.02")


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def is_ldcf(case):
    return "ldcfK" in CASES[case][0]


@functools.lru_cache(maxsize=None)
def model(case):
    return synth.make_model(**dict(TINY, **CASES[case][0]))


@functools.lru_cache(maxsize=None)
def frames(H, W):
    a = np.stack([synth.make_frame(17 + f, H, W, "luv") for f in range(N_FRAMES)])
    a.setflags(write=False)
    return a


def _oracle_pyramid(case, H, W, frame, approx, want):
    from oracle import binding as ob
    plan = ob.Plan(model(case), H, W, 3)
    if approx:
        ob.set_x86_tables(*ob.x86_fixture())
    ob.set_approx(approx)
    try:
        return (plan,) + ob.chns_pyramid(plan, frame, want_taps=want, want_chns=want)
    finally:
        ob.set_approx(0)


@functools.lru_cache(maxsize=None)
def expected(case, H, W, approx=0):
    """-> (plan, [per frame: dict(pyr, det, hits, ldcf)]) from the oracle; approx 3: under set_approx(3) with the committed x86
    tables (option arith's yardstick).  Computed once per process and shared by the tests: read-only."""
    from oracle import binding as ob
    out = []
    for frame in frames(H, W):
        plan, pyr, _, _ = _oracle_pyramid(case, H, W, frame, approx, False)
        pyr.setflags(write=False)
        e = dict(pyr=pyr, ldcf=None)
        if is_ldcf(case):
            lvL, pyrL, k = ob.ldcf(plan, pyr)
            e["ldcf"] = (lvL, pyrL, k)
            e["det"], e["hits"] = ob.detect_ldcf(plan, lvL, pyrL, cap=CAP)
        else:
            e["det"], e["hits"] = ob.detect(plan, pyr, cap=CAP)
        out.append(e)
    return plan, out


def expected_taps(case, H, W, f):
    """-> (taps per real scale, raw channels per level) of frame f: the stage outputs, not kept (they are large)."""
    _, _, taps, chns = _oracle_pyramid(case, H, W, frames(H, W)[f], 0, True)
    return taps, chns


def n_windows(case, H, W):
    plan, exp = expected(case, H, W)
    lv = exp[0]["ldcf"][0] if is_ldcf(case) else plan.levels
    return sum(max(lv[i].nWinR, 0) * max(lv[i].nWinC, 0) for i in range(plan.nScales))


def hit_fraction(case, H, W):
    _, exp = expected(case, H, W)
    return sum(len(e["hits"]) for e in exp) / float(N_FRAMES * n_windows(case, H, W))
