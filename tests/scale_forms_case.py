"""Shared by tests/test_scale_forms.py (CPU) and tests/test_gpu_scale_forms.py: the forks of the real-scale image resample
(PlanBuild::imageStrips, stripPlan, PyramidRun::imageResample, launchStrip), one case on each side of each, each at the smallest frame
that reaches it.  Every case is synth.make_model(seed=3, name="TINY", nTrees=32, ...) on the frames synth.make_frame(41 + f, H, W, "luv"),
one launch of `n` frames on a context, plan and frames of its own; expected value everywhere: the oracle's chns_pyramid + detect, every
level, hit, box and score compared as bits.  After the comparison the GPU test asserts that HipDetector.scale_forms()
(acf_hip_get_scale_forms) equals what the case names: a case that passes on another route fails.

A case: (fork, model keywords over TINY, H, W, cascThr, run, n, scales)
  run     options set before the plan (scale_streams, fused_smooth), "taps": 1, "env": ACF_HIP_FORCE_FALLBACK names (the case runs in a
          child process, as tests/test_gpu_variants.py's do)
  n       frames in the launch (the plan is made for n)
  scales  one token per real scale, "<h>x<w>:<route>[+slow][+xt2]:<P|-><Q|->:t<nty>:n<nSplit>:<why|->:<why_pair|->": the route
          (HipDetector.SCALE_ROUTES), P / Q = the plan holds a strip plan of the scale alone / with the next scale, nty and nSplit of the
          k_resample_strip launch the scale made (0: none), and why stripPlan refused the plan of the scale alone / of the pair ("-": not
          refused, or not asked).

What the CPU test restates from the oracle's plan for every case (rules(), from the header's description and the issue, not from the
library's output): each real scale's size, source and adoption; which axes go down, up or are exact; the tap counts (level_forms_case's
restated resampleCoef); hence every refusal reason but no_tiling, which plans were asked for, SLOW, xt and — given which plans hold —
the route.  nty, nSplit and no_tiling need the whole tiling; the case states them and the report must agree.

The rules.  Real scale k is resampled from the last adopted scale before it (the frame's own size, or scale 0.5 with nApprox > 0 or
nPerOct 1).  Its image comes, in this order: from the previous scale's smoothing when that scale is its source, it is the exact half
of it and the smoothing is the fused one (HALF_FUSED); from the previous scale's strip pair (PAIR_B); from k_resample_strip when the
plan of the scale alone holds and it is not an exact half — as output A of a pair when the pair's plan holds, the next scale has the
same source, and neither taps nor scale_streams are on; from k_resample_half when it is an exact half; from k_resample_up when both
axes go up and the rows are whole quads; else from the generic k_resample (xt 2 under 4096 blocks).  A pair (k, k + 1) is planned when
k is not adopted, both share the source size, (k - 1, k) holds no pair plan and k + 1 is no larger than k on either axis.

What the cases showed (and DESIGN.md 8 records):
  * An exact half that is not adopted (136 x 200, nApprox 0: scale 8 of scale 0) is never HALF_FUSED, since only the scale right after
    its source can be: it is PAIR_B when (7, 8) is planned and launched, HALF otherwise.
  * A planned pair blocks the next pairing even where it is never launched: at 384 x 384 (2, 3) holds a pair plan, scale 2 is
    HALF_FUSED (the exact half of the adopted scale 1), so the pair is never launched, and (3, 4), of the same source, is not planned
    because (2, 3) holds a plan.  Written down, not changed.
  * Scale 0's size is fitted to both axes at once, so the frames tried here (130..135 x 165..178) round both axes the same way; the
    mixed case is a frame whose rows stay (132 -> 132 takes resampleCoef's up-sampling branch) while its columns go down.
  * The scan (SCAN below): oracle plans of TINY for nPerOct 1..8 x nApprox 0..2 nPerOct x nOctUp 0..1 x H, W in 16, 20, .. 400 (1,505,440
    plans) and again for H, W that are no multiple of 4 (17..399, every third quad: 1,474,560 plans), every asked plan run through a
    stand-alone host build of buildResample + stripPlan.  Reached: not_down, rows (only with a frame that is no multiple of 4),
    slow_taps, x_taps, b_steps and - for pairs only, 7,182 plans of the first grid, the smallest 328 x 64 with nPerOct 6, nApprox 7,
    nOctUp 1 - no_tiling.  Never reached: align (a plan's source planes start at multiples of ha * wa floats and rows comes first) and
    pair_mismatch (imageStrips asks only for scales of one source); the op cannot reach them either, it builds both descriptors from
    one source (UNREACHABLE; the coverage test excludes them).  The plan of a scale alone is never refused by no_tiling.
  * The scan also corrected two beliefs.  k_resample_strip<true, false> IS reachable from the pipeline (55,781 pair plans of the first grid:
    non-default nPerOct with nOctUp 1 gives neighbouring real scales under an octave apart whose B still has at most half of A's
    columns; pair_fast is the smallest, 36 x 40).  And a launched pair can have ntyB < nty (pair_fast_ntyb_below, pair_slow_ntyb_below:
    184 / 176 rows of A in three tiles of 62 / 60, 56 / 52 rows of B in two tiles of 31 / 30).  Octave-apart pairs such as pair_nty4 (84
    rows of A in four tiles of yt = 22, 44 rows of B in four tiles of 11) have ntyB = nty.  The report word carries no ntyB: the CPU test
    derives it from nty by stripPlan's formula (nty_b()) and holds it against PAIR_NTY_B.
  * "Shaped like 1080p": default parameters, a launched pair whose y ratios lie in [1.9, 2) and [3.9, 4.1] and whose B is exactly a
    quarter in x.  The smallest such frame on the grid of multiples of 4 is 156 x 160 (pair_1080p_smallest; the CPU test rescans the
    smaller frames).  pair_slow_* keep 264 x 320, the smallest such frame found with A at least 64 columns wide (two column segments).
  * pair_blocked stands at 384 x 384, not at the 240 x 320 the issue names: with TINY, 240 x 320 has the real scales 120 x 160, 60 x 80
    and 28 x 36, and the pair (2, 3) is refused by x_taps (36 columns from 160, ratio 4.4), so it is never planned.  384 x 384 is the
    smallest frame derived here where (2, 3) holds a plan, scale 2 is HALF_FUSED and a scale 4 of the same source exists.
  * nSplit (n<k> in the tokens, n_split in tests/resample_pair_case.py) comes out of launchStrip's cost model over the device's CU
    count and LDS per CU: the figures stated are the MI355X's (256 CUs, 160 KB) and hold on no other device.  The CPU side bounds them
    by nSteps / 8 only.
  * xt = RS_XT needs 4096 blocks of 64 rows x 8 columns: 8 VGA frames of 3 planes give 8 * 3 * 8 * 20 = 3840 at scale 0's size, and a
    generic scale is smaller than the frame unless it is up-sampled; no case within 8 VGA frames reaches it.  The op runs RS_XT always
    (tests/test_gpu_ops.py test_im_resample).

Hit fractions (windows of every level, the frames of the case together; tests/test_scale_forms.py asserts each strictly inside
(0.05, 0.9)), measured with the oracle at the cascThr listed with each case (chosen per case on the oracle among -0.5, -1, -1.5 and -2
as the value whose fraction lies nearest 0.3: -2 for every case with these 32 trees):
  half_fused 0.182, half_fused_smooth_0 0.182, half_taps 0.182, half_not_adopted 0.203, adopt_nperoct_1 0.188, pair_blocked 0.184,
  strip_fast_b1 0.184, strip_fast_b2 0.187, strip_fast_b5 0.178, x_taps 0.172, pair_slow_b1 0.154, pair_slow_b2 0.183,
  pair_slow_b5 0.195, pair_off_streams 0.183, pair_off_taps 0.183, pair_off_env 0.183, pair_nty4 0.179, up_x2 0.277, up_barely
  0.163, mixed 0.189, env_no_up 0.277, env_generic 0.187, env_no_strip 0.187, env_no_strip_half 0.182, pair_no_tiling 0.257,
  pair_fast 0.172, pair_fast_ntyb_below 0.312, pair_slow_ntyb_below 0.307, pair_1080p_smallest 0.185
"""
import functools
import os
import sys

import numpy as np

if __name__ == "__main__":
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from acf_amd import synth  # noqa: E402

import level_forms_case as lf  # noqa: E402

HIT_LO, HIT_HI = 0.05, 0.9
TINY = dict(seed=3, name="TINY", nTrees=32)
FRAME_SEED = 41
CAP = 1 << 17
ROUTES = ("none", "half_fused", "pair_b", "strip", "strip_pair_a", "half", "up", "generic")
WHYS = ("not_down", "rows", "align", "pair_mismatch", "slow_taps", "x_taps", "b_steps", "no_tiling")
UNREACHABLE = ("align", "pair_mismatch")
REACHED = ("not_down", "rows", "slow_taps", "x_taps", "b_steps", "no_tiling")   # what the scan reached: every one has a case
# the scan's result: plans per grid, and per reason the number of (plan, real scale) refusals of the plan alone / of the pair
SCAN = dict(plans=(1505440, 1474560),
            alone=dict(not_down=1276813 + 1863442, rows=0 + 5149747, align=0, pair_mismatch=0, slow_taps=644499 + 1185, x_taps=1391774 + 10101, b_steps=0, no_tiling=0),
            pair=dict(not_down=1044507 + 1761789, rows=0 + 3776840, align=0, pair_mismatch=0, slow_taps=626405 + 1059, x_taps=1221054 + 8693, b_steps=1461627 + 12248,
                      no_tiling=7182 + 0))
# row tiles of B in the launched pairs (the report has nty only; tests/test_scale_forms.py derives ntyB from it)
PAIR_NTY_B = dict(pair_slow_b1=1, pair_slow_b2=1, pair_slow_b5=1, pair_nty4=4, pair_fast=1, pair_fast_ntyb_below=2, pair_slow_ntyb_below=2, pair_1080p_smallest=1)
RS_XO, RS_XT = 4, 8

# id -> (fork, model keywords, H, W, cascThr, run, n, scales)
CASES = {
    "half_fused": ("the exact half of its source, from the source's fused smoothing",
        {}, 128, 192, -2.0, {}, 2,
        "128x192:none:--:t0:n0:-:- 64x96:half_fused:P-:t0:n0:-:- 28x40:strip:P-:t1:n1:-:-"),
    "half_fused_smooth_0": ("option fused_smooth 0: the same scale through k_resample_half",
        {}, 128, 192, -2.0, {'fused_smooth': 0}, 2,
        "128x192:none:--:t0:n0:-:- 64x96:half:P-:t0:n0:-:- 28x40:strip:P-:t1:n1:-:-"),
    "half_taps": ("taps: no fused smoothing, k_resample_half",
        {}, 128, 192, -2.0, {'taps': 1}, 2,
        "128x192:none:--:t0:n0:-:- 64x96:half:P-:t0:n0:-:- 28x40:strip:P-:t1:n1:-:-"),
    "half_not_adopted": ("nApprox 0: scale 8 is the exact half of scale 0, eight scales after it; every pair refused by b_steps / x_taps / slow_taps",
        {'nApprox': 0}, 136, 200, -2.0, {}, 2,
        "136x200:none:--:t0:n0:-:- 124x184:strip:P-:t1:n5:-:b_steps 116x172:strip:P-:t1:n5:-:b_steps 104x152:strip:P-:t1:n4:-:b_steps 96x140:strip:P-:t1:n4:-:b_steps 88x128:strip:P-:t1:n4:-:b_steps 80x116:strip:P-:t1:n3:-:b_steps 76x112:strip:P-:t1:n3:-:b_steps 68x100:half:P-:t0:n0:-:b_steps 64x96:strip:P-:t1:n3:-:b_steps 56x84:strip:P-:t1:n2:-:b_steps 52x76:strip:P-:t1:n2:-:b_steps 48x72:strip:P-:t1:n2:-:b_steps 44x64:strip:P-:t1:n2:-:b_steps 40x60:strip+slow:P-:t1:n1:-:x_taps 36x52:generic+xt2:--:t0:n0:x_taps:x_taps 32x48:generic+xt2:--:t0:n0:x_taps:x_taps 28x40:generic+xt2:--:t0:n0:x_taps:x_taps 24x36:generic+xt2:--:t0:n0:x_taps:x_taps 20x28:generic+xt2:--:t0:n0:x_taps:slow_taps 16x24:generic+xt2:--:t0:n0:slow_taps:-"),
    "adopt_nperoct_1": ("nApprox 0 with nPerOct 1: scale 0.5 is adopted",
        {'nPerOct': 1, 'nApprox': 0}, 136, 200, -2.0, {}, 2,
        "136x200:none:--:t0:n0:-:- 68x100:half_fused:P-:t0:n0:-:- 36x52:strip:P-:t1:n1:-:x_taps 16x24:generic+xt2:--:t0:n0:x_taps:-"),
    "pair_blocked": ("(2, 3) planned, never launched (2 is HALF_FUSED), and (3, 4) not planned because of it",
        {}, 384, 384, -2.0, {}, 2,
        "384x384:none:--:t0:n0:-:- 192x192:half_fused:P-:t0:n0:-:- 96x96:half_fused:PQ:t0:n0:-:- 48x48:strip:P-:t1:n1:-:- 16x16:generic+xt2:--:t0:n0:slow_taps:-"),
    "strip_fast_b1": ("k_resample_strip<false, false>, 1 frame",
        {}, 200, 264, -2.0, {}, 1,
        "200x264:none:--:t0:n0:-:- 100x132:half_fused:P-:t0:n0:-:- 52x68:strip:P-:t1:n2:-:x_taps 16x20:generic+xt2:--:t0:n0:x_taps:-"),
    "strip_fast_b2": ("k_resample_strip<false, false>, 2 frames",
        {}, 200, 264, -2.0, {}, 2,
        "200x264:none:--:t0:n0:-:- 100x132:half_fused:P-:t0:n0:-:- 52x68:strip:P-:t1:n2:-:x_taps 16x20:generic+xt2:--:t0:n0:x_taps:-"),
    "strip_fast_b5": ("k_resample_strip<false, false>, 5 frames",
        {}, 200, 264, -2.0, {}, 5,
        "200x264:none:--:t0:n0:-:- 100x132:half_fused:P-:t0:n0:-:- 52x68:strip:P-:t1:n2:-:x_taps 16x20:generic+xt2:--:t0:n0:x_taps:-"),
    "x_taps": ("scale 3 at an x ratio of 4.1: refused by x_taps, alone and as B",
        {}, 264, 392, -2.0, {}, 2,
        "264x392:none:--:t0:n0:-:- 132x196:half_fused:P-:t0:n0:-:- 68x100:strip:P-:t1:n3:-:x_taps 32x48:generic+xt2:--:t0:n0:x_taps:-"),
    "pair_slow_b1": ("shaped like 1080p with A 84 columns wide: k_resample_strip<true, true>, 1 frame",
        {}, 264, 320, -2.0, {'scale_streams': 0}, 1,
        "264x320:none:--:t0:n0:-:- 132x160:half_fused:P-:t0:n0:-:- 68x84:strip_pair_a+slow:PQ:t1:n2:-:- 32x40:pair_b:P-:t0:n0:-:-"),
    "pair_slow_b2": ("k_resample_strip<true, true>, 2 frames",
        {}, 264, 320, -2.0, {'scale_streams': 0}, 2,
        "264x320:none:--:t0:n0:-:- 132x160:half_fused:P-:t0:n0:-:- 68x84:strip_pair_a+slow:PQ:t1:n2:-:- 32x40:pair_b:P-:t0:n0:-:-"),
    "pair_slow_b5": ("k_resample_strip<true, true>, 5 frames",
        {}, 264, 320, -2.0, {'scale_streams': 0}, 5,
        "264x320:none:--:t0:n0:-:- 132x160:half_fused:P-:t0:n0:-:- 68x84:strip_pair_a+slow:PQ:t1:n2:-:- 32x40:pair_b:P-:t0:n0:-:-"),
    "pair_off_streams": ("the pair planned but off: scale_streams 1 (the default)",
        {}, 264, 320, -2.0, {}, 2,
        "264x320:none:--:t0:n0:-:- 132x160:half_fused:P-:t0:n0:-:- 68x84:strip:PQ:t1:n2:-:- 32x40:strip+slow:P-:t1:n1:-:-"),
    "pair_off_taps": ("the pair planned but off: taps",
        {}, 264, 320, -2.0, {'scale_streams': 0, 'taps': 1}, 2,
        "264x320:none:--:t0:n0:-:- 132x160:half:P-:t0:n0:-:- 68x84:strip:PQ:t1:n2:-:- 32x40:strip+slow:P-:t1:n1:-:-"),
    "pair_off_env": ("the pair not planned: resample_no_pair",
        {}, 264, 320, -2.0, {'scale_streams': 0, 'env': 'resample_no_pair'}, 2,
        "264x320:none:--:t0:n0:-:- 132x160:half_fused:P-:t0:n0:-:- 68x84:strip:P-:t1:n2:-:- 32x40:strip+slow:P-:t1:n1:-:-"),
    "pair_nty4": ("a pair of four row tiles",
        {}, 344, 320, -2.0, {'scale_streams': 0}, 2,
        "344x320:none:--:t0:n0:-:- 172x160:half_fused:P-:t0:n0:-:- 84x80:strip_pair_a+slow:PQ:t4:n2:-:- 44x40:pair_b:P-:t0:n0:-:-"),
    "pair_no_tiling": ("a pair refused by no_tiling: 268 and 80 rows from 656, no row tiling fits both outputs",
        {'nPerOct': 6, 'nApprox': 7, 'nOctUp': 1}, 328, 64, -2.0, {}, 2,
        "656x128:up:--:t0:n0:not_down:not_down 268x52:strip:P-:t2:n1:-:no_tiling 80x16:strip+slow:P-:t2:n1:-:-"),
    "pair_fast": ("k_resample_strip<true, false> from the pipeline: neither output above four y taps; B one step short of A",
        {'nPerOct': 7, 'nApprox': 3, 'nOctUp': 1}, 36, 40, -2.0, {'scale_streams': 0}, 2,
        "72x80:up:--:t0:n0:not_down:not_down 48x52:up:--:t0:n0:not_down:not_down 32x36:strip_pair_a:PQ:t1:n1:-:- 16x16:pair_b:P-:t0:n0:-:-"),
    "pair_fast_ntyb_below": ("<true, false> with three row tiles of A and two of B",
        {'nPerOct': 7, 'nApprox': 7, 'nOctUp': 1}, 196, 56, -2.0, {'scale_streams': 0}, 2,
        "392x112:up:--:t0:n0:not_down:not_down 184x52:strip_pair_a:PQ:t3:n1:-:- 56x16:pair_b:P-:t0:n0:-:-"),
    "pair_slow_ntyb_below": ("<true, true> with three row tiles of A and two of B",
        {'nPerOct': 7, 'nApprox': 7, 'nOctUp': 1}, 188, 56, -2.0, {'scale_streams': 0}, 2,
        "376x112:up:--:t0:n0:not_down:not_down 176x52:strip_pair_a+slow:PQ:t3:n1:-:- 52x16:pair_b:P-:t0:n0:-:-"),
    "pair_1080p_smallest": ("the smallest frame whose pair has 1080p's ratios (y 1.95 and 3.9, x 1.9 and exactly 4)",
        {}, 156, 160, -2.0, {'scale_streams': 0}, 2,
        "156x160:none:--:t0:n0:-:- 80x84:strip_pair_a+slow:PQ:t1:n2:-:- 40x40:pair_b:P-:t0:n0:-:-"),
    "up_x2": ("nOctUp 1: scale 0 is twice the frame",
        {'nOctUp': 1}, 64, 96, -2.0, {}, 2,
        "128x192:up:--:t0:n0:not_down:- 64x96:none:--:t0:n0:-:- 28x40:strip:P-:t1:n1:-:-"),
    "up_barely": ("130 x 175 -> 132 x 176; the smaller scales' source has 130 rows: rows",
        {}, 130, 175, -2.0, {}, 2,
        "132x176:up:--:t0:n0:not_down:not_down 64x88:generic+xt2:--:t0:n0:rows:rows 28x36:generic+xt2:--:t0:n0:rows:-"),
    "mixed": ("132 x 170 -> 132 x 168: y unchanged (resampleCoef's up-sampling branch), x down",
        {}, 132, 170, -2.0, {}, 2,
        "132x168:generic+xt2:--:t0:n0:not_down:not_down 68x88:strip:P-:t1:n2:-:x_taps 32x40:generic+xt2:--:t0:n0:x_taps:-"),
    "env_no_up": ("resample_no_up: the up-sampled scale through k_resample",
        {'nOctUp': 1}, 64, 96, -2.0, {'env': 'resample_no_up'}, 2,
        "128x192:generic+xt2:--:t0:n0:not_down:- 64x96:none:--:t0:n0:-:- 28x40:strip:P-:t1:n1:-:-"),
    "env_generic": ("resample_generic: the strip scale through k_resample, its plan still held",
        {}, 200, 264, -2.0, {'env': 'resample_generic'}, 2,
        "200x264:none:--:t0:n0:-:- 100x132:half_fused:P-:t0:n0:-:- 52x68:generic+xt2:P-:t0:n0:-:x_taps 16x20:generic+xt2:--:t0:n0:x_taps:-"),
    "env_no_strip": ("resample_no_strip: no plan asked for",
        {}, 200, 264, -2.0, {'env': 'resample_no_strip'}, 2,
        "200x264:none:--:t0:n0:-:- 100x132:half_fused:--:t0:n0:-:- 52x68:generic+xt2:--:t0:n0:-:- 16x20:generic+xt2:--:t0:n0:-:-"),
    "env_no_strip_half": ("resample_no_strip with fused_smooth 0: k_resample_half",
        {}, 128, 192, -2.0, {'env': 'resample_no_strip', 'fused_smooth': 0}, 2,
        "128x192:none:--:t0:n0:-:- 64x96:half:--:t0:n0:-:- 28x40:generic+xt2:--:t0:n0:-:-"),
}


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def parse_scales(case):
    """-> [dict(h, w) + the keys of HipDetector.scale_forms()] of the case's tokens"""
    out = []
    for tok in CASES[case][7].split():
        size, route, plans, nty, nsplit, why, why_pair = tok.split(":")
        h, w = (int(v) for v in size.split("x"))
        route, *flags = route.split("+")
        assert route in ROUTES and set(flags) <= {"slow", "xt2"} and nty[0] == "t" and nsplit[0] == "n", tok
        out.append(dict(h=h, w=w, route=route, slow="slow" in flags, xt2="xt2" in flags, plan_strip=plans[0] == "P", plan_pair=plans[1] == "Q",
                        nty=int(nty[1:]), n_split=int(nsplit[1:]), why=None if why == "-" else why, why_pair=None if why_pair == "-" else why_pair))
    return out


def expect(case):
    """what scale_forms() must report"""
    return [{k: v for k, v in s.items() if k not in ("h", "w")} for s in parse_scales(case)]


@functools.lru_cache(maxsize=None)
def model(case):
    return synth.make_model(**dict(TINY, cascThr=CASES[case][4], **CASES[case][1]))


@functools.lru_cache(maxsize=None)
def frames(H, W, n):
    a = np.stack([synth.make_frame(FRAME_SEED + f, H, W, "luv") for f in range(n)])
    a.setflags(write=False)
    return a


def case_frames(case):
    return frames(CASES[case][2], CASES[case][3], CASES[case][6])


@functools.lru_cache(maxsize=None)
def oracle_plan(case):
    from oracle import binding as ob
    return ob.Plan(model(case), CASES[case][2], CASES[case][3], 3)


@functools.lru_cache(maxsize=None)
def expected(case):
    """-> (plan, [per frame: dict(pyr, det, hits)]) from the oracle.  Read-only, shared."""
    from oracle import binding as ob
    plan = oracle_plan(case)
    out = []
    for frame in case_frames(case):
        pyr, _, _ = ob.chns_pyramid(plan, frame)
        pyr.setflags(write=False)
        det, hits = ob.detect(plan, pyr, cap=CAP)
        out.append(dict(pyr=pyr, det=det, hits=hits))
    return plan, out


def n_windows(case):
    plan = oracle_plan(case)
    return sum(max(plan.levels[i].nWinR, 0) * max(plan.levels[i].nWinC, 0) for i in range(plan.nScales))


def hit_fraction(case):
    _, exp = expected(case)
    return sum(len(e["hits"]) for e in exp) / float(len(exp) * n_windows(case))


# ------------------------------------------------------------------ the rules, restated (the CPU test holds every case against them)

def real_scales(plan, m, H, W):
    """the real scales of the oracle's plan with the reference's I = I1 bookkeeping (chnsPyramid.cpp:297-338): size, whether the
    scale is resampled at all, whether its smoothed image is adopted as the source of the following scales, and its source"""
    out = []
    cur, cur_idx = (H, W), -1
    for i in plan.real:
        l = plan.levels[i]
        h, w = l.hC * m["shrink"], l.wC * m["shrink"]
        same = (h, w) == (H, W)
        adopt = same or (l.scale == 0.5 and (m["nApprox"] > 0 or m["nPerOct"] == 1))
        out.append(dict(h=h, w=w, scale=l.scale, resampled=not same, adopt=adopt, src=cur_idx, src_h=cur[0], src_w=cur[1]))
        if adopt:
            cur, cur_idx = (h, w), len(out) - 1
    return out


def axes(s):
    """((kind, taps) of y, (kind, taps) of x) of a real scale's resample: kind "exact" (1/2, 1/3, 1/4), "down" or "up" (equal sizes go "up")"""
    return lf.axis_taps(s["src_h"], s["h"]), lf.axis_taps(s["src_w"], s["w"])


def cheap_reason(a, b=None):
    """stripPlan's refusal of scale a alone (b None) or of the pair (a, b), in its order, as far as tap counts tell: not_down, rows,
    slow_taps (more than 8 y taps; the taps of a row are consecutive source rows, so none lies further than 15 from the first unless
    there are more than 8), x_taps, b_steps.  None: not refused, or no_tiling."""
    both = [s for s in (a, b) if s is not None]
    ax = [axes(s) for s in both]
    if any(k == "up" for yx in ax for k, _ in yx):
        return "not_down"
    if a["src_h"] % 4 or a["src_h"] < 8:
        return "rows"
    if any(y[0] == "down" and y[1] > 8 for y, _ in ax):
        return "slow_taps"
    if any(x[0] == "down" and x[1] > 4 for _, x in ax):
        return "x_taps"
    if b is not None and -(-b["w"] // (RS_XO // 2)) > -(-a["w"] // RS_XO):
        return "b_steps"
    return None


def nty_b(a, b, nty):
    """B's row tiles beside nty row tiles of A, by stripPlan's formula: a tile holds an even number yt of A's rows and yt / 2 of B's"""
    yt = (-(-a["h"] // nty) + 1) // 2 * 2
    assert -(-a["h"] // yt) == nty
    return -(-b["h"] // (yt // 2))


def is_slow(s):
    y, _ = axes(s)
    return y[0] == "down" and y[1] > 4


def exact_half(s):
    y, x = axes(s)
    return (y[0] == "exact" and x[0] == "exact" and s["src_h"] == 2 * s["h"] and s["src_w"] == 2 * s["w"] and s["src_h"] % 4 == 0 and s["h"] % 2 == 0)


def rules(case):
    """-> per real scale dict(route, slow, xt2, asked, asked_pair, cheap, cheap_pair): what the rules in the module's docstring give for
    the case, taking from the case's tokens only which plans hold (P / Q)"""
    _, kw, H, W, _, run, n, _ = CASES[case]
    m = model(case)
    rs = real_scales(oracle_plan(case), m, H, W)
    tok = parse_scales(case)
    env = set(run.get("env", "").split(",")) - {""}
    taps = bool(run.get("taps", 0))
    streams = bool(run.get("scale_streams", 1)) and len(rs) > 1 and not taps
    fuse_sm = m["colorSmooth"] > 0 and m["colorEnabled"] and not taps and bool(run.get("fused_smooth", 1)) and m["shrink"] == 4
    out = []
    pair_done = False
    for k, s in enumerate(rs):
        r = dict(route="none", slow=False, xt2=False, asked=False, asked_pair=False, cheap=None, cheap_pair=None)
        out.append(r)
        if not s["resampled"]:
            pair_done = False
            continue
        nxt = rs[k + 1] if k + 1 < len(rs) else None
        r["asked"] = "resample_no_strip" not in env
        r["asked_pair"] = bool(r["asked"] and "resample_no_pair" not in env and nxt is not None and nxt["resampled"] and not s["adopt"] and
                               (s["src_h"], s["src_w"]) == (nxt["src_h"], nxt["src_w"]) and not (k > 0 and tok[k - 1]["plan_pair"]) and
                               nxt["w"] <= s["w"] and nxt["h"] <= s["h"])
        r["cheap"] = cheap_reason(s) if r["asked"] else None
        r["cheap_pair"] = cheap_reason(s, nxt) if r["asked_pair"] else None
        prev = rs[k - 1] if k > 0 else None
        half = exact_half(s)
        generic_only = "resample_generic" in env
        y, x = axes(s)
        was_pair_b, pair_done = pair_done, False
        if prev is not None and s["src"] == k - 1 and half and fuse_sm and prev["w"] >= 16:
            r["route"] = "half_fused"
        elif was_pair_b:
            r["route"] = "pair_b"
        elif tok[k]["plan_strip"] and not half and not generic_only:
            pair = tok[k]["plan_pair"] and nxt is not None and nxt["src"] == s["src"] and not taps and not streams
            r["route"] = "strip_pair_a" if pair else "strip"
            r["slow"] = is_slow(s) or (pair and is_slow(nxt))
            pair_done = pair
        elif half:
            r["route"] = "half"
        elif y[0] == "up" and x[0] == "up" and s["h"] % 4 == 0 and s["src_h"] >= 4 and not generic_only and "resample_no_up" not in env:
            r["route"] = "up"
        else:
            r["route"] = "generic"
            r["xt2"] = -(-s["h"] // 64) * -(-s["w"] // (4 * RS_XT)) * 3 * n < 4096
    return out


# ------------------------------------------------------------------ the GPU side (tests/test_gpu_scale_forms.py; a child process for "env")

def compare(det, case):
    plan, exp = expected(case)
    for f, e in enumerate(exp):
        where = (case, "frame", f)
        for i in range(plan.nScales):
            assert np.array_equal(bits(det.read_level(f, i)), bits(plan.level_view(e["pyr"], i))), where + ("pyramid level", i)
        got, got_hits = det.detections(f)
        want, want_hits = e["det"], e["hits"]
        assert len(want_hits) > 0, where
        assert len(got_hits) == len(want_hits) and len(got) == len(want), where + (len(got_hits), len(want_hits))
        for key in ("scale", "c", "r"):
            assert np.array_equal(got_hits[key], want_hits[key]), where + ("hits", key)
        assert np.array_equal(bits(got_hits["score"]), bits(want_hits["score"])), where + ("hit scores",)
        for key in ("x", "y", "w", "h", "scale"):
            assert np.array_equal(got[key], want[key]), where + ("detections", key)
        assert np.array_equal(bits(got["score"]), bits(want["score"])), where + ("detection scores",)


def check_forms(case, forms):
    want = expect(case)
    assert len(forms) == len(want), (case, len(forms), len(want))
    for k, (g, w) in enumerate(zip(forms, want)):
        assert g == w, (case, "real scale", k, g, w)


def run_case(case):
    """the case's launch on a context of its own: compare with the oracle, then assert the forms.  -> the reported forms"""
    import torch
    from acf_amd.detector import HipDetector
    _, kw, H, W, _, run, n, _ = CASES[case]
    _, exp = expected(case)
    max_hits = max(1 << 14, 2 * max(len(e["hits"]) for e in exp))
    pool = torch.from_numpy(np.array(case_frames(case))).cuda()
    det = HipDetector(taps=bool(run.get("taps", 0)))
    try:
        for k, v in run.items():
            if k not in ("taps", "env"):
                det.set_option(k, v)
        det.set_model(model(case))
        det.plan(H, W, 3, max_batch=n, max_hits=max_hits)
        before = det.scale_forms()
        det.run(pool.contiguous(), n)
        forms = det.scale_forms()
        print(case, " ".join(form_token(f) for f in forms))
        # the comparison first, then the form; a wrong form is reported even where the comparison has failed already
        errs = []
        for check in (lambda: compare(det, case), lambda: check_forms(case, forms), lambda: check_before(case, before)):
            try:
                check()
            except AssertionError as e:
                errs.append(e)
        assert not errs, errs
    finally:
        det.close()
    return forms


def check_before(case, before):
    """the query on a plan that has not run: the plan's side as after the run, the run's side zero"""
    want = [dict(w, route="none", slow=False, xt2=False, nty=0, n_split=0) for w in expect(case)]
    assert before == want, (case, "before the first call", before, want)


def form_token(f):
    return "%s%s%s:%s%s:t%d:n%d:%s:%s" % (f["route"], "+slow" if f["slow"] else "", "+xt2" if f["xt2"] else "", "P" if f["plan_strip"] else "-",
                                         "Q" if f["plan_pair"] else "-", f["nty"], f["n_split"], f["why"] or "-", f["why_pair"] or "-")


if __name__ == "__main__":
    print("forms", sys.argv[1], " ".join(form_token(f) for f in run_case(sys.argv[1])))
    print("ok", sys.argv[1])
