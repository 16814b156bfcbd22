"""Shared by tests/test_level_forms.py (CPU) and tests/test_gpu_level_forms.py: the level stage's plan-time decisions
(PlanBuild::levelJobs, PyramidRun::planLevels), one case on each side of every fork, each at the smallest geometry that reaches it.
Every case is synth.make_model(seed=3, name="TINY", nTrees=32, ...) on the frames synth.make_frame(41 + f, H, W, "luv"), launch k
of the case taking frames k, k + 1, ... in slots 0, 1, ...; expected value everywhere: the oracle's chns_pyramid + detect, compared as bits.  After the comparison the GPU test asserts from
HipDetector.level_forms() (acf_hip_get_level_forms) that the call took the form the case names: a case that passes on another form fails.

A case: (fork, model keywords over TINY, H, W, cascThr, run, path, approx_first, levels)
  run     options set before the plan (fused_levels, level_segments, keep_pyramid, rank_cells; every launch plans on a context of its
          own and takes frames of its own, see launches()), "taps": 1 (the plan holds the taps and
          the raw channels are compared through TAP_CHNS), "env": ACF_HIP_FORCE_FALLBACK names (the case runs in a child process, as
          tests/test_gpu_variants.py's do), "batches": the batch sizes to run (default: (2,))
  path    "fused" / "wave_smooth" / "smooth_jobs" / "copy", approx_first: k_resample(approx) runs in front
  levels  one token per level, "<hC><r|a>:<mode><taker>[!why,...]": r a real level, a an approximated one; mode as REPORTED, r = LM_REAL,
          d = LM_DD, u = LM_UU, x = LM_DU, y = LM_UD (under wave_smooth every level is smoothed from its raw channels: r); taker A =
          k_level_all, G = a k_level<R, mode> group launch, - = no level kernel; why = the fusedOk reasons the level carries (taps, exact,
          rows, window, tall, mixed).  R is not written: it is ceil(hC / 64), which the CPU test checks against the plan and the GPU test
          against the report.
What the levels leave as (emit_rank, emit_f32) and the segment count follow from the case by the rules of expect() below, which restate
planLevels from the header's description of the options, not from its code's output.

Forks and their cases (hC is the tallest level's height in cells; W = 64 wherever height is the subject):
  R boundaries, real levels: real_<hC>_a7 / real_<hC>_a0 for hC 64 / 65 (R 1 / 2), 256 / 257 (R 4 / 5: both k_level_all for a real
    level), 512 / 513 (R 8 / 9: k_level_all / the k_level<9, LM_REAL> group, which also ends emit_rank), 576 / 577 (the last
    wave-per-plane height / the first smooth_jobs height: "tall"), with nApprox 7 and nApprox 0, H = 4 hC.
  R boundaries, approximated levels: approx_256 / approx_257 (R 4 / 5: k_level_all / group, H = 1090 / 1095, the smallest frames
    whose level 1 has those heights) and approx_512 / approx_513 (R 8 / 9: fused / "rows" and wave_smooth, H = 2180 / 2185).
  Exact ratio and tap count (nApprox >= nPerOct): exact_p1a1, exact_p2a3, exact_p4a7 (64 x 64: an approximated level exactly half
    its real level on both axes), taps_p1a1, taps_p2a3, taps_p4a7 (67 x 96: 24 -> 11 columns needs four taps, no axis exact), and the
    nearest plans that need neither: neither_p1a1 (66 x 72: 17 -> 8 rows, 18 -> 8 columns, three taps), neither_p2a1, neither_p4a3.
    An exact axis counts as "not down" in the mode, so an exact x with a down y reports LM_UD ("mixed") next to "exact": the
    source's claim that LM_DU / LM_UD cannot happen holds for levels that are not exact, and no such level can be fused anyway.
  The ha bound: window_r2_below / window_r2_at (nPerOct 4, nApprox 5, 763 / 767 x 64: level 3 is 119 / 120 rows from 191 / 192, the
    bound for R = 2 down is 192; "window" is the only reason in the plan) and window_r1_below / window_r1_at (nPerOct 4, nApprox 7,
    506 / 510 x 72: level 5 is 56 / 57 rows from 127 / 128, the bound for R = 1 down is 128).  For R = 1 the bound cannot be the only
    reason: hb <= 64 and ha >= 128 is a ratio of at least 2, a whole octave, where the columns shrink by 2 as well and need four taps
    or are exact; a scan of nPerOct 1..4 x nApprox <= 2 nPerOct x W 64..96 x H 100..800 finds "window" at R = 1 only beside "taps" or
    "exact".  Up-sampling levels never reach it (ha < hb <= 64 R).
  Modes: real_64_a7 has LM_DD (levels 1-4, 9-11) and LM_UU (levels 5-7) among k_level_all's jobs, approx_512 has both among the
    group jobs (LM_DD R 6..8, LM_UU R 5..6) beside LM_DD among k_level_all's.  (At W = 64 the small levels' widths are 4..7 cells and
    their scales follow the width: real_512_a7's last level is 128 rows from 224, past the bound, so that frame is a wave_smooth
    case.)  groups_forced: every level a group launch (ACF_HIP_FORCE_FALLBACK=level_groups, R 1..2 of every mode).
  Pad parity: pad_<pad_h>_<pad_w>_<H> for pad_h 4 / 12 (py 1 / 3), pad_w 0 / 4 / 12 (px 0 / 1 / 3), H 256 (levels 0 and 11 are 64 rows:
    py odd and hC % 64 == 0, the level kernels may not write the ranks) and H 260 (65 rows; no level a multiple of 64: they do, behind
    a descriptor shifted by one cell), each run with keep_pyramid 1 / 0 x rank_cells 1 / 0, every run on a fresh context and plan.  The profile has one name,
    k_pad_reflect, for the float and the 16-bit pad kernel; padLevels launches each on emit_f32 / emit_rank alone, so with keep_pyramid 0
    "only the 16-bit pad kernel" is asserted as emit_rank and not emit_f32, and by read_level refusing to answer.
  Batch shape: batch_pad (pad 4 / 4, H 260) and batch_group (approx_257's frame) at 1, 4, 5, 8 and 9 frames: the LEVEL_WAVES remainder
    and both sides of levelSegFrames (8 frames and fewer are cut into column segments, 9 are not).
  Options: opt_fused_levels_0 (smooth_jobs), opt_fused_levels_2 (wave_smooth with no reason), opt_segments_1 / opt_segments_3, smooth_0 (copy).
  The tap route: taps_fused, taps_wave_smooth, taps_smooth_jobs, taps_copy.

Largest frame: 2308 x 64 (real_577_*), 147,712 pixels: 577 cells is the first height past the level kernels, and H = 4 hC at shrink 4.

Hit fractions (windows of every level, the frames of the case's pool together; tests/test_level_forms.py asserts each strictly inside
(0.05, 0.9), tests/channel_params_case.py's window), measured with the oracle at the cascThr listed with each case (chosen per case
on the oracle among -0.5, -1, -1.5 and -2 as the value whose fraction lies nearest 0.3: -2 for every case with these 32 trees):
  real_64_a7 0.228, real_64_a0 0.261, real_65_a7 0.234, real_65_a0 0.267, real_256_a7 0.234, real_256_a0 0.262,
  real_257_a7 0.224, real_257_a0 0.259, real_512_a7 0.251, real_512_a0 0.281, real_513_a7 0.243, real_513_a0 0.275,
  real_576_a7 0.257, real_576_a0 0.288, real_577_a7 0.261, real_577_a0 0.293, approx_256 0.252, approx_257 0.245,
  approx_512 0.252, approx_513 0.266, exact_p1a1 0.313, taps_p1a1 0.261, exact_p2a3 0.308, taps_p2a3 0.268, exact_p4a7 0.303,
  taps_p4a7 0.252, neither_p1a1 0.282, neither_p2a1 0.308, neither_p4a3 0.303, window_r2_below 0.270, window_r2_at 0.282,
  window_r1_below 0.243, window_r1_at 0.252, groups_forced 0.194, pad_4_0_256 0.300, pad_4_0_260 0.302, pad_4_4_256 0.284,
  pad_4_4_260 0.285, pad_4_12_256 0.269, pad_4_12_260 0.266, pad_12_0_256 0.321, pad_12_0_260 0.324, pad_12_4_256 0.301,
  pad_12_4_260 0.304, pad_12_12_256 0.282, pad_12_12_260 0.282, batch_pad 0.253, batch_group 0.274, opt_fused_levels_0 0.228,
  opt_fused_levels_2 0.228, opt_segments_1 0.228, opt_segments_3 0.228, smooth_0 0.287, taps_fused 0.228, taps_wave_smooth 0.303,
  taps_smooth_jobs 0.228, taps_copy 0.287
"""
import functools
import os
import sys

import numpy as np

if __name__ == "__main__":
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from acf_amd import synth  # noqa: E402

HIT_LO, HIT_HI = 0.05, 0.9
TINY = dict(seed=3, name="TINY", nTrees=32)
FRAME_SEED = 41
CAP = 1 << 17
MODES = dict(r="real", d="dd", u="uu", x="du", y="ud")
TAKERS = {"A": "all", "G": "group", "-": None}
WHY_ORDER = ("taps", "exact", "rows", "window", "tall", "mixed")
BATCHES = (1, 4, 5, 8, 9)
PAD_SWEEP = [dict(keep_pyramid=k, rank_cells=r) for k in (1, 0) for r in (1, 0)]

# id -> (fork, model keywords, H, W, cascThr, run, path, approx_first, levels)
CASES = {
    "real_64_a7": ("real level of 64 rows (R 1), nApprox 7",
        {}, 256, 64, -2.0, {}, "fused", False,
        "64r:rA 60a:dA 52a:dA 48a:dA 44a:dA 40a:uA 36a:uA 32a:uA 28r:rA 24a:dA 20a:dA 16a:dA"),
    "real_64_a0": ("real level of 64 rows (R 1), nApprox 0",
        {'nApprox': 0}, 256, 64, -2.0, {}, "fused", False,
        "64r:rA 60r:rA 52r:rA 48r:rA 44r:rA 40r:rA 36r:rA 32r:rA 28r:rA 24r:rA 20r:rA 16r:rA"),
    "real_65_a7": ("real level of 65 rows (R 2), nApprox 7",
        {}, 260, 64, -2.0, {}, "fused", False,
        "65r:rA 61a:dA 53a:dA 49a:dA 45a:dA 41a:uA 37a:uA 32a:uA 28r:rA 24a:dA 20a:dA 16a:dA"),
    "real_65_a0": ("real level of 65 rows (R 2), nApprox 0",
        {'nApprox': 0}, 260, 64, -2.0, {}, "fused", False,
        "65r:rA 61r:rA 53r:rA 49r:rA 45r:rA 41r:rA 37r:rA 32r:rA 28r:rA 24r:rA 20r:rA 16r:rA"),
    "real_256_a7": ("real level of 256 rows (R 4), nApprox 7",
        {}, 1024, 64, -2.0, {}, "fused", False,
        "256r:rA 240a:dA 208a:dA 192a:dA 176a:dA 160a:uA 144a:uA 128a:uA 112r:rA 96a:dA 80a:dA 64a:dA"),
    "real_256_a0": ("real level of 256 rows (R 4), nApprox 0",
        {'nApprox': 0}, 1024, 64, -2.0, {}, "fused", False,
        "256r:rA 240r:rA 208r:rA 192r:rA 176r:rA 160r:rA 144r:rA 128r:rA 112r:rA 96r:rA 80r:rA 64r:rA"),
    "real_257_a7": ("real level of 257 rows (R 5), nApprox 7",
        {}, 1028, 64, -2.0, {}, "fused", False,
        "257r:rA 241a:dA 209a:dA 193a:dA 177a:dA 161a:uA 144a:uA 129a:uA 113r:rA 96a:dA 80a:dA 64a:dA"),
    "real_257_a0": ("real level of 257 rows (R 5), nApprox 0",
        {'nApprox': 0}, 1028, 64, -2.0, {}, "fused", False,
        "257r:rA 241r:rA 209r:rA 193r:rA 177r:rA 161r:rA 144r:rA 129r:rA 113r:rA 96r:rA 80r:rA 64r:rA"),
    "real_512_a7": ("real level of 512 rows (R 8), nApprox 7",
        {}, 2048, 64, -2.0, {}, "wave_smooth", True,
        "512r:rA 480a:rA 416a:rA 384a:rA 352a:rA 320a:rA 288a:rA 256a:rA 224r:rA 192a:rA 160a:rA 128a:rA!window"),
    "real_512_a0": ("real level of 512 rows (R 8), nApprox 0",
        {'nApprox': 0}, 2048, 64, -2.0, {}, "fused", False,
        "512r:rA 480r:rA 416r:rA 384r:rA 352r:rA 320r:rA 288r:rA 256r:rA 224r:rA 192r:rA 160r:rA 128r:rA"),
    "real_513_a7": ("real level of 513 rows (R 9: the k_level<9, LM_REAL> group), nApprox 7",
        {}, 2052, 64, -2.0, {}, "wave_smooth", True,
        "513r:rG 480a:rA 416a:rA 386a:rA 353a:rA 320a:rA 289a:rA 257a:rA 224r:rA 193a:rA 160a:rA 127a:rA!window"),
    "real_513_a0": ("real level of 513 rows (R 9: the k_level<9, LM_REAL> group), nApprox 0",
        {'nApprox': 0}, 2052, 64, -2.0, {}, "fused", False,
        "513r:rG 480r:rA 416r:rA 386r:rA 353r:rA 320r:rA 289r:rA 257r:rA 224r:rA 193r:rA 160r:rA 127r:rA"),
    "real_576_a7": ("real level of 576 rows (R 9, the last wave-per-plane height), nApprox 7",
        {}, 2304, 64, -2.0, {}, "wave_smooth", True,
        "576r:rG 540a:rG!rows 468a:rA 432a:rA 396a:rA 360a:rA 324a:rA 288a:rA 252r:rA 216a:rA 180a:rA 144a:rA"),
    "real_576_a0": ("real level of 576 rows (R 9, the last wave-per-plane height), nApprox 0",
        {'nApprox': 0}, 2304, 64, -2.0, {}, "fused", False,
        "576r:rG 540r:rG 468r:rA 432r:rA 396r:rA 360r:rA 324r:rA 288r:rA 252r:rA 216r:rA 180r:rA 144r:rA"),
    "real_577_a7": ("real level of 577 rows (the first smooth_jobs height), nApprox 7",
        {}, 2308, 64, -2.0, {}, "smooth_jobs", True,
        "577r:r-!tall 542a:d-!rows 469a:d- 432a:d- 396a:d- 361a:u- 324a:u- 288a:u- 253r:r- 216a:d- 181a:d- 145a:d-"),
    "real_577_a0": ("real level of 577 rows (the first smooth_jobs height), nApprox 0",
        {'nApprox': 0}, 2308, 64, -2.0, {}, "smooth_jobs", False,
        "577r:r-!tall 542r:r- 469r:r- 432r:r- 396r:r- 361r:r- 324r:r- 288r:r- 253r:r- 216r:r- 181r:r- 145r:r-"),
    "approx_256": ("approximated level of 256 rows (R 4): k_level_all",
        {}, 1090, 64, -2.0, {}, "fused", False,
        "272r:rA 256a:dA 221a:dA 204a:dA 187a:dA 170a:uA 153a:uA 136a:uA 119r:rA 102a:dA 85a:dA 68a:dA"),
    "approx_257": ("approximated level of 257 rows (R 5): a group launch",
        {}, 1095, 64, -2.0, {}, "fused", False,
        "274r:rA 257a:dG 222a:dA 205a:dA 188a:dA 171a:uA 154a:uA 137a:uA 120r:rA 103a:dA 86a:dA 68a:dA"),
    "approx_512": ("approximated level of 512 rows (R 8): fused",
        {}, 2180, 64, -2.0, {}, "fused", False,
        "545r:rG 512a:dG 443a:dG 407a:dG 374a:dG 341a:uG 305a:uG 272a:uG 240r:rA 204a:dA 171a:dA 138a:dA"),
    "approx_513": ("approximated level of 513 rows (R 9): rows, wave_smooth",
        {}, 2185, 64, -2.0, {}, "wave_smooth", True,
        "548r:rG 513a:rG!rows 444a:rA 409a:rA 375a:rA 340a:rA 309a:rA 274a:rA 239r:rA 205a:rA 170a:rA 135a:rA"),
    "exact_p1a1": ("an approximated level exactly half its real level",
        {'nPerOct': 1, 'nApprox': 1}, 64, 64, -2.0, {}, "wave_smooth", True,
        "16r:rA 8a:rA!exact 4r:rA"),
    "taps_p1a1": ("an approximated level that needs four taps",
        {'nPerOct': 1, 'nApprox': 1}, 67, 96, -2.0, {}, "wave_smooth", True,
        "17r:rA 8a:rA!taps 4r:rA"),
    "exact_p2a3": ("an approximated level exactly half its real level",
        {'nPerOct': 2, 'nApprox': 3}, 64, 64, -2.0, {}, "wave_smooth", True,
        "16r:rA 11a:rA 8a:rA!exact 6a:rA 4r:rA"),
    "taps_p2a3": ("an approximated level that needs four taps",
        {'nPerOct': 2, 'nApprox': 3}, 67, 96, -2.0, {}, "wave_smooth", True,
        "17r:rA 12a:rA 8a:rA!taps 6a:rA 4r:rA"),
    "exact_p4a7": ("an approximated level exactly half its real level",
        {'nPerOct': 4, 'nApprox': 7}, 64, 64, -2.0, {}, "wave_smooth", True,
        "16r:rA 13a:rA 11a:rA 10a:rA 8a:rA!exact 7a:rA 6a:rA 5a:rA 4r:rA"),
    "taps_p4a7": ("an approximated level that needs four taps",
        {'nPerOct': 4, 'nApprox': 7}, 67, 96, -2.0, {}, "wave_smooth", True,
        "17r:rA 14a:rA 12a:rA 10a:rA 8a:rA!taps 7a:rA 6a:rA 5a:rA 4r:rA"),
    "neither_p1a1": ("nApprox >= nPerOct with neither an exact ratio nor four taps",
        {'nPerOct': 1, 'nApprox': 1}, 66, 72, -2.0, {}, "fused", False,
        "17r:rA 8a:dA 4r:rA"),
    "neither_p2a1": ("nApprox = nPerOct - 1: neither",
        {'nPerOct': 2, 'nApprox': 1}, 64, 64, -2.0, {}, "fused", False,
        "16r:rA 11a:dA 8r:rA 6a:dA 4r:rA"),
    "neither_p4a3": ("nApprox = nPerOct - 1: neither",
        {'nPerOct': 4, 'nApprox': 3}, 64, 64, -2.0, {}, "fused", False,
        "16r:rA 13a:dA 11a:dA 10a:uA 8r:rA 7a:dA 6a:dA 5a:uA 4r:rA"),
    "window_r2_below": ("ha = 191 under the bound 192 of R 2 down",
        {'nPerOct': 4, 'nApprox': 5}, 763, 64, -2.0, {}, "fused", False,
        "191r:rA 155a:dA 131a:dA 119a:dA 95a:uA 83a:uA 72r:rA 60a:dA 48a:dA"),
    "window_r2_at": ("ha = 192 at the bound 192 of R 2 down",
        {'nPerOct': 4, 'nApprox': 5}, 767, 64, -2.0, {}, "wave_smooth", True,
        "192r:rA 156a:rA 132a:rA 120a:rA!window 96a:rA 84a:rA 72r:rA 60a:rA 48a:rA"),
    "window_r1_below": ("ha = 127 under the bound 128 of R 1 down",
        {'nPerOct': 4, 'nApprox': 7}, 506, 72, -2.0, {}, "wave_smooth", True,
        "127r:rA 105a:rA 91a:rA 77a:rA 63a:rA!exact,mixed 56a:rA!taps 42a:rA!taps,exact,mixed 35a:rA!taps"),
    "window_r1_at": ("ha = 128 at the bound 128 of R 1 down",
        {'nPerOct': 4, 'nApprox': 7}, 510, 72, -2.0, {}, "wave_smooth", True,
        "128r:rA 106a:rA 92a:rA 78a:rA 64a:rA!exact,window 57a:rA!taps,window 43a:rA!taps,exact,window,mixed 35a:rA!taps,window"),
    "groups_forced": ("every level a group launch, LM_DD and LM_UU at R 1..2",
        {}, 320, 64, -2.0, {'env': 'level_groups'}, "fused", False,
        "80r:rG 75a:dG 65a:dG 60a:dG 55a:dG 50a:uG 45a:uG 40a:uG 35r:rG 30a:dG 25a:dG 20a:dG"),
    "pad_4_0_256": ("py 1, px 0, levels of 64 rows: no rank stores",
        {'pad_h': 4, 'pad_w': 0}, 256, 64, -2.0, {}, "fused", False,
        "64r:rA 60a:dA 52a:dA 48a:dA 44a:dA 40a:uA 36a:uA 32a:uA 28r:rA 24a:dA 20a:dA 16a:dA"),
    "pad_4_0_260": ("py 1, px 0, no level a multiple of 64 rows: rank stores shifted by one cell",
        {'pad_h': 4, 'pad_w': 0}, 260, 64, -2.0, {}, "fused", False,
        "65r:rA 61a:dA 53a:dA 49a:dA 45a:dA 41a:uA 37a:uA 32a:uA 28r:rA 24a:dA 20a:dA 16a:dA"),
    "pad_4_4_256": ("py 1, px 1, levels of 64 rows: no rank stores",
        {'pad_h': 4, 'pad_w': 4}, 256, 64, -2.0, {}, "fused", False,
        "64r:rA 60a:dA 52a:dA 48a:dA 44a:dA 40a:uA 36a:uA 32a:uA 28r:rA 24a:dA 20a:dA 16a:dA"),
    "pad_4_4_260": ("py 1, px 1, no level a multiple of 64 rows: rank stores shifted by one cell",
        {'pad_h': 4, 'pad_w': 4}, 260, 64, -2.0, {}, "fused", False,
        "65r:rA 61a:dA 53a:dA 49a:dA 45a:dA 41a:uA 37a:uA 32a:uA 28r:rA 24a:dA 20a:dA 16a:dA"),
    "pad_4_12_256": ("py 1, px 3, levels of 64 rows: no rank stores",
        {'pad_h': 4, 'pad_w': 12}, 256, 64, -2.0, {}, "fused", False,
        "64r:rA 60a:dA 52a:dA 48a:dA 44a:dA 40a:uA 36a:uA 32a:uA 28r:rA 24a:dA 20a:dA 16a:dA"),
    "pad_4_12_260": ("py 1, px 3, no level a multiple of 64 rows: rank stores shifted by one cell",
        {'pad_h': 4, 'pad_w': 12}, 260, 64, -2.0, {}, "fused", False,
        "65r:rA 61a:dA 53a:dA 49a:dA 45a:dA 41a:uA 37a:uA 32a:uA 28r:rA 24a:dA 20a:dA 16a:dA"),
    "pad_12_0_256": ("py 3, px 0, levels of 64 rows: no rank stores",
        {'pad_h': 12, 'pad_w': 0}, 256, 64, -2.0, {}, "fused", False,
        "64r:rA 60a:dA 52a:dA 48a:dA 44a:dA 40a:uA 36a:uA 32a:uA 28r:rA 24a:dA 20a:dA 16a:dA"),
    "pad_12_0_260": ("py 3, px 0, no level a multiple of 64 rows: rank stores shifted by one cell",
        {'pad_h': 12, 'pad_w': 0}, 260, 64, -2.0, {}, "fused", False,
        "65r:rA 61a:dA 53a:dA 49a:dA 45a:dA 41a:uA 37a:uA 32a:uA 28r:rA 24a:dA 20a:dA 16a:dA"),
    "pad_12_4_256": ("py 3, px 1, levels of 64 rows: no rank stores",
        {'pad_h': 12, 'pad_w': 4}, 256, 64, -2.0, {}, "fused", False,
        "64r:rA 60a:dA 52a:dA 48a:dA 44a:dA 40a:uA 36a:uA 32a:uA 28r:rA 24a:dA 20a:dA 16a:dA"),
    "pad_12_4_260": ("py 3, px 1, no level a multiple of 64 rows: rank stores shifted by one cell",
        {'pad_h': 12, 'pad_w': 4}, 260, 64, -2.0, {}, "fused", False,
        "65r:rA 61a:dA 53a:dA 49a:dA 45a:dA 41a:uA 37a:uA 32a:uA 28r:rA 24a:dA 20a:dA 16a:dA"),
    "pad_12_12_256": ("py 3, px 3, levels of 64 rows: no rank stores",
        {'pad_h': 12, 'pad_w': 12}, 256, 64, -2.0, {}, "fused", False,
        "64r:rA 60a:dA 52a:dA 48a:dA 44a:dA 40a:uA 36a:uA 32a:uA 28r:rA 24a:dA 20a:dA 16a:dA"),
    "pad_12_12_260": ("py 3, px 3, no level a multiple of 64 rows: rank stores shifted by one cell",
        {'pad_h': 12, 'pad_w': 12}, 260, 64, -2.0, {}, "fused", False,
        "65r:rA 61a:dA 53a:dA 49a:dA 45a:dA 41a:uA 37a:uA 32a:uA 28r:rA 24a:dA 20a:dA 16a:dA"),
    "batch_pad": ("odd py, batches of 1, 4, 5, 8, 9",
        {'pad_h': 4, 'pad_w': 4}, 260, 64, -2.0, {'batches': (1, 4, 5, 8, 9)}, "fused", False,
        "65r:rA 61a:dA 53a:dA 49a:dA 45a:dA 41a:uA 37a:uA 32a:uA 28r:rA 24a:dA 20a:dA 16a:dA"),
    "batch_group": ("a group launch, batches of 1, 4, 5, 8, 9",
        {}, 1095, 64, -2.0, {'batches': (1, 4, 5, 8, 9)}, "fused", False,
        "274r:rA 257a:dG 222a:dA 205a:dA 188a:dA 171a:uA 154a:uA 137a:uA 120r:rA 103a:dA 86a:dA 68a:dA"),
    "opt_fused_levels_0": ("option fused_levels 0: smooth_jobs",
        {}, 256, 64, -2.0, {'fused_levels': 0}, "smooth_jobs", True,
        "64r:r- 60a:d- 52a:d- 48a:d- 44a:d- 40a:u- 36a:u- 32a:u- 28r:r- 24a:d- 20a:d- 16a:d-"),
    "opt_fused_levels_2": ("option fused_levels 2: wave_smooth with no reason",
        {}, 256, 64, -2.0, {'fused_levels': 2}, "wave_smooth", True,
        "64r:rA 60a:rA 52a:rA 48a:rA 44a:rA 40a:rA 36a:rA 32a:rA 28r:rA 24a:rA 20a:rA 16a:rA"),
    "opt_segments_1": ("option level_segments 1: one chain",
        {}, 256, 64, -2.0, {'level_segments': 1}, "fused", False,
        "64r:rA 60a:dA 52a:dA 48a:dA 44a:dA 40a:uA 36a:uA 32a:uA 28r:rA 24a:dA 20a:dA 16a:dA"),
    "opt_segments_3": ("option level_segments 3",
        {}, 256, 64, -2.0, {'level_segments': 3}, "fused", False,
        "64r:rA 60a:dA 52a:dA 48a:dA 44a:dA 40a:uA 36a:uA 32a:uA 28r:rA 24a:dA 20a:dA 16a:dA"),
    "smooth_0": ("smooth 0: plane copies",
        {'smooth': 0}, 256, 64, -2.0, {}, "copy", True,
        "64r:r- 60a:d- 52a:d- 48a:d- 44a:d- 40a:u- 36a:u- 32a:u- 28r:r- 24a:d- 20a:d- 16a:d-"),
    "taps_fused": ("taps on the fused path: rawOut",
        {}, 256, 64, -2.0, {'taps': 1}, "fused", False,
        "64r:rA 60a:dA 52a:dA 48a:dA 44a:dA 40a:uA 36a:uA 32a:uA 28r:rA 24a:dA 20a:dA 16a:dA"),
    "taps_wave_smooth": ("taps on wave_smooth",
        {'nPerOct': 4, 'nApprox': 7}, 64, 64, -2.0, {'taps': 1}, "wave_smooth", True,
        "16r:rA 13a:rA 11a:rA 10a:rA 8a:rA!exact 7a:rA 6a:rA 5a:rA 4r:rA"),
    "taps_smooth_jobs": ("taps on smooth_jobs",
        {}, 256, 64, -2.0, {'taps': 1, 'fused_levels': 0}, "smooth_jobs", True,
        "64r:r- 60a:d- 52a:d- 48a:d- 44a:d- 40a:u- 36a:u- 32a:u- 28r:r- 24a:d- 20a:d- 16a:d-"),
    "taps_copy": ("taps on copy",
        {'smooth': 0}, 256, 64, -2.0, {'taps': 1}, "copy", True,
        "64r:r- 60a:d- 52a:d- 48a:d- 44a:d- 40a:u- 36a:u- 32a:u- 28r:r- 24a:d- 20a:d- 16a:d-"),
}


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def parse_levels(case):
    """-> [dict(hC, real, R, mode, by, why)] of the case's level tokens"""
    out = []
    for tok in CASES[case][8].split():
        geo, form = tok.split(":")
        form, _, why = form.partition("!")
        hC = int(geo[:-1])
        out.append(dict(hC=hC, real=geo[-1] == "r", R=(hC + 63) // 64, mode=MODES[form[0]], by=TAKERS[form[1]],
                        why=tuple(w for w in WHY_ORDER if w in why.split(","))))
    return out


def expect(case, run, batch):
    """What level_forms() must report for one run (run: the case's options, for the pad sweep with keep_pyramid / rank_cells of the
    run) of `batch` frames on a plan for max(batches) frames.  The rules, from include/acf_hip.h's options: the level kernels write
    the rank cells when the path is fused, every level is k_level_all's, no level is a multiple of 64 rows under an odd pad, and
    rank cells, the tile cascade (both default on) are on and taps off; floats unless they write ranks and keep_pyramid is 0; column
    segments only on the fused path without taps for batches of at most min(max_batch, 8) frames: level_segments if > 1, one if 1,
    else enough for 4096 waves, at most 8."""
    _, kw, H, W, _, _, path, approx_first, _ = CASES[case]
    lv = parse_levels(case)
    py = kw.get("pad_h", 0) // 4
    taps = run.get("taps", 0)
    wave = path in ("fused", "wave_smooth")
    n_all = sum(l["by"] == "all" for l in lv)
    emit_rank = (path == "fused" and n_all == len(lv) and not any((py & 1) and l["hC"] % 64 == 0 for l in lv) and
                 bool(run.get("rank_cells", 1)) and not taps)
    emit_f32 = not (emit_rank and not run.get("keep_pyramid", 1))
    seg = 0
    if wave and n_all:
        seg = 1
        opt = run.get("level_segments", 0)
        if path == "fused" and not taps and batch <= min(max(batches(case)), 8) and opt != 1:
            waves = n_all * synth.n_channels(model(case)) * batch
            seg = max(1, min(opt if opt > 1 else (4096 + waves - 1) // waves, 8))
    return dict(path=path, emit_rank=emit_rank, emit_f32=emit_f32, segments=seg, approx_first=approx_first,
                levels=[dict(R=l["R"], mode=l["mode"], by=l["by"], why=l["why"]) for l in lv])


def batches(case):
    return tuple(CASES[case][5].get("batches", (2,)))


def runs(case):
    """the runs of a case: the pad cases sweep keep_pyramid x rank_cells, every other case runs its options once"""
    run = {k: v for k, v in CASES[case][5].items() if k not in ("batches", "env")}
    return [dict(run, **s) for s in PAD_SWEEP] if case.startswith("pad_") else [run]


def launches(case):
    """-> [(run, batch, first)]: every run x every batch size.  Each launch gets a context and a plan of its own and the frames
    first .. first + batch - 1 of the case's pool, first = the launch's number, so that no launch finds in any slot, float or rank, what
    an earlier one would have left there: a kernel that drops stores cannot pass on an earlier launch's cells."""
    out = []
    for run in runs(case):
        for n in batches(case):
            out.append((run, n, len(out)))
    return out


@functools.lru_cache(maxsize=None)
def model(case):
    return synth.make_model(**dict(TINY, cascThr=CASES[case][4], **CASES[case][1]))


@functools.lru_cache(maxsize=None)
def frames(H, W, n):
    a = np.stack([synth.make_frame(FRAME_SEED + f, H, W, "luv") for f in range(n)])
    a.setflags(write=False)
    return a


def case_frames(case):
    """the case's pool: enough frames for its last launch (launches)"""
    return frames(CASES[case][2], CASES[case][3], max(first + n for _, n, first in launches(case)))


@functools.lru_cache(maxsize=None)
def expected(case):
    """-> (plan, [per frame: dict(pyr, det, hits)]) from the oracle, for the frames of the case's pool.  Read-only, shared."""
    from oracle import binding as ob
    plan = ob.Plan(model(case), CASES[case][2], CASES[case][3], 3)
    out = []
    for frame in case_frames(case):
        pyr, _, _ = ob.chns_pyramid(plan, frame)
        pyr.setflags(write=False)
        det, hits = ob.detect(plan, pyr, cap=CAP)
        out.append(dict(pyr=pyr, det=det, hits=hits))
    return plan, out


def expected_chns(case, f):
    """raw channels per level of frame f (the tap route; not kept)"""
    from oracle import binding as ob
    plan, _ = expected(case)
    return ob.chns_pyramid(plan, case_frames(case)[f], want_taps=True, want_chns=True)[2]


def n_windows(case):
    plan, _ = expected(case)
    return sum(max(plan.levels[i].nWinR, 0) * max(plan.levels[i].nWinC, 0) for i in range(plan.nScales))


def hit_fraction(case):
    _, exp = expected(case)
    return sum(len(e["hits"]) for e in exp) / float(len(exp) * n_windows(case))


def axis_taps(na, nb):
    """(kind, taps) of resampling na -> nb samples, restated from imResampleMex.cpp's resampleCoef in float32: kind "exact" (na = 2, 3
    or 4 nb), "down" or "up"; taps = the most source samples an output sample of a down-sampling axis combines (weights above 1e-3 s)."""
    f32 = np.float32
    kind = "exact" if na in (2 * nb, 3 * nb, 4 * nb) else "down" if na > nb else "up"
    taps = 0
    if na > nb:
        s = f32(nb) / f32(na)
        s_inv = f32(1) / s
        wt0 = f32(1e-3) * s
        for yb in range(nb):
            ya0f = f32(yb) * s_inv
            ya1f = f32(ya0f + s_inv)
            ya0, ya1 = int(np.ceil(ya0f)), int(ya1f)
            n1 = 0
            for ya in range(max(ya0 - 1, 0), ya1 + 1):
                wt = f32(f32(ya0) - ya0f) * s if ya == ya0 - 1 else f32(ya1f - f32(ya1)) * s if ya == ya1 else s
                n1 += bool(wt > wt0)
            taps = max(taps, n1)
    return kind, taps


def level_reasons(plan_levels, i):
    """The fusedOk reasons of level i from the plan's geometry alone, as the issue states them (restated here, not read from the
    library): more than three taps on a down axis; an exact 1/k ratio; an approximated level of more than 8 rows per lane; ha >= 64 *
    ((3R + 1) / 2 for a down y axis, R else); taller than 576 cells; one axis down and the other not."""
    l = plan_levels[i]
    R = (l.hC + 63) // 64
    why = ["tall"] if l.hC > 576 else []
    if not l.isReal:
        lr = plan_levels[l.realIndex]
        (ky, ty), (kx, tx) = axis_taps(lr.hC, l.hC), axis_taps(lr.wC, l.wC)
        why += ["taps"] if (ky == "down" and ty > 3) or (kx == "down" and tx > 3) else []
        why += ["exact"] if "exact" in (ky, kx) else []
        why += ["rows"] if R > 8 else []
        why += ["window"] if lr.hC >= 64 * ((3 * R + 1) // 2 if ky == "down" else R) else []
        why += ["mixed"] if (ky == "down") != (kx == "down") else []
    return tuple(w for w in WHY_ORDER if w in why)


# ------------------------------------------------------------------ the GPU side (tests/test_gpu_level_forms.py; a child process for "env")

def channel_thresholds(m, nChns, chn):
    mH, mW = m["modelDsPad_h"] // m["shrink"], m["modelDsPad_w"] // m["shrink"]
    fids = m["fids"][:, :3].ravel()
    thrs = m["thrs"][:, :3].ravel()
    return np.unique(thrs[fids // (mH * mW) == chn].astype(np.float32))


def ranks_of(m, nChns, level):
    """ranks of a float level [nChns][wP][hP], as tests/test_rank_cells.py computes them"""
    out = np.zeros(level.shape, np.uint16)
    for z in range(nChns):
        t = channel_thresholds(m, nChns, z)
        out[z] = np.searchsorted(t, level[z].ravel(), side="right").reshape(level[z].shape)
    return out


def compare(det, case, run, n, first, forms):
    """slots 0..n-1 of the last run, which hold the pool's frames first..first+n-1, against the oracle: floats where the call kept them,
    rank cells where the plan has them (padded border included: whole levels), hits, scores, boxes"""
    from acf_amd import capi
    from acf_amd.detector import HipError
    plan, exp = expected(case)
    m = model(case)
    for f in range(n):
        e = exp[first + f]
        where = (case, sorted(run.items()), "batch", n, "slot", f, "frame", first + f)
        for i in range(plan.nScales):
            want = plan.level_view(e["pyr"], i)
            if forms["emit_f32"]:
                assert np.array_equal(bits(det.read_level(f, i)), bits(want)), where + ("pyramid level", i)
            if run.get("rank_cells", 1):
                assert np.array_equal(det.read_rank_level(f, i), ranks_of(m, plan.nChns, want)), where + ("rank level", i)
        if not forms["emit_f32"]:
            try:
                det.read_level(f, 0)
                raise AssertionError(where + ("read_level answered without a float pyramid",))
            except HipError:
                pass
        if run.get("taps", 0):
            chns = expected_chns(case, first + f)
            for i in range(plan.nScales):
                l = plan.levels[i]
                got = det.read_tap(f, capi.TAP_CHNS, i, (plan.nChns, l.wC, l.hC))
                assert np.array_equal(bits(got), bits(chns[i])), where + ("raw channels level", i)
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


def check_forms(case, run, n, forms, prof):
    """the form the case is named for, from level_forms(); the profile's kernel names where they tell forms apart (prof() calls of
    pyramid_run.hip.h launchLevels / padLevels, acf_hip.hip launchSmooth)"""
    want = expect(case, run, n)
    where = (case, sorted(run.items()), "batch", n)
    for key in ("path", "approx_first", "emit_rank", "emit_f32", "segments"):
        assert forms[key] == want[key], where + (key, forms[key], want[key])
    assert len(forms["levels"]) == len(want["levels"]), where
    for i, (g, w) in enumerate(zip(forms["levels"], want["levels"])):
        assert g == w, where + ("level", i, g, w)
    names = set(prof)
    kw = CASES[case][1]
    assert ("k_level(fused)" in names) == (want["path"] == "fused"), where + (sorted(names),)
    assert ("k_level(smooth)" in names) == (want["path"] == "wave_smooth"), where + (sorted(names),)
    assert ("k_resample(approx)" in names) == want["approx_first"], where + (sorted(names),)
    assert ("k_pad_reflect" in names) == bool(kw.get("pad_h", 0) or kw.get("pad_w", 0)), where + (sorted(names),)
    if want["path"] in ("smooth_jobs", "copy"):
        assert not any(k.startswith("k_level") for k in names), where + (sorted(names),)
    # without the level kernels' rank cells the cascade converts the float pyramid first
    assert ("k_rank" in names) == bool(run.get("rank_cells", 1) and not want["emit_rank"]), where + (sorted(names),)


def run_case(case):
    """every launch of the case (launches) on a context of its own: compare with the oracle, then assert the forms"""
    import torch
    from acf_amd.detector import HipDetector
    _, kw, H, W, _, _, _, _, _ = CASES[case]
    _, exp = expected(case)
    nmax = max(batches(case))
    max_hits = max(1 << 14, 2 * max(len(e["hits"]) for e in exp))
    pool = torch.from_numpy(np.array(case_frames(case))).cuda()
    for run, n, first in launches(case):
        det = HipDetector(taps=bool(run.get("taps", 0)))
        try:
            for k, v in run.items():
                if k != "taps":
                    det.set_option(k, v)
            det.set_option("profile", 1)
            det.set_model(model(case))
            det.plan(H, W, 3, max_batch=nmax, max_hits=max_hits)
            det.run(pool[first:first + n].contiguous(), n)
            prof = det.profile()
            forms = det.level_forms()
            print(case, sorted(run.items()), "batch", n, "first frame", first, {k: v for k, v in forms.items() if k != "levels"}, "kernels:", " ".join(sorted(prof)))
            # the comparison first, then the form; a wrong form is reported even where the comparison has failed already
            errs = []
            for check in (lambda: compare(det, case, run, n, first, forms), lambda: check_forms(case, run, n, forms, prof)):
                try:
                    check()
                except AssertionError as e:
                    errs.append(e)
            assert not errs, errs
        finally:
            det.close()


def forms_before_the_first_call(case):
    """level_forms() on a plan that has not run: call-wide words zero (path 0, no segments), the levels those of the plan's fused list"""
    from acf_amd.detector import HipDetector
    _, kw, H, W, _, _, path, _, _ = CASES[case]
    assert path == "fused"   # (the case's tokens are the fused list's then)
    det = HipDetector(model(case), H, W, 3, max_batch=2, max_hits=1 << 14)
    try:
        forms = det.level_forms()
    finally:
        det.close()
    want = expect(case, {}, 2)
    assert forms == dict(path="fused", emit_rank=False, emit_f32=False, segments=0, approx_first=False, levels=want["levels"]), forms


if __name__ == "__main__":
    run_case(sys.argv[1])
    print("ok", sys.argv[1])
