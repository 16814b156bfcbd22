"""The planned pipeline (acf_hip_plan + acf_hip_run, what bench.py times) away from the default channel parameters, against the oracle:
every pyramid level, the hits and the mapped boxes, bit for bit, for every case of tests/channel_params_case.py under the option sets
that select the pipeline's kernel forms.  With option profile on, the kernel names also tell which form ran where they differ
(acf_hip.hip launchTri, pyramid_run.hip.h smoothImage / launchLevels), so a case cannot pass on a form other than the one it is there for.

tests/test_channel_params.py holds the CPU side: the cases' hit fractions and the host plan; tests/test_oracle_vs_ref.py pins the
oracle to the reference's compiled kernels at these parameters."""
import numpy as np
import pytest

from acf_amd import capi

import channel_params_case as cp

pytestmark = pytest.mark.gpu

# name -> (options, taps)
OPTION_SETS = {
    "production": (dict(), False),                                               # the defaults, taps off
    "grad_tri_on_chain": (dict(fused_grad=2, fused_tri=2), False),               # k_smooth_grad / k_smooth_grad_tri: not reached at these sizes otherwise
    "separate_levels_staged": (dict(fused_levels=0, cascade_tiles=0), False),
    "no_rank_cells": (dict(rank_cells=0), False),
    "segments": (dict(smooth_segments=3, smooth_warm=16, level_segments=4, level_warm=16, count_repairs=1), False),
    "taps": (dict(), True),
}
SETS_12 = ("production", "grad_tri_on_chain")


def check_forms(case, optset, H, W, prof):
    """The kernel names option profile reports against the form the case is there for (names: the prof() calls of acf_hip.hip
    launchTri / launchSmooth and pyramid_run.hip.h)."""
    kw = cp.CASES[case][0]
    names = set(prof)
    tri = {n for n in names if n.startswith("k_tri") or n == "k_smooth_grad_tri"}
    grad = kw.get("gradMagEnabled", 1) or kw.get("gradHistEnabled", 1)
    normRad = kw.get("normRad", 5)
    if grad and normRad not in (0, 5):
        # the generic-radius normalisation: running sums (k_tri_x), the y pass on its own (k_tri_y), the cells from k_chns
        assert {"k_tri_x", "k_tri_y", "k_chns"} <= names and "k_triy_chns" not in names and "k_smooth_grad_tri" not in names, sorted(names)
    if normRad == 0:
        assert not tri, sorted(names)
    if not grad:
        assert not tri and "k_grad_mag" not in names and not any(n.startswith("k_smooth_grad") for n in names), sorted(names)
    if kw.get("nOrients") == 12 and normRad == 5 and (H, W) in ((128, 192), (240, 320)) and optset in SETS_12:
        assert "k_triy_chns" in names, sorted(names)     # (the <12> instantiation: nOrients 7 .. 12)
    if kw.get("smooth", 1) == 0:
        assert not any(n.startswith("k_level") for n in names) and "k_smooth_tri1(levels)" not in names, sorted(names)
    if kw.get("colorSmooth", 1) == 0:
        assert "k_smooth_vec" not in names and "k_smooth_tri1(image)" not in names and not any(n.startswith("k_smooth_grad") for n in names), sorted(names)


def compare(det, case, H, W, exp, optset):
    plan, frames_exp = exp
    ldcf = cp.is_ldcf(case)
    for f, e in enumerate(frames_exp):
        where = (case, optset, H, W, "frame", f)
        for i in range(plan.nScales):
            assert np.array_equal(cp.bits(det.read_level(f, i)), cp.bits(plan.level_view(e["pyr"], i))), where + ("pyramid level", i)
        if ldcf:
            lvL, pyrL, k = e["ldcf"]
            for i in range(plan.nScales):
                l = lvL[i]
                n = plan.nChns * k * l.hP * l.wP
                want = pyrL[l.offset:l.offset + n].reshape(plan.nChns * k, l.wP, l.hP)
                got = det.read_tap(f, capi.TAP_LDCF, i, (plan.nChns * k, l.wP, l.hP))
                assert np.array_equal(cp.bits(got), cp.bits(want)), where + ("LDCF level", i)
        got, got_hits = det.detections(f)
        want, want_hits = e["det"], e["hits"]
        assert len(want_hits) > 0, where
        assert len(got_hits) == len(want_hits) and len(got) == len(want), where + (len(got_hits), len(want_hits))
        for key in ("scale", "c", "r"):
            assert np.array_equal(got_hits[key], want_hits[key]), where + ("hits", key)
        assert np.array_equal(cp.bits(got_hits["score"]), cp.bits(want_hits["score"])), where + ("hit scores",)
        for key in ("x", "y", "w", "h", "scale"):
            assert np.array_equal(got[key], want[key]), where + ("detections", key)
        assert np.array_equal(cp.bits(got["score"]), cp.bits(want["score"])), where + ("detection scores",)


def compare_taps(det, case, H, W, plan):
    """The stage outputs per real scale and the raw channels per level, as test_pipeline_bit_exact reads them: a failure names its stage."""
    kw = cp.CASES[case][0]
    grad = kw.get("gradMagEnabled", 1) or kw.get("gradHistEnabled", 1)
    norm = grad and kw.get("normRad", 5) != 0
    for f in range(cp.N_FRAMES):
        taps, chns = cp.expected_taps(case, H, W, f)
        for k in range(len(plan.real)):
            t = taps[k]
            stages = [("smoothed", capi.TAP_SMOOTHED)]
            stages += [("M", capi.TAP_M), ("O", capi.TAP_O)] if grad else []
            stages += [("S", capi.TAP_S), ("Mnorm", capi.TAP_MNORM)] if norm else []
            for name, tap in stages:
                got = det.read_tap(f, tap, k, t[name].shape)
                assert np.array_equal(cp.bits(got), cp.bits(t[name])), (case, H, W, "frame", f, "real scale", k, name, float(np.abs(got - t[name]).max()))
        for i in range(plan.nScales):
            l = plan.levels[i]
            got = det.read_tap(f, capi.TAP_CHNS, i, (plan.nChns, l.wC, l.hC))
            assert np.array_equal(cp.bits(got), cp.bits(chns[i])), (case, H, W, "frame", f, "raw channels level", i, float(np.abs(got - chns[i]).max()))


def run_case(case, optset, options, taps, approx=0):
    import torch
    from acf_amd.detector import HipDetector
    from oracle import binding as ob
    for H, W in cp.CASES[case][1]:
        exp = cp.expected(case, H, W, approx)
        max_hits = max(1 << 16, 2 * max(len(e["hits"]) for e in exp[1]))
        det = HipDetector(cp.model(case), H, W, 3, max_batch=cp.N_FRAMES, max_hits=max_hits, taps=taps)
        try:
            assert len(det.levels) == exp[0].nScales and det.nChns == exp[0].nChns
            for k, v in options.items():
                det.set_option(k, v)
            if approx:
                det.set_x86_tables(*ob.x86_fixture())
                det.set_option("arith", 1)
            det.set_option("profile", 1)
            det.run(torch.from_numpy(np.array(cp.frames(H, W))).cuda())
            prof = det.profile()
            print(case, optset, "%dx%d" % (H, W), "kernels:", " ".join(sorted(prof)))
            compare(det, case, H, W, exp, optset)
            if taps:
                compare_taps(det, case, H, W, exp[0])
            check_forms(case, optset, H, W, prof)
            if options.get("count_repairs"):
                r = det.repairs()
                print(case, optset, "%dx%d" % (H, W), "repairs (smoothing checked, redone, level checked, redone):", r)
                assert 0 <= r[1] <= r[0] and 0 <= r[3] <= r[2], r
                # planScale: only k_smooth_vec's chains are cut (colour planes smoothed, shrink 4); three segments of a plane that is
                # itself a multiple of 4 each way hand over twice.  planLevels: LV_COPY has no chain to cut.
                kw = cp.CASES[case][0]
                if kw.get("colorSmooth", 1) == 0 or not kw.get("colorEnabled", 1) or kw.get("shrink", 4) != 4:
                    assert r[0] == 0, r
                elif H % 4 == 0 and W % 4 == 0:
                    assert r[0] > 0, r
                if kw.get("smooth", 1) == 0:
                    assert r[2] == 0, r
        finally:
            det.close()


@pytest.mark.parametrize("optset", list(OPTION_SETS))
@pytest.mark.parametrize("case", list(cp.CASES))
def test_case_bit_exact(oracle, case, optset):
    options, taps = OPTION_SETS[optset]
    run_case(case, optset, options, taps)


@pytest.mark.parametrize("case", cp.ARITH_CASES)
def test_case_bit_exact_reference_arithmetic(oracle, case):
    """Option arith with one x86 CPU's rcpps / rsqrtps tables against the oracle under set_approx(3): the x86 instantiations of
    gradMag, gradMagNorm in k_chns and k_triy_chns."""
    run_case(case, "arith", dict(), False, approx=3)
