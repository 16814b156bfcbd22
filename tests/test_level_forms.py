"""CPU preconditions of tests/test_gpu_level_forms.py (tests/level_forms_case.py): the oracle's plan and the library's host plan
(acf_hip_plan_levels) have the level geometry every case claims — the heights, which levels are approximated, and from the ratios to
their real levels (tap counts restated from the reference's resampleCoef) the reasons against fusing each level carries and the mode
it takes; every case's cascade separates its windows (hit fraction strictly inside (0.05, 0.9)); and the case list stands on both
sides of every fork it names."""
import ctypes as C

import numpy as np
import pytest

from acf_amd import capi, synth

import level_forms_case as lf


def _host_levels(case):
    _, _, H, W = lf.CASES[case][:4]
    params, keep = capi.make_params(lf.model(case))
    lv = (capi.Level * 256)()
    n, nc = C.c_int(), C.c_int()
    assert capi.load().acf_hip_plan_levels(C.byref(params), H, W, 3, lv, 256, C.byref(n), C.byref(nc)) == 0
    return [lv[i] for i in range(n.value)], nc.value


@pytest.mark.parametrize("case", list(lf.CASES))
def test_case_geometry(oracle, case):
    plan, _ = lf.expected(case)
    host, nc = _host_levels(case)
    want = lf.parse_levels(case)
    assert len(host) == plan.nScales == len(want) and nc == plan.nChns == synth.n_channels(lf.model(case))
    path = lf.CASES[case][6]
    for i, w in enumerate(want):
        l = plan.levels[i]
        for fld, _ in capi.Level._fields_:
            assert getattr(host[i], fld) == getattr(l, fld), (i, fld)
        assert l.hC == w["hC"] and bool(l.isReal) == w["real"] and w["R"] == -(-l.hC // 64), (i, l.hC, l.isReal, w)
        assert lf.level_reasons(plan.levels, i) == w["why"], (i, lf.level_reasons(plan.levels, i), w["why"])
        if path in ("fused", "smooth_jobs", "copy"):
            # the mode of the plan's fused list: a real level is copied; an approximated one goes down or up on both axes
            if l.isReal:
                assert w["mode"] == "real", (i, w)
            else:
                lr = plan.levels[l.realIndex]
                ky, kx = lf.axis_taps(lr.hC, l.hC)[0], lf.axis_taps(lr.wC, l.wC)[0]
                yd, xd = ky == "down", kx == "down"   # (an exact axis is not "down")
                assert w["mode"] == ("dd" if xd and yd else "du" if xd else "ud" if yd else "uu"), (i, ky, kx, w)
        else:
            assert w["mode"] == "real", (i, w)
    reasons = {r for w in want for r in w["why"]}
    assert (path == "fused") == (not reasons and lf.CASES[case][1].get("smooth", 1) > 0 and lf.CASES[case][5].get("fused_levels", 1) == 1), (path, reasons)
    assert lf.CASES[case][7] == (path != "fused" and not all(w["real"] for w in want))


@pytest.mark.parametrize("case", list(lf.CASES))
def test_case_hit_fraction(oracle, case):
    plan, exp = lf.expected(case)
    for f, e in enumerate(exp):
        assert np.isfinite(e["pyr"]).all() and len(e["hits"]) > 0, f
        assert len(e["hits"]) < lf.CAP
    frac = lf.hit_fraction(case)
    print(case, "windows", lf.n_windows(case), "hit fraction %.4f" % frac)
    assert lf.HIT_LO < frac < lf.HIT_HI, frac


def test_axis_taps_restates_the_reference():
    """resampleCoef facts the cases stand on: k:1 is exact, up-sampling has no tap count, 24 -> 11 needs four taps where 17 -> 8 and
    18 -> 8 need three, ratios up to 1.6 need three at most"""
    assert lf.axis_taps(16, 8) == ("exact", 2) and lf.axis_taps(12, 4)[0] == "exact" and lf.axis_taps(8, 16) == ("up", 0)
    assert lf.axis_taps(24, 11) == ("down", 4) and lf.axis_taps(17, 8)[1] == 3 and lf.axis_taps(18, 8)[1] == 3
    assert lf.axis_taps(64, 60)[1] <= 3 and lf.axis_taps(192, 120) == ("down", 3)


def test_both_sides_of_every_fork():
    L = {c: lf.parse_levels(c) for c in lf.CASES}
    path = {c: lf.CASES[c][6] for c in lf.CASES}
    # rows per lane 1 .. 9 among the level kernels' jobs, real and approximated; a height past them
    assert {l["R"] for c in L for l in L[c] if l["real"] and l["by"]} == set(range(1, 10))
    assert {l["R"] for c in L for l in L[c] if not l["real"] and l["by"] and path[c] == "fused"} == set(range(1, 9))
    for a, b in ((64, 65), (256, 257), (512, 513), (576, 577)):
        for s in ("a7", "a0"):
            assert L["real_%d_%s" % (a, s)][0]["hC"] == a and L["real_%d_%s" % (b, s)][0]["hC"] == b
    assert L["approx_256"][1] == dict(L["approx_256"][1], hC=256, real=False, by="all") and L["approx_257"][1] == dict(L["approx_257"][1], hC=257, real=False, by="group")
    assert path["approx_512"] == "fused" and L["approx_512"][1]["hC"] == 512 and path["approx_513"] == "wave_smooth" and L["approx_513"][1]["why"] == ("rows",)
    assert path["real_576_a0"] == "fused" and path["real_577_a0"] == "smooth_jobs" and L["real_577_a0"][0]["why"] == ("tall",)
    # every reason alone on a level somewhere (the window bound at R = 1: see the case file), and the nearest plans with none
    alone = {l["why"] for c in L for l in L[c] if len(l["why"]) == 1}
    assert {("taps",), ("exact",), ("rows",), ("window",), ("tall",)} <= alone
    for c in ("neither_p1a1", "neither_p2a1", "neither_p4a3", "window_r2_below"):
        assert path[c] == "fused"
    assert "window" in L["window_r1_at"][5]["why"] and "window" not in L["window_r1_below"][5]["why"]
    assert L["window_r2_at"][3]["why"] == ("window",) and L["window_r2_below"][3]["why"] == ()
    # LM_DD and LM_UU among k_level_all's jobs and among the group jobs
    for by in ("all", "group"):
        assert {"dd", "uu"} <= {l["mode"] for c in L for l in L[c] if l["by"] == by and path[c] == "fused"}
    assert set(path.values()) == {"fused", "wave_smooth", "smooth_jobs", "copy"}
    # pad parity: the level kernels write the ranks on the second frame only
    for ph in (4, 12):
        for pw in (0, 4, 12):
            a, b = "pad_%d_%d_256" % (ph, pw), "pad_%d_%d_260" % (ph, pw)
            assert any(l["hC"] % 64 == 0 for l in L[a]) and not any(l["hC"] % 64 == 0 for l in L[b])
            runs = lf.runs(a)
            assert len(runs) == 4
            assert [lf.expect(a, r, 2)["emit_rank"] for r in runs] == [False] * 4
            assert [lf.expect(b, r, 2)["emit_rank"] for r in runs] == [bool(r["rank_cells"]) for r in runs]
            assert [lf.expect(b, r, 2)["emit_f32"] for r in runs] == [not (r["rank_cells"] and not r["keep_pyramid"]) for r in runs]
    # batches: the remainder of four frames per workgroup, and both sides of the eight frames that are cut into segments
    for c in ("batch_pad", "batch_group"):
        assert lf.batches(c) == (1, 4, 5, 8, 9)
        seg = [lf.expect(c, lf.runs(c)[0], n)["segments"] for n in lf.batches(c)]
        assert all(s > 1 for s in seg[:4]) and seg[4] == 1, seg
    assert {c for c in lf.CASES if lf.CASES[c][5].get("taps")} == {"taps_fused", "taps_wave_smooth", "taps_smooth_jobs", "taps_copy"}
    assert {path[c] for c in lf.CASES if lf.CASES[c][5].get("taps")} == set(path.values())
