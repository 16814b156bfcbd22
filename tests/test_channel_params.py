"""CPU preconditions of tests/test_gpu_channel_params.py (tests/channel_params_case.py): every case's oracle plan builds, its pyramid
is finite, its cascade separates the windows (hit fraction strictly inside (0.05, 0.9) — a case outside it checks nothing and has to
be re-tuned), the parameter reaches the result (the pyramid differs from the baseline's), and the library's host-side plan
(acf_hip_plan_levels) is the oracle's, field by field."""
import ctypes as C

import numpy as np
import pytest

from acf_amd import capi

import channel_params_case as cp

CASE_SIZES = [(case, H, W) for case, (_, sizes) in cp.CASES.items() for H, W in sizes]


@pytest.mark.parametrize("case,H,W", CASE_SIZES)
def test_case_preconditions(oracle, case, H, W):
    plan, exp = cp.expected(case, H, W)
    assert plan.nScales > 0 and len(plan.real) > 0
    for f, e in enumerate(exp):
        assert np.isfinite(e["pyr"]).all(), f
        if e["ldcf"] is not None:
            assert np.isfinite(e["ldcf"][1]).all(), f
        assert len(e["hits"]) > 0, f
    frac = cp.hit_fraction(case, H, W)
    print(case, H, W, "windows", cp.n_windows(case, H, W), "hit fraction %.4f" % frac)
    assert cp.HIT_LO < frac < cp.HIT_HI, frac
    if case != "baseline" and (H, W) in cp.CASES["baseline"][1]:
        _, base = cp.expected("baseline", H, W)
        for e, b in zip(exp, base):
            assert e["pyr"].shape != b["pyr"].shape or not np.array_equal(cp.bits(e["pyr"]), cp.bits(b["pyr"])), \
                "the case's pyramid is the baseline's: the parameter does not reach the result"


@pytest.mark.parametrize("case,H,W", CASE_SIZES)
def test_plan_levels_match_oracle(oracle, case, H, W):
    plan, _ = cp.expected(case, H, W)
    params, keep = capi.make_params(cp.model(case))
    lv = (capi.Level * 256)()
    n, nc = C.c_int(), C.c_int()
    assert capi.load().acf_hip_plan_levels(C.byref(params), H, W, 3, lv, 256, C.byref(n), C.byref(nc)) == 0
    assert n.value == plan.nScales and nc.value == plan.nChns
    for i in range(n.value):
        for fld, _ in capi.Level._fields_:
            assert getattr(lv[i], fld) == getattr(plan.levels[i], fld), (i, fld)


def test_channel_counts_cover_the_range(oracle):
    """The cases move the channel count between 1 and 16 (what the tile cascade, the rank-cell tables and the LDS sizes depend on)."""
    counts = {cp.expected(case, *sizes[-1])[0].nChns for case, (_, sizes) in cp.CASES.items()}
    assert {1, 3, 4, 5, 7, 8, 9, 10, 11, 13, 16} <= counts, sorted(counts)
