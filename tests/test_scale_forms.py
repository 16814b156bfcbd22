"""CPU preconditions of tests/test_gpu_scale_forms.py (tests/scale_forms_case.py): from the oracle's plan every case has the real
scales, sources, adoption, axis kinds and tap counts that give, by the rules restated in the case file, the route, SLOW, xt and the
refusal reasons it claims; every case's cascade separates its windows (hit fraction strictly inside (0.05, 0.9)); and the case list
stands on both sides of every fork it names."""
import numpy as np
import pytest

import scale_forms_case as sf


@pytest.mark.parametrize("case", list(sf.CASES))
def test_case_geometry(oracle, case):
    _, kw, H, W, _, run, n, _ = sf.CASES[case]
    tok = sf.parse_scales(case)
    rs = sf.real_scales(sf.oracle_plan(case), sf.model(case), H, W)
    want = sf.rules(case)
    assert len(tok) == len(rs) == len(want)
    for k, (t, s, r) in enumerate(zip(tok, rs, want)):
        where = (case, "real scale", k, t, r)
        assert (t["h"], t["w"]) == (s["h"], s["w"]), where
        assert (t["route"], t["slow"], t["xt2"]) == (r["route"], r["slow"], r["xt2"]), where
        # the plan's side: a plan that was not asked for neither holds nor is refused; one that was holds or names its reason, which
        # is the restated one wherever tap counts tell (no_tiling: none of them)
        for held, why, asked, cheap in ((t["plan_strip"], t["why"], r["asked"], r["cheap"]), (t["plan_pair"], t["why_pair"], r["asked_pair"], r["cheap_pair"])):
            assert asked == (held or why is not None) and not (held and why), where
            assert why == cheap or (why == "no_tiling" and cheap is None), where
        assert (t["nty"] > 0) == (t["n_split"] > 0) == (t["route"] in ("strip", "strip_pair_a")), where
        assert t["n_split"] <= max(1, -(-s["w"] // sf.RS_XO) // 8), where
        if t["route"] in ("strip", "strip_pair_a"):
            assert s["src_h"] % 4 == 0 and s["src_h"] >= 8, where


@pytest.mark.parametrize("case", list(sf.CASES))
def test_case_hit_fraction(oracle, case):
    plan, exp = sf.expected(case)
    for f, e in enumerate(exp):
        assert np.isfinite(e["pyr"]).all() and len(e["hits"]) > 0, f
        assert len(e["hits"]) < sf.CAP
    frac = sf.hit_fraction(case)
    print(case, "windows", sf.n_windows(case), "hit fraction %.4f" % frac)
    assert sf.HIT_LO < frac < sf.HIT_HI, frac


def shaped_like_1080p(rs):
    """the real scales k whose pair (k, k + 1) could be launched with 1080p's ratios: y in [1.9, 2) and [3.9, 4.1], B a quarter in x"""
    out = []
    for k in range(len(rs) - 1):
        a, b = rs[k], rs[k + 1]
        if a["resampled"] and b["resampled"] and not a["adopt"] and a["src"] == b["src"] and b["w"] <= a["w"] and b["h"] <= a["h"]:
            ya, yb = a["src_h"] / a["h"], b["src_h"] / b["h"]
            if 1.9 <= ya < 2.0 and 3.9 <= yb <= 4.1 and b["src_w"] == 4 * b["w"] and sf.cheap_reason(a) is None and sf.cheap_reason(a, b) is None:
                out.append(k)
    return out


def test_geometries_the_cases_stand_on(oracle):
    T = {c: sf.parse_scales(c) for c in sf.CASES}
    R = {c: sf.real_scales(sf.oracle_plan(c), sf.model(c), sf.CASES[c][2], sf.CASES[c][3]) for c in sf.CASES}
    # 128 x 192: scale 1 is 64 x 96, adopted, the exact half of the frame
    assert (R["half_fused"][1]["h"], R["half_fused"][1]["w"], R["half_fused"][1]["adopt"], R["half_fused"][1]["src"]) == (64, 96, True, 0)
    # 136 x 200, nApprox 0: nothing but scale 0 is adopted; scale 8 is its exact half and HALF, scales 1 and 2 are 184 and 172 columns:
    # ceil(172 / 2) = 86 steps of B against ceil(184 / 4) = 46 of A
    r = R["half_not_adopted"]
    assert [s["adopt"] for s in r] == [True] + [False] * (len(r) - 1) and all(s["src"] == 0 for s in r[1:])
    assert (r[8]["h"], r[8]["w"]) == (68, 100) and sf.exact_half(r[8]) and T["half_not_adopted"][8]["route"] == "half"
    assert (r[1]["w"], r[2]["w"]) == (184, 172) and T["half_not_adopted"][1]["why_pair"] == "b_steps"
    # ... with nPerOct 1 scale 0.5 is adopted all the same
    assert R["adopt_nperoct_1"][1]["adopt"] and R["adopt_nperoct_1"][2]["src"] == 1
    # the blocked pairing: (2, 3) holds a pair plan, 2 is HALF_FUSED, 3 runs alone and (3, 4), same source, was never asked for
    t, r = T["pair_blocked"], R["pair_blocked"]
    assert t[2]["plan_pair"] and t[2]["route"] == "half_fused" and t[3]["route"] == "strip" and not t[3]["plan_pair"] and t[3]["why_pair"] is None
    assert r[3]["src"] == r[4]["src"] == 1 and sf.cheap_reason(r[3], r[4]) is not None
    # 200 x 264: 52 x 68 from 100 x 132; 264 x 392: scale 3 at an x ratio of 4.1
    assert (R["strip_fast_b2"][2]["h"], R["strip_fast_b2"][2]["w"], R["strip_fast_b2"][2]["src_h"], R["strip_fast_b2"][2]["src_w"]) == (52, 68, 100, 132)
    s = R["x_taps"][3]
    assert 4.0 < s["src_w"] / s["w"] < 4.2 and T["x_taps"][3]["why"] == "x_taps"
    # the pair shaped like 1080p's: A about 1.94 in y, B about 4.1, x 1.9 and exactly 4; SLOW through B
    a, b = R["pair_slow_b2"][2], R["pair_slow_b2"][3]
    assert not sf.is_slow(a) and sf.is_slow(b) and sf.axes(b)[1][0] == "exact" and b["src_w"] == 4 * b["w"] and a["w"] >= 64
    # B's row tiles from the reported nty, and B's steps against A's
    for c, want in sf.PAIR_NTY_B.items():
        k = [t["route"] for t in T[c]].index("strip_pair_a")
        assert sf.nty_b(R[c][k], R[c][k + 1], T[c][k]["nty"]) == want <= T[c][k]["nty"], c
    k = [t["route"] for t in T["pair_fast"]].index("strip_pair_a")
    assert -(-R["pair_fast"][k + 1]["w"] // 2) == -(-R["pair_fast"][k]["w"] // 4) - 1 and not sf.is_slow(R["pair_fast"][k]) and not sf.is_slow(R["pair_fast"][k + 1])
    assert T["pair_no_tiling"][1]["why_pair"] == "no_tiling" and sf.cheap_reason(R["pair_no_tiling"][1], R["pair_no_tiling"][2]) is None
    # 240 x 320, where the issue looked for the blocked pairing: with TINY its pair (2, 3) is refused by x_taps
    m240 = sf.synth.make_model(**dict(sf.TINY, cascThr=-2.0))
    r240 = sf.real_scales(oracle.Plan(m240, 240, 320, 3), m240, 240, 320)
    assert [(s["h"], s["w"]) for s in r240] == [(240, 320), (120, 160), (60, 80), (28, 36)] and sf.cheap_reason(r240[2], r240[3]) == "x_taps"
    # 156 x 160 is the smallest frame of the grid shaped like 1080p: no smaller one has a pair with those ratios that tap counts admit
    assert shaped_like_1080p(R["pair_1080p_smallest"]) == [1]
    for H in range(16, 401, 4):
        for W in range(16, min(400, 156 * 160 // H) + 1, 4):
            if H * W < 156 * 160:
                assert not shaped_like_1080p(sf.real_scales(oracle.Plan(m240, H, W, 3), m240, H, W)), (H, W)
    for c in ("pair_slow_b1", "pair_slow_b2", "pair_slow_b5", "pair_nty4"):
        assert [x["route"] for x in T[c][2:4]] == ["strip_pair_a", "pair_b"] and T[c][2]["slow"] and T[c][2]["n_split"] >= 2
    for c in ("pair_off_streams", "pair_off_taps", "pair_off_env"):
        assert [x["route"] for x in T[c][2:4]] == ["strip", "strip"], c
    assert T["pair_off_streams"][2]["plan_pair"] and T["pair_off_taps"][2]["plan_pair"] and not T["pair_off_env"][2]["plan_pair"]
    assert T["pair_nty4"][2]["nty"] >= 2
    # up, barely up, mixed
    assert sf.axes(R["up_x2"][0]) == (("up", 0), ("up", 0)) and R["up_x2"][0]["h"] == 2 * 64
    assert (R["up_barely"][0]["h"], R["up_barely"][0]["w"]) == (132, 176) and T["up_barely"][1]["why"] == "rows"
    y, x = sf.axes(R["mixed"][0])
    assert (y[0], x[0]) == ("up", "down") and R["mixed"][0]["h"] == R["mixed"][0]["src_h"] and T["mixed"][0]["route"] == "generic"


def test_both_sides_of_every_fork():
    T = {c: sf.parse_scales(c) for c in sf.CASES}
    flat = [t for c in T for t in T[c]]
    assert {t["route"] for t in flat} == set(sf.ROUTES)
    assert {t["slow"] for t in flat if t["route"] == "strip"} == {False, True}
    assert {t["nty"] >= 2 for t in flat if t["nty"]} == {False, True} and {t["n_split"] >= 2 for t in flat if t["n_split"]} == {False, True}
    reached = {t[k] for t in flat for k in ("why", "why_pair")} - {None}
    assert reached == set(sf.REACHED) and not reached & set(sf.UNREACHABLE)
    # ... which are the reasons the scan reached, alone or in a pair; the others it never reached
    scanned = {w for w in sf.WHYS if sf.SCAN["alone"][w] + sf.SCAN["pair"][w] > 0}
    assert scanned == set(sf.REACHED) and set(sf.WHYS) - scanned == set(sf.UNREACHABLE)
    assert sf.SCAN["alone"]["no_tiling"] == 0 and not any(t["why"] == "no_tiling" for t in flat) and any(t["why_pair"] == "no_tiling" for t in flat)
    # launched pairs: <true, false> and <true, true>, ntyB equal to nty and below it, B's steps equal to A's and fewer
    pairs = {c: [t for t in T[c] if t["route"] == "strip_pair_a"] for c in T}
    assert {c for c in pairs if pairs[c]} == set(sf.PAIR_NTY_B)
    assert {(p[0]["slow"], sf.PAIR_NTY_B[c] < p[0]["nty"]) for c, p in pairs.items() if p} == {(s, b) for s in (False, True) for b in (False, True)}
    # HALF_FUSED against HALF on one frame; the three switches that turn a planned pair off; batches of 1, 2 and 5
    assert T["half_fused"][1]["route"] == "half_fused" and T["half_fused_smooth_0"][1]["route"] == T["half_taps"][1]["route"] == "half"
    for stem in ("strip_fast", "pair_slow"):
        assert [sf.CASES["%s_b%d" % (stem, n)][6] for n in (1, 2, 5)] == [1, 2, 5]
    assert {sf.CASES[c][5]["env"] for c in sf.CASES if "env" in sf.CASES[c][5]} == {"resample_no_up", "resample_generic", "resample_no_strip", "resample_no_pair"}
