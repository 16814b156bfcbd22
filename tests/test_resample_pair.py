"""CPU preconditions of tests/test_gpu_resample_pair.py (tests/resample_pair_case.py): every shape has the property it is chosen for,
from tap counts restated from the reference's resampleCoef, and the case list stands on both sides of every fork it names."""
import pytest

import resample_pair_case as rp


@pytest.mark.parametrize("case", list(rp.CASES))
def test_case_properties(case):
    ha, wa, hbA, wbA, hbB, wbB, d, props, word = rp.CASES[case]
    assert ha * wa <= 640 * 128 and hbB <= hbA and wbB <= wbA and d in (1, 2, 3)
    (yA, xA), (yB, xB) = rp.axes(ha, wa, hbA, wbA), rp.axes(ha, wa, hbB, wbB)
    for key, got in (("yA", yA), ("xA", xA), ("yB", yB), ("xB", xB)):
        want = props.get(key)
        if want is not None:
            assert (got[0] if isinstance(want, str) else got) == want, (key, got, want)
    sA, sB = rp.slow(ha, hbA), rp.slow(ha, hbB)
    assert props.get("slowA", sA) == sA and props.get("slowB", sB) == sB, (sA, sB)
    why = rp.cheap_reason(ha, wa, hbA, wbA, hbB, wbB)
    if word["pair"]:
        assert why is None and word["slow"] == (sA or sB), (why, sA, sB)
        assert word["n_steps"] == -(-wbA // 4) and word["n_steps_b"] == -(-wbB // 2) and word["n_steps_b"] <= word["n_steps"]
        assert 1 <= word["nty_b"] <= word["nty"] and 1 <= word["n_split"] <= max(1, word["n_steps"] // 8)
        # a row tile holds an even number of A's rows and half as many of B's
        yt = (-(-hbA // word["nty"]) + 1) // 2 * 2
        assert -(-hbA // yt) == word["nty"] and -(-hbB // (yt // 2)) == word["nty_b"], yt
    else:
        assert why == word["why"] or (why is None and word["why"] == "no_tiling"), (why, word["why"])


def test_both_sides_of_every_fork():
    C = rp.CASES
    on = {c: v[8] for c, v in C.items() if v[8]["pair"]}
    # <true, false> and <true, true>; A fast with B slow, and both slow
    assert {w["slow"] for w in on.values()} == {False, True}
    assert C["slow_b_only"][7] == dict(C["slow_b_only"][7], slowA=False, slowB=True) and C["slow_both_anisotropic"][7]["slowA"]
    # every residue of wbA mod 4 with wbB odd and even; odd heights
    assert {(v[3] % 4, v[5] % 2) for c, v in C.items() if c.startswith("wa")} == {(r, p) for r in range(4) for p in range(2)}
    assert C["heights_odd"][2] % 2 == 1 and C["heights_odd"][4] % 2 == 1
    # B's steps equal to, below and one above A's
    assert on["wa0_wb_even"]["n_steps_b"] == on["wa0_wb_even"]["n_steps"] and on["b_steps_below"]["n_steps_b"] == on["b_steps_below"]["n_steps"] - 1
    assert C["b_steps_above"][8]["why"] == "b_steps" and -(-C["b_steps_above"][5] // 2) == -(-C["b_steps_above"][3] // 4) + 1
    # row tiles
    assert {w["nty"] for w in on.values()} >= {1, 3, 5, 8}
    assert any(w["nty"] >= 2 and w["nty_b"] == w["nty"] for w in on.values()) and any(w["nty"] >= 2 and w["nty_b"] < w["nty"] for w in on.values())
    # column segments beside B, with a segment that has fewer steps of B than of A
    for c in ("split2_d1", "split2_d2", "split2_d3", "split5_nty2_d3"):
        w = on[c]
        per = -(-w["n_steps"] // w["n_split"])
        assert C[c][3] >= 64 and w["n_split"] >= 2 and w["n_steps_b"] < w["n_steps"] and w["n_steps_b"] % per != 0
    assert {C[c][6] for c in on} == {1, 2, 3}
    assert C["ha8"][0] == 8 and on["ha8"]["pair"] and C["ha10_rows"][0] % 4 != 0
    assert {v[8]["why"] for v in C.values() if not v[8]["pair"]} == {"not_down", "rows", "slow_taps", "x_taps", "b_steps", "no_tiling"}
