"""CPU preconditions of tests/test_gpu_cascade_edges.py (tests/cascade_edges_case.py), with the oracle alone: the numpy restatement of
evaluate() equals acfo_acf_detect1 as bits on every operator case, the hit share lies in (0.05, 0.9), and every designed position
matters — leaving out its h <= cascThr test (dips), exchanging its pair (bumps) or turning its <= into < (ties) changes at least 32
windows of the hit list.  These are conditions on the inputs, not measurements of the library."""
import numpy as np
import pytest

import cascade_edges_case as ce


@pytest.mark.parametrize("depth,n", ce.GROUPS)
def test_every_position_of_the_group_matters(oracle, depth, n):
    for family, pos in ce.group_cases(depth, n):
        r = ce.check_conditions(family, depth, n, pos)
        assert set(r["changes"]) == {T for T in pos if family == "tie" or T != n - 1}


@pytest.mark.parametrize("n", ce.OVERFLOW)
def test_overflow_models_fill_the_tail_beyond_the_leaf_codes(oracle, n):
    """no position before tree 128: more windows than codes.cap pass tree 127 (check_conditions asserts it), and the positions at the
    tail's start, around the end of its first 64-tree code row and at the last tree still matter"""
    seen = set()
    for family, pos in ce.overflow_cases(n):
        assert min(pos) >= 128
        ce.check_conditions(family, 2, n, pos, overflow=True)
        seen |= set(pos)
    assert seen == {t for t in (128, 129, 190, 191, 192, 193, n - 1) if t < n}


@pytest.mark.parametrize("depth,n", ce.GROUPS)
def test_positions_cover_every_tree(depth, n):
    cases = ce.group_cases(depth, n)
    for family in ("dip", "bump"):
        models = [pos for f, pos in cases if f == family]
        assert sorted(t for pos in models for t in pos) == ce.positions(n)          # every tree once
        assert all(len(pos) <= 8 and all(b - a >= 2 for a, b in zip(pos, pos[1:])) for pos in models)
        assert any(pos[-1] == n - 1 for pos in models)                             # the length's last tree is a position
    ties = sorted(t for f, pos in cases if f == "tie" for t in pos)
    assert ties == ce.tie_positions(n) and {0, n - 1} <= set(ties)
    assert {t for t in (15, 16, 31, 32, 127, 128) if t < n} <= set(ties)


@pytest.mark.parametrize("name", sorted(ce.BIG_WINDOWS))
def test_big_window_models_meet_the_conditions(oracle, name):
    ce.big_window_conditions(name)


@pytest.mark.parametrize("H,W", ce.PIPE_SIZES)
@pytest.mark.parametrize("family,pos", ce.PIPE_MODELS)
def test_pipeline_models_meet_the_conditions(oracle, family, pos, H, W):
    """multi-level: the restatement equals the oracle's hits on all five frames, and every position's mutant changes at least 8 hits in
    some frame"""
    ce.pipe_check_conditions(family, pos, H, W)


def test_pipeline_plans_end_in_levels_smaller_than_a_tile():
    """the point of the pipeline cases: levels of fewer windows than a tile's 32 rows x 16 columns, down to two windows (96 x 128:
    1 x 2; a 3 : 4 frame has no level of 4 x 4 cells) and to a single window (96 x 96)"""
    from oracle import binding as ob
    last = {}
    for H, W in ce.PIPE_SIZES:
        plan = ob.Plan(ce.make_model("dip", 2, ce.PIPE_TREES, (0,)), H, W, 3)
        wins = [(plan.levels[i].nWinR, plan.levels[i].nWinC) for i in range(plan.nScales)]
        assert plan.nScales >= 12 and all(r >= 1 and c >= 1 for r, c in wins)
        assert all(r < 32 for r, c in wins) and sum(c < 16 for r, c in wins) >= 6
        last[(H, W)] = wins[-1]
    assert last == {(96, 128): (1, 2), (96, 96): (1, 1)}


def test_the_restatement_sees_each_mutant_class():
    """evaluate()'s three mutants on a model small enough to read: a skipped test resurrects the dip's class, the exchanged pair loses
    the bump's, the strict comparison keeps the tie's"""
    F, nWr = ce.buffer_features()
    for family, kw in (("dip", dict(skip=(3,))), ("bump", dict(swap=3)), ("tie", dict(strict=(3,)))):
        lv = ce.leaf_values(ce.make_model(family, 2, 8, (3,)), F)
        hit, _, left = ce.evaluate(lv)
        mut = ce.evaluate(lv, **kw)[0]
        gone = (left == 3).sum()
        assert gone >= ce.MIN_CHANGE
        if family == "dip":
            assert (mut & ~hit).sum() == gone and not (hit & ~mut).any()
        elif family == "bump":
            assert (hit & ~mut).sum() == hit.sum() and not (mut & ~hit).any()     # (the whole right class leaves at the exchanged tree)
        else:
            assert (mut & ~hit).sum() == gone and not (hit & ~mut).any()


def test_forms_table_is_consistent():
    """expect_forms' restatement of the plan on the stage ends it is there for"""
    f = dict(rank=False, tiles=1, persist=1, tall=False)
    assert ce.expect_forms(2, 128, f)["waveTail"] is False and ce.expect_forms(2, 129, f)["codeScan"] is True
    assert ce.expect_forms(2, 17, f)["b"] == (0, 16, 17, 17, 17)
    assert ce.expect_forms(3, 30, f)["kernel"] == "tileD" and ce.expect_forms(1, 30, f)["kernel"] is None
    assert ce.expect_forms(3, 33, f)["kernel"] == "tile3D" and ce.expect_forms(3, 33, f)["firstStage"] == 3
    assert ce.expect_forms(1, 33, f)["kernel"] == "tileD" and ce.expect_forms(1, 33, f)["firstStage"] == 2
    assert ce.expect_forms(4, 129, f)["pooledTail"] is True and ce.expect_forms(1, 129, f)["pooledTail"] is False
    assert ce.expect_forms(1, 129, f)["codeScan"] is True and ce.expect_forms(0, 129, dict(f, tiles=0))["codeScan"] is False
    assert not ce.rank_supported(0, 129) and not ce.rank_supported(3, 30) and ce.rank_supported(1, 32)
    assert np.float32(ce.CASC_THR + ce.Q) > np.float32(ce.CASC_THR)
