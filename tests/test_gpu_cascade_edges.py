"""The cascade's rule at every tree position, at the tie and at every stage end (tests/cascade_edges_case.py): designed models whose
hits a kernel loses or gains if it tests h <= cascThr anywhere but after each single tree, adds two neighbouring trees out of order,
or compares with `<`.  Every model under every form — float tiles, rank tiles (acf_hip_op_acf_detect1_rank), no tiles, one workgroup
per tile and persistent workgroups, the environment's forms in child processes, the pipeline with rank cells from the level kernel —
against the oracle in number, order, position and score bits; then HipDetector.cascade_forms() against the form the case is there
for.  The closing test holds the union of the reported records against the forks.  tests/test_cascade_edges.py holds the CPU side.

What the plan cannot reach from these shapes (written down, not asserted): NW 16 (only ACF_HIP_TILE_NW=16 selects it), NW 1 (a wave
of 64 lanes is below the sparse stage's 128 threads for a model of more than 64 sparse trees, and below TR x 2), passW 32 on the TINY
window (its lists fit with 64 at every NW), tailNodesLds != 0 (fixed to 0 at plan time), and k_cascade_tile3D on float cells at depth
1 (only ACF_HIP_TILED_POOLED1 selects it; tests/test_gpu_variants.py runs that form)."""
import os
import subprocess
import sys

import numpy as np
import pytest

import cascade_edges_case as ce

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
REPORTED = []
# (setting, depth, length): the four settings on the depth-2 lengths; no_tail_codes and tiled_staged change nothing at depth 2 (they
# are read for depths 1, 3, 4 only), so depth 3 runs them as well, where they select k_cascade_tail alone and k_cascade_tileD
CHILD = [(s, 2, n) for s in ce.CHILD_ENVS for n in ce.CHILD_LENGTHS] + \
        [(s, 3, n) for s in ce.CHILD_ENVS[1:3] for n in (33, 129)]


@pytest.fixture(scope="module")
def dev():
    from acf_amd.detector import HipDetector
    d = HipDetector()
    yield d
    d.close()


@pytest.mark.parametrize("depth,n", ce.GROUPS)
def test_every_position_under_every_form(dev, oracle, depth, n):
    REPORTED.extend(ce.run_group(dev, depth, n, ce.group_cases(depth, n)))


@pytest.mark.parametrize("n", ce.OVERFLOW)
def test_tail_overflow_on_float_and_rank_cells(dev, oracle, n):
    """every window reaches the tail: the first codes.cap through the leaf codes and their scan, the rest through the wave tail"""
    recs = ce.run_group(dev, 2, n, ce.overflow_cases(n))
    assert all(r["codes_cap"] == ce.CODES_CAP < r["qcap"] for r in recs)
    REPORTED.extend(recs)


@pytest.mark.parametrize("depth,n,option", [(0, 129, None), (3, 30, None), (1, 20, None), (2, 129, "rank_cells"), (2, 129, "cascade_tiles")])
def test_rank_entry_refuses_where_no_rank_cells_would_be_read(dev, depth, n, option):
    from acf_amd.detector import HipError
    family, pos = ce.group_cases(depth, n)[0]
    dev.set_model(ce.make_model(family, depth, n, pos))
    if option:
        dev.set_option(option, 0)
    try:
        with pytest.raises(HipError) as e:
            dev.op_acf_detect1_rank(np.array(ce.buffer()))
        assert e.value.code == 2, e.value   # ACF_HIP_E_UNSUPPORTED
    finally:
        if option:
            dev.set_option(option, 1)


@pytest.mark.parametrize("setting,depth,n", CHILD)
def test_environment_selected_forms(setting, depth, n):
    """a form only the environment selects: its own process (the environment is read once per process)"""
    k, v = setting.split("=", 1)
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "cascade_edges_case.py"), str(depth), str(n)], cwd=ROOT, env=dict(os.environ, **{k: v}),
                       capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and r.stdout.strip().endswith("ok %d %d" % (depth, n)), (setting, depth, n, r.stdout[-1500:], r.stderr[-3000:])


@pytest.mark.parametrize("name", sorted(ce.BIG_WINDOWS))
def test_big_windows_take_the_planned_waves(dev, oracle, name):
    """windows of 20 x 20 and 12 x 12 cells over 16 channels: the waves per workgroup and the sparse stage's pass width that the tile
    plan picks for each cell type, printed; float cells must take what tests/cascade_edges_case.py derives from buildTileSet's rule
    (20 x 20: NW 8 in more than 80 KiB, NOT fewer waves — NW 2 does not fit 80 KiB and NW 1 is below the sparse stage's threads;
    12 x 12: NW 4), rank cells fewer than eight waves at 20 x 20"""
    m, chns, want = ce.big_window_case(name)
    recs = {}
    for rank in (False, True):
        got, rec = ce.launch(dev, m, np.array(chns), dict(rank=rank, tiles=1, persist=1))
        recs[rank] = rec
        print("window %s, %s cells: NW %d passW %d TC %d tiles %d LDS %d" % (name, "rank" if rank else "float", rec["NW"], rec["passW"], rec["TC"], rec["nTiles"], rec["tileLds"]))
        assert len(want) > 0 and ce.same_hits(got, want), (name, rank, len(got), len(want))
        ce.check_forms(rec, dict(path="tiled2", kernel="tile3", rank=rank, b=(0, 16, 32, 32, 128), codeScan=True, waveTail=True), (name, rank))
        assert rec["TC"] == 2 * rec["NW"] and rec["passW"] in (32, 64)
    assert recs[False]["NW"] == ce.BIG_WINDOWS[name]["float_nw"], recs[False]
    assert (recs[False]["tileLds"] > 80 * 1024) == (name == "20x20")
    assert name != "20x20" or recs[True]["NW"] < 8
    REPORTED.extend(recs.values())


@pytest.mark.parametrize("H,W", ce.PIPE_SIZES)
@pytest.mark.parametrize("family,pos", ce.PIPE_MODELS)
def test_pipeline_levels_smaller_than_a_tile(oracle, family, pos, H, W):
    for n, keep, persist in ce.PIPE_RUNS:
        REPORTED.append(ce.pipe_run(family, pos, H, W, n, keep, persist))


def test_reported_records_cover_every_fork():
    """the union of what the launches above reported, not of what the table claims"""
    assert len(REPORTED) > 1000, "the coverage is that of the cases' own reports: run this file whole, in order and in one process"
    assert {r["path"] for r in REPORTED} == {"tiled2", "staged"}   # ("none": a buffer smaller than a window has no case here)
    assert {r["kernel"] for r in REPORTED} == {None, "tile3", "tile3D", "tileD"}
    for k in ("tile3", "tile3D"):
        on = [r for r in REPORTED if r["kernel"] == k]
        assert {r["rank"] for r in on} == {False, True} and {r["persist"] for r in on} == {False, True}, k
    assert {8} < {r["NW"] for r in REPORTED if r["kernel"]}
    assert {r["passW"] for r in REPORTED if r["kernel"] in ("tile3", "tile3D")} <= {32, 64}
    sparse = {(r["b"][4] - r["b"][2] > 32) + (r["b"][4] - r["b"][2] > 64) for r in REPORTED if r["kernel"] == "tile3"}
    assert sparse == {0, 1, 2}      # the sparse stage's thread-per-tree forms: up to 32, up to 64, more trees
    assert {(r["codeScan"], r["waveTail"]) for r in REPORTED if r["path"] == "tiled2"} == {(False, False), (True, True)}
    staged = [r for r in REPORTED if r["path"] == "staged"]
    assert {(r["codeScan"], r["pooledTail"], r["waveTail"]) for r in staged} == {(False, False, False), (False, False, True), (True, False, True), (True, True, True)}
    assert {r["frames"] for r in REPORTED} == {1, 2, 5}
