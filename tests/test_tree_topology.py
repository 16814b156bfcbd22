"""Variable-depth trees (treeDepth 0, the child-pointer walk) of every shape — the CPU side: the oracle against a plain Python walker
and against the equivalent full-depth heap model, the conditions the GPU tests (tests/test_gpu_tree_topology.py) rest on (hit
fractions, both outcomes of the early stop), acf_hip_check_model's refusals and acceptances, and the model files.  The cases live in
tests/tree_topology_case.py."""
import os
import re
import subprocess

import numpy as np
import pytest

import crop_scores_case as cs
import tree_topology_case as tc
from acf_amd import capi
from acf_amd.modelio import read_cpb, write_cpb, write_model

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HOST = os.path.join(ROOT, "acf_amd", "host")

# every shape at 40 trees, and at 193 the two whose trees differ by index (bare roots at 127 / 128 / 192)
WALKER_CASES = [(s, 40) for s in tc.SHAPES] + [("bare", 193), ("mixed", 193)]


# ------------------------------------------------------------------ the generator itself

@pytest.mark.parametrize("shape", tc.SHAPES)
def test_generator_builds_the_shape_and_the_garbage(shape):
    n = 193
    m = tc.detect_model(shape, n)
    depth, nodes = tc.GEOMETRY[shape]
    child, fids, thrs, hs = m["child"], m["fids"], m["thrs"], m["hs"]
    assert child.shape == (n, nodes) == fids.shape == thrs.shape == hs.shape
    role = tc.roles(m)
    assert tc.depth_of(m) == depth
    # parent-first, inside the row
    t, k = np.nonzero(child)
    assert (child[t, k] < nodes).all() and (child[t, k].astype(np.int64) - 1 > k).all()
    # garbage where no walk looks
    assert (fids[role == tc.LEAF] == tc.BAD_FID).all() and np.isnan(thrs[role == tc.LEAF]).all() and np.isfinite(hs[role == tc.LEAF]).all()
    assert np.isnan(hs[role == tc.TEST]).all() and (fids[role == tc.TEST] < tc.NC * 16).all() and np.isfinite(thrs[role == tc.TEST]).all()
    unused = role == tc.UNUSED
    assert (child[unused] == 0).all() and (fids[unused] >= 1 << 31).all() and np.isinf(thrs[unused]).all() and np.isnan(hs[unused]).all()
    bare_roots = np.nonzero(child[:, 0] == 0)[0].tolist()
    if shape == "bare":
        assert bare_roots == [0, 15, 16, 31, 32, 127, 128, n - 1]
    elif shape == "one_node":
        assert bare_roots == list(range(n))
    else:
        assert bare_roots == []
    if shape == "sparse":
        assert unused.mean() > 0.97 and (child.max(axis=1) == nodes - 1).all()      # a handful of 511 slots, the last pair at the row's end
    if shape == "scattered":
        # not breadth-first: some tree's right-hand child owns an earlier pair than its left-hand sibling; and slots are skipped
        assert unused.any() and any(child[t, child[t, 0]] and child[t, child[t, 0] - 1] and child[t, child[t, 0]] < child[t, child[t, 0] - 1]
                                    for t in range(n))
    if shape == "chain":
        assert ((role == tc.TEST).sum(axis=1) == 8).all()
    if shape in ("heap2", "heap3"):
        assert (child[:, :(1 << depth) - 1] == 2 * np.arange((1 << depth) - 1) + 2).all() and not unused.any()
    if shape == "mixed":
        leaf_depths = {tc.depth_of(dict(child=child[t:t + 1])) for t in range(n)}
        assert leaf_depths == {1, 2, 3, 4}   # walk lengths differ from tree to tree


def test_generator_is_reproducible():
    a, b = tc.detect_model("scattered", 40), tc.detect_model("scattered", 40)
    for k in ("fids", "thrs", "hs", "child"):
        assert a[k].tobytes() == b[k].tobytes()


# ------------------------------------------------------------------ the oracle against the plain walker

@pytest.mark.parametrize("shape,nTrees", WALKER_CASES)
def test_oracle_detect1_equals_the_walker(oracle, shape, nTrees):
    """acfo_acf_detect1 against leaves summed in f32 in tree order until h <= cascThr: same hits, same order, same score bits — on the
    float buffer and on the byte buffer with byte thresholds."""
    m = tc.detect_model(shape, nTrees)
    want = tc.walk_hits(tc.buffer_f32(), m)
    got = tc.oracle_detect1(oracle, m, tc.buffer_f32())
    assert np.isfinite(got["score"]).all()
    assert got.tobytes() == want.tobytes(), (len(got), len(want))
    tu = oracle.thrs_u8(m["thrs"])
    want8 = tc.walk_hits(tc.buffer_u8(), m, thrs=tu)
    got8 = tc.oracle_detect1(oracle, m, tc.buffer_u8(), tu)
    assert got8.tobytes() == want8.tobytes(), (len(got8), len(want8))


@pytest.mark.parametrize("shape", tc.SHAPES)
def test_windows_at_a_time_walker_equals_the_walk_from_the_root(shape):
    """walk_hits takes all windows of a tree at a time; walk() is the plain loop on one window.  Three windows, hit or not."""
    m = tc.detect_model(shape, 40)
    chns = tc.buffer_f32()
    hits = tc.walk_hits(chns, m)
    by_pos = {(int(h["c"]), int(h["r"])): h["score"] for h in hits}
    for c, r in ((0, 0), (23, 17), (56, 40)):
        s = tc.score_window(chns[:, c:c + 4, r:r + 4], m, m["cascThr"])
        if (c, r) in by_pos:
            assert tc.bits(s) == tc.bits(by_pos[(c, r)])
        else:
            assert s <= np.float32(m["cascThr"])


@pytest.mark.parametrize("shape", tc.EVAL_SHAPES)
def test_oracle_evaluate_equals_the_walker_and_gives_both_outcomes(oracle, shape):
    """acfo_evaluate on the window at (0, 0) against the walker at cascThr 0 and at a full pass; over the four leaf ranges both an early
    stop and a full pass occur (what the GPU test of op_evaluate relies on)."""
    seen = set()
    for k in range(len(tc.EVAL_LEAVES)):
        m, chns = tc.eval_model(shape, k), tc.eval_buffer(k)
        for thr in (0.0, cs.FULL):
            got = tc.oracle_evaluate(oracle, m, chns, thr)
            assert np.isfinite(got) and tc.bits(got) == tc.bits(tc.score_window(chns[:, :4, :4], m, thr)), (k, thr)
        seen.add(bool(tc.oracle_evaluate(oracle, m, chns, 0.0) > 0))
    assert seen == {True, False}


# ------------------------------------------------------------------ the oracle against the padded model

@pytest.mark.parametrize("shape,nTrees", WALKER_CASES)
def test_oracle_variable_equals_padded(oracle, shape, nTrees):
    m = tc.detect_model(shape, nTrees)
    D = max(1, tc.depth_of(m))
    p = tc.pad_full(m, D)
    assert p["treeDepth"] == D and p["fids"].shape == (nTrees, (1 << (D + 1)) - 1) and np.isfinite(p["thrs"]).all() and np.isfinite(p["hs"]).all()
    assert tc.oracle_detect1(oracle, m, tc.buffer_f32()).tobytes() == tc.oracle_detect1(oracle, p, tc.buffer_f32()).tobytes()
    tu, tup = oracle.thrs_u8(m["thrs"]), oracle.thrs_u8(p["thrs"])
    assert tc.oracle_detect1(oracle, m, tc.buffer_u8(), tu).tobytes() == tc.oracle_detect1(oracle, p, tc.buffer_u8(), tup).tobytes()


@pytest.mark.parametrize("nTrees", tc.PAD_TREES)
@pytest.mark.parametrize("D", tc.PAD_DEPTHS)
def test_oracle_mixed_equals_padded_at_every_depth(oracle, D, nTrees):
    """the models of the GPU's variable-against-padded comparison: equal on the oracle, and the hit fraction is inside the band"""
    m = tc.detect_model("mixed", nTrees, maxDepth=D)
    assert tc.depth_of(m) == D
    a = tc.oracle_detect1(oracle, m, tc.buffer_f32())
    assert a.tobytes() == tc.oracle_detect1(oracle, tc.pad_full(m, D), tc.buffer_f32()).tobytes()
    assert 0.01 <= len(a) / tc.n_windows(m, tc.WP, tc.HP) <= 0.90
    with pytest.raises(ValueError):
        tc.pad_full(tc.detect_model("mixed", nTrees, maxDepth=D + 1), D)


# ------------------------------------------------------------------ the conditions of the GPU cases

def test_case_table_is_complete():
    assert sorted(tc.CASES) == sorted((s, n) for s in tc.SHAPES for n in tc.TREE_COUNTS)


@pytest.mark.parametrize("shape", tc.SHAPES)
def test_hit_fractions(oracle, shape):
    """The oracle's hit fraction of every detect case, float and byte buffer: the recorded one, and inside [0.01, 0.90] — a case whose
    windows all pass or all fail compares nothing.  one_node: every tree is one leaf and all windows score alike, so its cases keep
    every window (1.0) and compare every score."""
    nw = tc.n_windows(tc.detect_model(shape, 12), tc.WP, tc.HP)
    assert nw == 57 * 41
    for n in tc.TREE_COUNTS:
        m = tc.detect_model(shape, n)
        f32 = len(tc.oracle_detect1(oracle, m, tc.buffer_f32())) / nw
        u8 = len(tc.oracle_detect1(oracle, m, tc.buffer_u8(), oracle.thrs_u8(m["thrs"]))) / nw
        print(shape, n, "cascThr %.4f" % m["cascThr"], "hit fraction %.3f (f32) %.3f (u8)" % (f32, u8))
        assert (round(f32, 3), round(u8, 3)) == tc.CASES[(shape, n)], (n, f32, u8)
        if shape == "one_node":
            assert f32 == 1.0 and u8 == 1.0
        else:
            assert 0.01 <= f32 <= 0.90 and 0.01 <= u8 <= 0.90, (n, f32, u8)


@pytest.mark.parametrize("name", list(tc.PIPE_MODELS))
def test_pipeline_hit_fractions(oracle, name):
    """the planned pipeline's cases: the oracle's hits over all windows of all levels, per frame; at stride 2 (the dedup path) too.
    mixed193: some window is still alive after 128 trees (the wave-per-window tail has work)."""
    plan, exp, nwin = tc.pipe_expected(name)
    frac = tuple(round(len(e["hits"]) / nwin, 3) for e in exp)
    print(name, "levels", plan.nScales, "windows", nwin, "hit fractions", frac)
    assert frac == tc.PIPE_FRACTIONS[name]
    assert all(0.01 <= f <= 0.90 for f in frac)
    _, exp2, nwin2 = tc.pipe_expected(name, 2)
    assert nwin2 > 3 * nwin and all(0.01 <= len(e["hits"]) / nwin2 <= 0.90 for e in exp2)
    assert len({e["hits"].tobytes() for e in exp}) == tc.PIPE_FRAMES   # three different frames, three different results


@pytest.mark.parametrize("shape", tc.CROP_SHAPES)
def test_crop_models_give_both_outcomes(oracle, shape):
    batch = cs.crops(16, 16, "luv")
    m = tc.crop_model(shape, True)
    stopped = cs.stopped_early(oracle, m, m, batch)
    assert stopped.any() and (~stopped).any(), stopped
    full = tc.crop_model(shape, False)
    s = cs.oracle_scores(oracle, full, full, batch, cs.FULL)
    assert np.isfinite(s).all() and len(set(cs.bits(s).tolist())) == 16


@pytest.mark.parametrize("shape", tc.CROP_SHAPES)
def test_byte_crop_models_give_both_outcomes(oracle, shape):
    planes = np.stack([oracle.ingest_u8(im, capi.PIX_RGB) for im in tc.crop_bytes()])
    m = tc.crop_model_u8(shape, True)
    stopped = cs.stopped_early(oracle, m, m, planes)
    assert stopped.any() and (~stopped).any(), stopped


def test_cpp_case_has_hits_in_the_band(oracle):
    m = tc.cpp_model()
    plan = oracle.Plan(m, tc.CPP_H, tc.CPP_W, 3)
    nwin = sum(int(plan.levels[i].nWinR) * int(plan.levels[i].nWinC) for i in range(plan.nScales))
    for f in tc.cpp_frames():
        pyr, _, _ = oracle.chns_pyramid(plan, f)
        det, _ = oracle.detect(plan, pyr)
        assert 0.01 <= len(det) / nwin <= 0.90, (len(det), nwin)


# ------------------------------------------------------------------ acf_hip_check_model

@pytest.mark.parametrize("shape", tc.SHAPES)
def test_check_model_accepts_every_shape_with_its_garbage(shape):
    for n in (12, 193):
        assert tc.check_model(tc.detect_model(shape, n), tc.NC) == (0, "")
        assert tc.check_model(tc.detect_model(shape, n), 0) == (0, "")
    assert tc.check_model(tc.pad_full(tc.detect_model(shape, 40), max(1, tc.GEOMETRY[shape][0])), tc.NC) == (0, "")


def _first_test_node(m, below_root=False):
    role = tc.roles(m)
    t, k = np.nonzero((role == tc.TEST) & (np.arange(role.shape[1]) >= (3 if below_root else 0)))
    return int(t[0]), int(k[0])


def _defect(name):
    """-> (model, nChns of the check)"""
    m = tc.detect_model("mixed", 40)
    m["child"], m["fids"] = m["child"].copy(), m["fids"].copy()
    nodes = m["child"].shape[1]
    if name == "self_reference":
        m["child"][5, 0] = 1                         # ftr < thr leads from node 0 to node 0
    elif name == "backward_pointer":
        t, k = _first_test_node(m, below_root=True)
        m["child"][t, k] = 2                         # the root's own pair
    elif name == "two_node_cycle":
        t, k = _first_test_node(m, below_root=True)
        j = int(m["child"][t, k])                    # k -> (j - 1, j); j -> (k, k + 1)
        m["child"][t, j] = k + 1
    elif name == "child_equals_nTreeNodes":
        m["child"][39, 0] = nodes
    elif name == "fid_at_nF":
        t, k = _first_test_node(m)
        m["fids"][t, k] = tc.NC * 16
    elif name == "fewer_channels":
        return m, 4
    return m, tc.NC


@pytest.mark.parametrize("defect", ["self_reference", "backward_pointer", "two_node_cycle", "child_equals_nTreeNodes", "fid_at_nF", "fewer_channels"])
def test_check_model_refuses(defect):
    m, nChns = _defect(defect)
    rc, why = tc.check_model(m, nChns)
    assert rc == capi.E_INVALID, defect
    if defect in ("fid_at_nF", "fewer_channels"):
        assert "feature id" in why and "child[]" not in why, why
        assert tc.check_model(m, 0) == (0, "")       # structure only: the channels are not known
        if defect == "fewer_channels":
            assert tc.check_model(m, tc.NC) == (0, "") and (m["fids"][tc.roles(m) == tc.TEST] >= 4 * 16).any()
    else:
        assert "child[]" in why and "after its parent" in why, why
        assert tc.check_model(m, 0)[0] == capi.E_INVALID


def test_check_model_does_not_inspect_leaves_of_fixed_depths():
    m = tc.pad_full(tc.detect_model("mixed", 40), 4)
    m["fids"] = m["fids"].copy()
    m["fids"][:, 15:] = tc.BAD_FID
    assert tc.check_model(m, tc.NC) == (0, "")
    m["fids"][7, 14] = tc.NC * 16
    assert tc.check_model(m, tc.NC)[0] == capi.E_INVALID


def test_check_model_arguments():
    import ctypes as C
    lib = capi.load()
    why = C.create_string_buffer(8)
    assert lib.acf_hip_check_model(None, 0, why, 8) == capi.E_INVALID and why.value
    m, _ = _defect("self_reference")
    params, keep = capi.make_params(m)
    assert lib.acf_hip_check_model(C.byref(params), 0, None, 0) == capi.E_INVALID
    assert lib.acf_hip_check_model(C.byref(params), 0, why, 8) == capi.E_INVALID and len(why.value) == 7   # cut to cap, terminated
    assert lib.acf_hip_check_model(C.byref(params), -1, None, 0) == capi.E_INVALID


def test_the_entry_is_declared_in_every_list():
    n = "acf_hip_check_model"
    header = open(os.path.join(ROOT, "include", "acf_hip.h")).read()
    assert re.search(r"ACF_HIP_API int %s\(" % n, header)
    assert n in capi.DECLARED_SYMBOLS
    for f in ("acf_hip_loader.h", "acf_hip_loader.cpp"):
        assert "ACF_HIP_FN(%s)" % n in open(os.path.join(ROOT, "acf_amd", "host", f)).read(), f
    assert "#define ACF_HIP_ABI_VERSION 9" in header     # additive: the version stays


def _body(src, head):
    """the text of the function that starts with `head`, up to the next line that closes it at column 0"""
    at = src.index(head)
    return src[at:src.index("\n}\n", at)]


def test_the_check_comes_before_anything_is_stored_allocated_or_launched():
    """Call order, by reading: acf_hip_set_model checks before it copies the arrays; acf_hip_op_evaluate checks its own channel count
    before it allocates or launches (its refusal is not tested by launching: a regression would be a hang or a wild read on a device
    that others share); the plan's and op_acf_detect1's tables check first of all."""
    csrc = os.path.join(ROOT, "acf_amd", "csrc")
    main = open(os.path.join(csrc, "acf_hip.hip")).read()
    b = _body(main, "int acf_hip_set_model(")
    assert 0 < b.index("checkModel(*p, 0,") < b.index("c->p = *p") < b.index("c->child.assign") < b.index("c->hasModel = true")
    b = _body(open(os.path.join(csrc, "ops.hip.h")).read(), "int acf_hip_op_evaluate(")
    assert 0 < b.index("checkModel(p, nChns,") < b.index("Scratch s;") < b.index("s.upload(") < b.index("hipLaunchKernelGGL(k_evaluate_window")
    b = _body(open(os.path.join(csrc, "cascade_plan.hip.h")).read(), "static int buildCascadeTables(")
    assert 0 < b.index("checkModel(p, nChns, cell,") < b.index("std::vector<uint8_t> internal")
    assert "hipMalloc" not in b[:b.index("checkModel(")] and "devUpload" not in b[:b.index("checkModel(")]
    # the crops entries take the model from the context alone (what acf_hip_set_model accepted) and compare its largest test's
    # feature id before the first launch
    b = _body(open(os.path.join(csrc, "crops_run.hip.h")).read(), "int planCropCall(")
    assert 0 < b.index("needModel(c") < b.index("ensureCropModel(c)") < b.index("c->crop.fidMax")
    assert "hipLaunchKernelGGL" not in b


# ------------------------------------------------------------------ model files

@pytest.fixture(scope="module")
def cli():
    subprocess.check_call(["make", "-s", "-C", HOST])
    return os.path.join(HOST, "acf_hip_detect")


@pytest.mark.parametrize("shape", ["sparse", "scattered", "one_node"])
def test_model_files_round_trip(cli, tmp_path, shape):
    """`.cpb` and ACFHIPM1 with nTreeNodes 511 / 40 / 1 and the garbage in place: Python (acf_amd/modelio.py) and C++ (ModelIO) write the
    same bytes and read each other's files, NaN payloads and 0xFFFFFFFF feature ids included."""
    m = tc.detect_model(shape, 17)
    write_model(str(tmp_path / "m.acfm"), m)
    write_cpb(str(tmp_path / "py.cpb"), m)
    subprocess.check_call([cli, "--convert", str(tmp_path / "m.acfm"), "--out", str(tmp_path / "cc.cpb")])
    py = (tmp_path / "py.cpb").read_bytes()
    assert (tmp_path / "cc.cpb").read_bytes() == py
    subprocess.check_call([cli, "--convert", str(tmp_path / "py.cpb"), "--out", str(tmp_path / "cc2.cpb")])
    assert (tmp_path / "cc2.cpb").read_bytes() == py
    got, _, _ = read_cpb(str(tmp_path / "cc.cpb"))
    assert got["treeDepth"] == 0 and got["fids"].shape == m["fids"].shape
    for k in ("fids", "child"):
        assert np.asarray(got[k]).astype(np.uint32).tobytes() == m[k].tobytes(), k
    for k in ("thrs", "hs"):
        assert np.asarray(got[k]).astype(np.float32).tobytes() == m[k].tobytes(), k
    assert got["cascThr"] == m["cascThr"]
    assert tc.check_model(dict(m, **{k: got[k] for k in ("fids", "thrs", "hs", "child")}), tc.NC) == (0, "")
