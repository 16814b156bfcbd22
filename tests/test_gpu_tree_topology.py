"""Variable-depth trees (treeDepth 0) of every shape on the device: the child-pointer walk of casc_eval<0> (k_cascade_first / _queue),
k_cascade_tail<0> and tree_leaf (k_evaluate_window, crop_cascade, k_crop_score, k_evaluate_windows) against the oracle, and against the
device's own fixed-depth kernels on the equivalent full heap model — hits identical in number, order, position and score bits.  The
models carry garbage wherever a walk must not look (tests/tree_topology_case.py), so a read of a wrong node is a NaN score or a refusal.

tests/test_tree_topology.py holds the CPU side: the oracle against a plain walker, the hit fractions of these cases, and
acf_hip_check_model.  No test here calls an evaluating entry with a model that acf_hip_check_model rejects."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import crop_scores_case as cs
import tree_topology_case as tc
from acf_amd import capi
from acf_amd.modelio import write_cpb

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
# what option profile calls the kernels that only fixed-depth models reach: the tile kernels, the code-scan tails, the rank cells
TILE_LABELS = {"k_cascade_tile", "k_tail_scan", "k_cascade_tail3", "k_rank"}


@pytest.fixture(scope="module")
def dev():
    from acf_amd.detector import HipDetector
    d = HipDetector()
    d.set_option("profile", 1)
    yield d
    d.close()


def set_checked_model(dev, m, nChns=tc.NC):
    """nothing is launched on a model the host check rejects"""
    assert tc.check_model(m, nChns) == (0, "")
    dev.set_model(m)


def assert_hits_equal(got, want):
    assert len(got) == len(want), (len(got), len(want))
    for k in ("scale", "c", "r"):
        assert np.array_equal(got[k], want[k]), k
    assert np.array_equal(tc.bits(got["score"]), tc.bits(want["score"]))


def test_set_model_refuses_a_self_reference():
    """The one refusal that is tested on a context: acf_hip_set_model itself.  Nothing is called after it."""
    from acf_amd.detector import HipDetector
    m = tc.detect_model("mixed", 40)
    m["child"] = m["child"].copy()
    m["child"][5, 0] = 1
    d = HipDetector()
    try:
        params, keep = capi.make_params(m)
        rc = d.lib.acf_hip_set_model(d.ctx, C.byref(params))
        why = (d.lib.acf_hip_last_error(d.ctx) or b"").decode()
        assert rc == capi.E_INVALID, rc
        assert why.startswith("set_model: child[] of tree 5, node 0 is 1") and "after its parent" in why, why
    finally:
        d.close()


@pytest.mark.parametrize("nTrees", tc.TREE_COUNTS)
@pytest.mark.parametrize("shape", tc.SHAPES)
def test_op_acf_detect1(dev, oracle, shape, nTrees):
    """12 trees: one stage (k_cascade_first emits the hits); 16 / 17: a stage end and a one-tree last stage (k_cascade_queue); 40: three
    stages; 129 / 193 / 300: k_cascade_tail<0> on a one-tree tail, a partial and a whole-plus-partial 64-tree batch."""
    m = tc.detect_model(shape, nTrees)
    want = tc.oracle_detect1(oracle, m, tc.buffer_f32())
    assert abs(len(want) / tc.n_windows(m, tc.WP, tc.HP) - tc.CASES[(shape, nTrees)][0]) < 0.001
    set_checked_model(dev, m)
    dev.profile()
    got = dev.op_acf_detect1(tc.buffer_f32())
    names = set(dev.profile())
    assert_hits_equal(got, want)
    assert "k_cascade" in names and not (names & TILE_LABELS), sorted(names)


@pytest.mark.parametrize("nTrees", tc.TREE_COUNTS)
@pytest.mark.parametrize("shape", tc.SHAPES)
def test_op_acf_detect1_u8(dev, oracle, shape, nTrees):
    """byte planes and byte thresholds; odd tree counts let the library derive the bytes from the model's thrs (NaN and inf included)"""
    m = tc.detect_model(shape, nTrees)
    tu = oracle.thrs_u8(m["thrs"])
    want = tc.oracle_detect1(oracle, m, tc.buffer_u8(), tu)
    assert abs(len(want) / tc.n_windows(m, tc.WP, tc.HP) - tc.CASES[(shape, nTrees)][1]) < 0.001
    set_checked_model(dev, m)
    got = dev.op_acf_detect1_u8(tc.buffer_u8(), None if nTrees % 2 else tu)
    assert_hits_equal(got, want)


@pytest.mark.parametrize("nTrees", tc.PAD_TREES)
@pytest.mark.parametrize("D", tc.PAD_DEPTHS)
def test_variable_equals_padded_on_the_device(dev, oracle, D, nTrees):
    """device(variable) against device(pad_full(.., D)) with cascade_tiles 1: the child walk against the tile kernels (depth 2:
    k_cascade_tile3 and its tails; 1 and 3: k_cascade_tileD in front of the staged kernels) and the code-scan tail (193 trees), with no
    checker in between; floats and bytes."""
    m = tc.detect_model("mixed", nTrees, maxDepth=D)
    p = tc.pad_full(m, D)
    dev.set_option("cascade_tiles", 1)
    set_checked_model(dev, m)
    dev.profile()
    a = dev.op_acf_detect1(tc.buffer_f32())
    va = set(dev.profile())
    a8 = dev.op_acf_detect1_u8(tc.buffer_u8())
    set_checked_model(dev, p)
    b = dev.op_acf_detect1(tc.buffer_f32())
    vb = set(dev.profile())
    b8 = dev.op_acf_detect1_u8(tc.buffer_u8())
    print("D", D, "trees", nTrees, "variable:", sorted(va), "padded:", sorted(vb))
    assert 0 < len(a) < tc.n_windows(m, tc.WP, tc.HP)
    assert_hits_equal(a, b)
    assert_hits_equal(a8, b8)
    assert_hits_equal(a, tc.oracle_detect1(oracle, m, tc.buffer_f32()))
    assert not (va & TILE_LABELS), sorted(va)
    if D == 2:
        assert "k_cascade_tile" in vb, sorted(vb)


@pytest.mark.parametrize("shape", tc.EVAL_SHAPES)
def test_op_evaluate(dev, oracle, shape):
    """k_evaluate_window on the window at (0, 0) of the (10, 9, 7) buffer at cascThr 0 and at a full pass; both an early stop and a full
    pass occur (one_node: every root a leaf; bare: the first tree's)."""
    seen = set()
    for k in range(len(tc.EVAL_LEAVES)):
        m, chns = tc.eval_model(shape, k), tc.eval_buffer(k)
        set_checked_model(dev, m)
        for thr in (0.0, cs.FULL):
            got = dev.op_evaluate(chns, thr)
            want = tc.oracle_evaluate(oracle, m, chns, thr)
            assert tc.bits(got) == tc.bits(want), (k, thr, got, want)
        seen.add(bool(tc.oracle_evaluate(oracle, m, chns, 0.0) > 0))
    assert seen == {True, False}
    if shape == "bare":
        assert m["child"][0, 0] == 0


@pytest.mark.parametrize("shape", tc.CROP_SHAPES)
def test_evaluate_crops(dev, oracle, shape):
    """16 crops of 16 x 16 (k_crop_score: crop_cascade's tree_leaf on the cells in LDS), the early stop and the full pass"""
    batch = cs.crops(16, 16, "luv")
    dev.profile()
    for early, thr in ((False, cs.FULL), (True, 0.0)):
        m = tc.crop_model(shape, early)
        set_checked_model(dev, m)
        want = cs.oracle_scores(oracle, m, m, batch, thr)
        got = dev.evaluate_crops(batch, None, thr)
        assert np.array_equal(cs.bits(got), cs.bits(want)), (early, got, want)
    assert "k_crop_score" in dev.profile()


@pytest.mark.parametrize("shape", tc.CROP_SHAPES)
def test_evaluate_crops_u8(dev, oracle, shape):
    imgs = tc.crop_bytes()
    planes = np.stack([oracle.ingest_u8(im, capi.PIX_RGB) for im in imgs])
    for early, thr in ((False, cs.FULL), (True, 0.0)):
        m = tc.crop_model_u8(shape, early)
        set_checked_model(dev, m)
        got = dev.evaluate_crops_u8(np.array(imgs), capi.PIX_RGB, cascThr=thr)
        assert np.array_equal(cs.bits(got), cs.bits(cs.oracle_scores(oracle, m, m, planes, thr))), (early, got)


# ------------------------------------------------------------------ the planned pipeline

def nms_params():
    return capi.make_nms(type="maxg", overlap=0.65, ovrDnm="min", prune=True, maxCount=40, pruneRatio=0.1)


# name -> (options, detector keywords, model stride, frames to run, read the float levels, runs, device NMS)
PIPE_SETS = {
    "batch3": (dict(), dict(max_batch=3), 4, (0, 1, 2), True, 1, False),
    "streams2": (dict(), dict(max_batch=4, streams=2), 4, (0, 1, 2, 0), True, 1, False),
    "stride2": (dict(), dict(max_batch=3), 2, (0, 1, 2), True, 1, False),
    "no_pyramid_rank_cells": (dict(keep_pyramid=0, rank_cells=1), dict(max_batch=3), 4, (0, 1, 2), False, 1, False),
    "graph_twice": (dict(graph=1), dict(max_batch=3), 4, (0, 1, 2), True, 2, False),
    "device_nms": (dict(), dict(max_batch=3), 4, (0, 1, 2), True, 1, True),
}


@pytest.mark.parametrize("optset", list(PIPE_SETS))
@pytest.mark.parametrize("name", list(tc.PIPE_MODELS))
def test_planned_pipeline(oracle, name, optset):
    """acf_hip_plan + acf_hip_run on TINY frames of 200 x 264: every level bit for bit, hits and boxes as bytes.  The profile shows the
    staged cascade (its label k_cascade covers k_cascade_first, k_cascade_queue and, past 128 trees, k_cascade_tail: a hit of the
    193-tree model has passed all three) and no tile kernel, code-scan tail or rank pass."""
    import torch
    from acf_amd.detector import HipDetector
    options, kw, stride, which, levels, runs, nms = PIPE_SETS[optset]
    m = tc.pipe_model(name, stride=stride)
    assert tc.check_model(m, tc.NC) == (0, "")
    plan, exp, _ = tc.pipe_expected(name, stride)
    frames = torch.from_numpy(np.array(tc.pipe_frames())[list(which)]).cuda()
    det = HipDetector(m, tc.PIPE_H, tc.PIPE_W, 3, max_hits=1 << 16, **kw)
    try:
        assert len(det.levels) == plan.nScales and det.nChns == plan.nChns
        for k, v in options.items():
            det.set_option(k, v)
        single = kw.get("streams", 1) == 1
        if single:
            det.set_option("profile", 1)
        if nms:
            det.set_nms(nms_params())
        for rep in range(runs):
            det.run(frames)
            for f, src in enumerate(which):
                e = exp[src]
                where = (name, optset, "run", rep, "frame", f)
                if levels:
                    for i in range(plan.nScales):
                        assert np.array_equal(tc.bits(det.read_level(f, i)), tc.bits(plan.level_view(e["pyr"], i))), where + ("level", i)
                got, got_hits = det.detections(f)
                assert len(e["hits"]) > 0
                if nms:
                    r = e["det"]
                    keep = oracle.nms(np.stack([r["x"], r["y"], r["w"], r["h"]], axis=1), r["score"].astype(np.float64), nms_params())
                    assert 1 <= len(keep) < len(r) <= capi.NMS_CAP
                    assert det.raw_detections(f).tobytes() == r.tobytes(), where
                    assert got.tobytes() == r[keep].tobytes(), where
                else:
                    assert got_hits.tobytes() == e["hits"].tobytes(), where + (len(got_hits), len(e["hits"]))
                    assert got.tobytes() == e["det"].tobytes(), where
        if single:
            names = set(det.profile())
            print(name, optset, "kernels:", " ".join(sorted(names)))
            assert "k_cascade" in names and not (names & TILE_LABELS), sorted(names)
    finally:
        det.close()


# ------------------------------------------------------------------ the C++ host

@pytest.fixture(scope="module")
def cli():
    host = os.path.join(ROOT, "acf_amd", "host")
    subprocess.check_call(["make", "-s", "-C", host])
    return os.path.join(host, "acf_hip_detect")


def run_cli(cli, tmp_path, m, batch, extra):
    n, d, W, H = batch.shape
    write_cpb(str(tmp_path / "m.cpb"), m)
    (tmp_path / "f.raw").write_bytes(np.ascontiguousarray(batch).tobytes())
    e = dict(os.environ)
    e["ACF_HIP_LIBRARY"] = capi.LIB_PATH
    p = subprocess.run([cli, "--model", str(tmp_path / "m.cpb"), "--frames", str(tmp_path / "f.raw"), "--rows", str(W), "--cols", str(H),
                        "--channels", str(d), "--count", str(n), "--luv"] + extra, env=e, stdout=subprocess.PIPE, stderr=subprocess.PIPE,
                       universal_newlines=True, timeout=120)
    assert p.returncode == 0, p.stderr
    return p.stdout.splitlines()


def test_cli_detects_from_a_scattered_cpb(cli, oracle, tmp_path):
    """acf::HipDetector after ModelIO has read a `.cpb` whose pairs are out of heap order, with unused slots and garbage between them"""
    m = tc.cpp_model()
    assert tc.check_model(m, tc.NC) == (0, "")
    frames = np.array(tc.cpp_frames())
    lines = [l.split() for l in run_cli(cli, tmp_path, m, frames, [])]
    plan = oracle.Plan(m, tc.CPP_H, tc.CPP_W, 3)
    got = []
    for t in lines:
        if t[0] == "frame":
            got.append([])
        else:
            got[-1].append((int(t[0]), int(t[1]), int(t[2]), int(t[3]), int(t[5], 16)))
    assert len(got) == tc.CPP_FRAMES
    for f in range(tc.CPP_FRAMES):
        pyr, _, _ = oracle.chns_pyramid(plan, frames[f])
        det, _ = oracle.detect(plan, pyr)
        want = [(int(d["x"]), int(d["y"]), int(d["w"]), int(d["h"]), int(np.float32(d["score"]).view(np.uint32))) for d in det]
        assert len(want) > 0 and got[f] == want


def test_cli_scores_crops_from_a_scattered_cpb(cli, oracle, tmp_path):
    """--score-crops: acf::HipDetector::evaluateCrops with the model's channels, cascThr 0; crops that stop early and crops that pass"""
    m = tc.crop_model("scattered", True)
    assert tc.check_model(m, tc.NC) == (0, "")
    batch = np.array(cs.crops(16, 16, "luv"))
    lines = run_cli(cli, tmp_path, m, batch, ["--score-crops"])
    got = np.array([int(l.split()[3], 16) for l in lines if l.startswith("crop ")], np.uint32)
    assert np.array_equal(got, cs.bits(cs.oracle_scores(oracle, m, m, batch, 0.0)))
