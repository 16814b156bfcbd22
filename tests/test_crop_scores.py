"""Detector::evaluate(const cv::Mat&) on batches of crops — the CPU side: the preconditions the GPU tests
(tests/test_gpu_crop_scores.py) rest on, checked on the oracle alone, so that those tests cannot go vacuous; and the lists every
layer keeps of the two new entries."""
import os
import re

import numpy as np
import pytest

import crop_scores_case as cs
from acf_amd import capi, synth

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.parametrize("case", cs.BASE + cs.VARIANTS, ids=lambda c: c[0])
def test_full_pass_gives_sixteen_distinct_scores(oracle, case):
    """cascThr = -1e30 walks every tree: 16 crops, 16 different scores, so one wrong cell anywhere shows in some score."""
    _, kw, H, W, kind, d = case
    m = cs.model(**kw)
    s = cs.oracle_scores(oracle, m, m, cs.crops(H, W, kind), cs.FULL)
    assert len(set(cs.bits(s).tolist())) == 16


@pytest.mark.parametrize("case", cs.EARLY, ids=lambda c: c[0])
def test_early_stop_leaves_give_both_outcomes(oracle, case):
    """cascThr = 0 with the early-stop leaves: at least one crop of 0..15 stops before the last tree and at least one walks them all."""
    _, kw, H, W, kind, d = case
    m = cs.model(early=True, **kw)
    stopped = cs.stopped_early(oracle, m, m, cs.crops(H, W, kind))
    assert stopped.any() and (~stopped).any(), stopped


def test_stock_leaves_stop_every_crop_at_once(oracle):
    """... which the stock leaves do not: with them cascThr = 0 ends every walk, the reason for the leaves above."""
    m = cs.model(name="FACE80")
    assert cs.stopped_early(oracle, m, m, cs.crops(80, 80, "rgb")).all()


def test_toolbox_default_channels_score_differently(oracle):
    """FACE80 on the toolbox defaults' channels (computeChannels) against its own: no score of the 16 coincides."""
    m = cs.model(name="FACE80")
    dfl = synth.make_model(seed=3, name="TINY", nTrees=16, isLuv=0)
    a = cs.oracle_scores(oracle, m, m, cs.crops(80, 80, "rgb"), cs.FULL)
    b = cs.oracle_scores(oracle, m, dfl, cs.crops(80, 80, "rgb"), cs.FULL)
    assert not (cs.bits(a) == cs.bits(b)).any()


def test_the_entries_are_declared_in_every_list():
    names = ["acf_hip_evaluate_crops", "acf_hip_evaluate_crops_u8"]
    header = open(os.path.join(ROOT, "include", "acf_hip.h")).read()
    for n in names:
        assert re.search(r"ACF_HIP_API int %s\(" % n, header), n
        assert n in capi.DECLARED_SYMBOLS
        for f in ("acf_hip_loader.h", "acf_hip_loader.cpp"):
            assert "ACF_HIP_FN(%s)" % n in open(os.path.join(ROOT, "acf_amd", "host", f)).read(), (n, f)
    assert "#define ACF_HIP_ABI_VERSION 9" in header     # additive: the version stays
