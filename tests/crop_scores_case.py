"""Shared by tests/test_crop_scores.py (CPU) and tests/test_gpu_crop_scores.py: the models, crops and oracle scores of
Detector::evaluate(const cv::Mat&) on batches of crops.  Expected value everywhere: oracle.chns_compute(chns model, crop), then
acfo_evaluate on those channels with the scoring model, compared as bits."""
import ctypes as C
import functools

import numpy as np

from acf_amd import capi, synth

FULL = -1e30     # cascThr of the full pass: every tree is walked
N_TREES = 128


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def model(early=False, **kw):
    """synth.make_model(seed=3, nTrees=128, ..); early: leaves with which cascThr = 0 stops some crops early and lets others pass."""
    m = synth.make_model(seed=3, nTrees=N_TREES, **kw)
    if early:
        hs = m["hs"]
        m["hs"] = (-0.05 + 0.35 * synth.uniform(6, hs.size)).astype(np.float32).reshape(hs.shape)
    return m


@functools.lru_cache(maxsize=None)
def crops(H, W, kind, n=16, first=100):
    a = np.stack([synth.make_frame(first + k, H, W, kind) for k in range(n)])
    a.setflags(write=False)
    return a


def oracle_scores(oracle, score_model, chns_model, crop_batch, cascThr):
    """-> (scores float32 [n], trees walked is not reported: a score > cascThr after the last tree is a full pass)"""
    prm, keep = capi.make_params(score_model)
    out = np.zeros(len(crop_batch), np.float32)
    for i, crop in enumerate(crop_batch):
        chns = np.ascontiguousarray(oracle.chns_compute(chns_model, crop), np.float32)
        nC, wC, hC = chns.shape
        out[i] = oracle.lib().acfo_evaluate(oracle.F(chns), hC, wC, nC, C.byref(prm), np.float32(cascThr))
    return out


def stopped_early(oracle, score_model, chns_model, crop_batch):
    """per crop: cascThr = 0 ended the walk before the last tree (the score then differs from the walk that ignores cascThr
    only if it stopped; equal scores with a final score <= 0 stopped at the last tree, which is a full walk all the same)"""
    s0 = oracle_scores(oracle, score_model, chns_model, crop_batch, 0.0)
    sf = oracle_scores(oracle, score_model, chns_model, crop_batch, FULL)
    return bits(s0) != bits(sf)


# (id, make_model keywords, H, W, frame kind, planes): the base models and shapes
BASE = [
    ("tiny_luv_16", dict(name="TINY", isLuv=1), 16, 16, "luv", 3),            # window == crop; the smallest plane normRad 5 takes
    ("face80_rgb_80", dict(name="FACE80"), 80, 80, "rgb", 3),
    ("inria_rgb_128x64", dict(name="INRIA"), 128, 64, "rgb", 3),
    ("face64_gray_64", dict(name="FACE64"), 64, 64, "gray", 1),
    ("face80_rgb_87x83", dict(name="FACE80"), 87, 83, "rgb", 3),     # cropped to 84 x 80: the window is smaller than the plane
]
# the same on TINY, one channel option each
VARIANTS = [
    ("shrink2", dict(name="TINY", isLuv=1, shrink=2, stride=2), 16, 16, "luv", 3),
    ("orients9_full", dict(name="TINY", isLuv=1, nOrients=9, full=1), 32, 32, "luv", 3),
    ("hardbin", dict(name="TINY", isLuv=1, softBin=-2), 16, 16, "luv", 3),
    ("no_norm", dict(name="TINY", isLuv=1, normRad=0), 16, 16, "luv", 3),
    ("no_color", dict(name="TINY", isLuv=1, colorEnabled=0), 16, 16, "luv", 3),
    ("no_hist", dict(name="TINY", isLuv=1, gradHistEnabled=0), 32, 32, "luv", 3),
    ("hsv", dict(name="TINY", colorSpace=capi.CS_HSV, isLuv=0), 16, 16, "rgb", 3),
    ("orig", dict(name="TINY", colorSpace=capi.CS_ORIG, isLuv=0), 16, 16, "rgb", 3),
    ("depth0", dict(name="TINY", isLuv=1, treeDepth=0), 16, 16, "luv", 3),
    ("depth3", dict(name="TINY", isLuv=1, treeDepth=3), 16, 16, "luv", 3),
]
# the models whose early-stop leaves give BOTH outcomes among crops 0..15 (asserted on the oracle by tests/test_crop_scores.py)
EARLY = BASE[:4] + [("face80_depth0_80", dict(name="FACE80", treeDepth=0), 80, 80, "rgb", 3)]
