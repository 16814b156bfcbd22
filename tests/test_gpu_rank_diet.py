"""The level kernels' rank cells after their diet (slots as 0x8000 - tlow, packed adds, the clamp on the raw bucket index, no select
for negative cells unless the model holds a zero threshold) and the filter without its edge-column selects, against the oracle.
Cases, models and frames: tests/rank_diet_case.py.

CPU: every rank case separates its windows (hit fraction strictly inside (0.05, 0.9)); the models are what the cases say (a zero
threshold in a colour and a histogram channel; at least 600 distinct thresholds per channel taken from the oracle's cells, on
which the host's rank tables are exact and have records with seven slots in use); the edge frames' real and approximated levels
have widths of every residue modulo 4.
GPU: rank cells of every level (border included) == searchsorted on the oracle's float level, hits, scores and boxes == the
oracle's, with keep_pyramid 1 (floats compared as bits too) and 0; the edge frames the same with one frame, uncut and cut in
column segments.

Hit fractions measured with the oracle (five frames of a set together; 128 x 192 / 130 x 175):
  tiny  a 0.183 / 0.241   b 0.234 / 0.341  c 0.092 / 0.141
  zero  a 0.258 / 0.345   b 0.329 / 0.423  c 0.683 / 0.726
  cells a 0.388 / 0.401   b 0.361 / 0.368  c 0.258 / 0.269
"""
import numpy as np
import pytest

import level_forms_case as lf
import rank_diet_case as rd
from test_rank_cells import host_ranks


@pytest.mark.parametrize("name,H,W,s", rd.RANK_CASES)
def test_case_hit_fraction(oracle, name, H, W, s):
    plan, exp = rd.expected(name, H, W, s)
    for e in exp:
        assert np.isfinite(e["pyr"]).all() and len(e["hits"]) < rd.CAP
    frac = rd.hit_fraction(plan, exp)
    print(name, H, W, s, "windows", rd.n_windows(plan), "hit fraction %.4f" % frac, [len(e["hits"]) for e in exp])
    assert rd.HIT_LO < frac < rd.HIT_HI, frac
    if s == "b":
        # most colour cells of the set are negative, in every level
        for e in exp:
            for i in range(plan.nScales):
                assert (plan.level_view(e["pyr"], i)[:3] < 0).mean() > 0.5
    if s == "c":
        for f in (0, 1, 4):   # colour cells of +0.0 or -0.0 only
            assert not any(plan.level_view(exp[f]["pyr"], i)[:3].any() for i in range(plan.nScales))


@pytest.mark.parametrize("H,W", rd.SIZES)
def test_models_are_what_the_cases_say(oracle, H, W):
    nC = rd.N_CHNS
    tiny, zero, cells = (rd.base_model(n, H, W) for n in rd.MODELS)
    for z in range(nC):
        assert (lf.channel_thresholds(tiny, nC, z) > 0).all()
        assert (lf.channel_thresholds(zero, nC, z)[0] == 0) == (z in (0, 5)), z
    plan, exp = rd.expected("cells", H, W, "a")
    full = 0
    for z in range(nC):
        t = lf.channel_thresholds(cells, nC, z)
        assert len(t) >= 600 and (t > 0).all(), (z, len(t))
        lv = np.concatenate([plan.level_view(e["pyr"], i)[z].ravel() for e in exp for i in range(plan.nScales)])
        assert np.isin(lv, t).sum() >= 200, z   # equality with a threshold happens on these frames
        v = np.concatenate([t, lv[:4000]])
        rc, got, _, info = host_ranks(cells, nC, z, v)
        assert rc == 0 and info[0] == 1 and info[3] == len(t), (z, info)
        assert np.array_equal(got, np.searchsorted(t, v, side="right").astype(np.uint16)), z
        # thresholds per bucket of 2^shift float patterns (info[1] = the channel's shift)
        full += int((np.unique(t.view(np.uint32) >> info[1], return_counts=True)[1] >= 6).sum())
    assert full > 0


def test_edge_frames_cover_every_tail(oracle):
    real, approx = set(), set()
    for H, W in rd.EDGE_SIZES:
        plan, _, e = rd.edge_expected(H, W)
        assert 64 <= W <= 96 and len(e["hits"]) > 0
        for i in range(plan.nScales):
            assert lf.level_reasons(plan.levels, i) == (), (H, W, i)   # the fused path
            (real if plan.levels[i].isReal else approx).add(plan.levels[i].wC % 4)
    assert real == {0, 1, 2, 3} and approx == {0, 1, 2, 3}, (real, approx)
    # with a warm-up of four columns a level of 16 / 24 columns is cut in two / three
    assert rd.edge_expected(128, 64)[0].levels[0].wC == 16 and rd.edge_expected(128, 96)[0].levels[0].wC == 24


# ------------------------------------------------------------------ GPU

@pytest.mark.gpu
@pytest.mark.parametrize("keep", [1, 0])
@pytest.mark.parametrize("name,H,W,s", rd.RANK_CASES)
def test_gpu_rank_cells_and_detections(oracle, name, H, W, s, keep):
    import torch
    from acf_amd.detector import HipDetector, HipError
    plan, exp = rd.expected(name, H, W, s)
    m = rd.model(name, H, W, s)
    max_hits = max(1 << 14, 2 * max(len(e["hits"]) for e in exp))
    det = HipDetector()
    try:
        det.set_option("keep_pyramid", keep)
        det.set_model(m)
        det.plan(H, W, 3, max_batch=5, max_hits=max_hits)
        det.run(torch.from_numpy(np.array(rd.frame_set(H, W, s))).cuda(), 5)
        forms = det.level_forms()
        assert forms["path"] == "fused" and forms["emit_rank"] and forms["emit_f32"] == bool(keep), forms
        for f in range(5):
            rd.compare(det, m, plan, exp[f], f, (name, H, W, s, "keep_pyramid", keep, "frame", f), floats=bool(keep))
        if not keep:
            with pytest.raises(HipError):
                det.read_level(0, 0)
    finally:
        det.close()


@pytest.mark.gpu
@pytest.mark.parametrize("run", rd.EDGE_RUNS, ids=["default", "segments3_warm4"])
@pytest.mark.parametrize("H,W", rd.EDGE_SIZES)
def test_gpu_edge_columns(oracle, H, W, run):
    import torch
    from acf_amd.detector import HipDetector
    plan, frame, e = rd.edge_expected(H, W)
    m = rd.edge_model()
    det = HipDetector()
    try:
        for k, v in run.items():
            det.set_option(k, v)
        det.set_model(m)
        det.plan(H, W, 3, max_batch=1, max_hits=max(1 << 14, 2 * len(e["hits"])))
        det.run(torch.from_numpy(frame[None].copy()).cuda(), 1)
        forms = det.level_forms()
        assert forms["path"] == "fused" and forms["emit_rank"] and forms["emit_f32"], forms
        assert forms["segments"] == (3 if run else 8), forms   # (default: enough segments for 4096 waves, at most 8)
        rd.compare(det, m, plan, e, 0, (H, W, sorted(run.items())), floats=True)
    finally:
        det.close()
