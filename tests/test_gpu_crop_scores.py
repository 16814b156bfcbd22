"""Detector::evaluate(const cv::Mat&) for batches of crops on the device: acf_hip_evaluate_crops / _u8 (k_crop_score, or the staged
form ending in k_evaluate_windows) against the oracle — oracle.chns_compute, then acfo_evaluate — bit for bit, no tolerance.
tests/test_crop_scores.py holds the preconditions (16 distinct full-pass scores; both outcomes with the early-stop leaves)."""
import ctypes as C

import numpy as np
import pytest

import crop_scores_case as cs
from acf_amd import capi, synth

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def dev():
    from acf_amd.detector import HipDetector
    d = HipDetector()
    d.set_option("profile", 1)
    yield d
    d.close()


def both_regimes(oracle, dev, kw, batch, chns=None, check_outcomes=False):
    """the full pass (stock leaves, cascThr -1e30) and the early stop (its leaves, cascThr 0) of one model on one batch"""
    for early, thr in ((False, cs.FULL), (True, 0.0)):
        m = cs.model(early=early, **kw)
        dev.set_model(m)
        want = cs.oracle_scores(oracle, m, chns or m, batch, thr)
        got = dev.evaluate_crops(batch, chns, thr)
        assert got.dtype == np.float32 and got.shape == (len(batch),)
        assert np.array_equal(cs.bits(got), cs.bits(want)), (early, got, want)
    return dev.profile()


@pytest.mark.parametrize("case", cs.BASE + cs.VARIANTS + cs.EARLY[4:], ids=lambda c: c[0])
def test_scores_equal_the_oracle(oracle, dev, case):
    _, kw, H, W, kind, d = case
    both_regimes(oracle, dev, kw, cs.crops(H, W, kind))


@pytest.mark.parametrize("n", [1, 3, 65, 300])
def test_batch_sizes(oracle, dev, n):
    """300 crops are more than the device has CUs: k_crop_score's workgroups take a second crop.  Early-stop leaves: the batch mixes
    crops that stop with crops that pass."""
    kw = dict(name="TINY", isLuv=1)
    batch = cs.crops(16, 16, "luv", n=n)
    both_regimes(oracle, dev, kw, batch)
    if n >= 16:
        m = cs.model(early=True, **kw)
        stopped = cs.stopped_early(oracle, m, m, batch)
        assert stopped.any() and (~stopped).any()


def test_both_forms_by_crop_size(oracle, dev):
    kw = dict(name="FACE80")
    dev.profile()
    prof = both_regimes(oracle, dev, kw, cs.crops(80, 80, "rgb"))
    assert "k_crop_score" in prof and "k_evaluate_windows" not in prof, prof
    prof = both_regimes(oracle, dev, kw, cs.crops(160, 160, "rgb", n=4))
    assert "k_evaluate_windows" in prof and "k_crop_score" not in prof, prof


def test_staged_form_in_chunks_and_other_shapes(oracle, dev):
    """the staged form where its planes are not multiples of anything: 163 x 161 (cropped to 160 x 160), gray 1-plane 200 x 168"""
    both_regimes(oracle, dev, dict(name="FACE80"), cs.crops(163, 161, "rgb", n=3))
    prof = both_regimes(oracle, dev, dict(name="FACE64"), cs.crops(200, 168, "gray", n=3))
    assert "k_evaluate_windows" in prof


def test_identity_with_chns_compute_and_op_evaluate(dev):
    batch = cs.crops(80, 80, "rgb", n=8)
    for early, thr in ((False, cs.FULL), (True, 0.0)):
        dev.set_model(cs.model(early=early, name="FACE80"))
        got = dev.evaluate_crops(batch, None, thr)
        want = np.array([dev.op_evaluate(dev.chns_compute(c), thr) for c in batch], np.float32)
        assert np.array_equal(cs.bits(got), cs.bits(want))


def rand_bytes(seed, shape):
    return (synth.splitmix64(seed, int(np.prod(shape))) >> np.uint64(56)).astype(np.uint8).reshape(shape)


U8 = [("rgb_tight", dict(name="FACE80", isLuv=0), capi.PIX_RGB, 80, 80, 0), ("bgra_padded", dict(name="FACE80", isLuv=0), capi.PIX_BGRA, 80, 80, 3),
      ("gray_face64", dict(name="FACE64"), capi.PIX_GRAY, 64, 64, 0), ("rgb_staged_odd", dict(name="INRIA"), capi.PIX_RGB, 181, 131, 0)]


@pytest.mark.parametrize("case", U8, ids=lambda c: c[0])
def test_u8_entry(oracle, dev, case):
    """padded: rows of (w + 3) pixels, i.e. a stride of w * 4 + 12 bytes; the oracle ingests the whole rows and the planes are cut"""
    _, kw, pix, H, W, pad = case
    cpp = capi.PIX_CPP[pix]
    n = 6
    imgs = rand_bytes(77, (n, H, W + pad, cpp) if cpp > 1 else (n, H, W))
    # smooth the noise a little so that the walks do not all end alike: average each byte with its right neighbour
    imgs = ((imgs.astype(np.uint16) + np.roll(imgs, 1, axis=2)) // 2).astype(np.uint8)
    planes = np.stack([oracle.ingest_u8(im, pix)[:, :W, :] for im in imgs])
    for early, thr in ((False, cs.FULL), (True, 0.0)):
        m = cs.model(early=early, **kw)
        dev.set_model(m)
        stride = (W + pad) * cpp if pad else 0
        got = dev.evaluate_crops_u8(imgs.reshape(n, -1) if pad else imgs, pix, row_stride=stride, cascThr=thr, h=H, w=W)
        assert np.array_equal(cs.bits(got), cs.bits(dev.evaluate_crops(planes, None, thr)))
        assert np.array_equal(cs.bits(got), cs.bits(cs.oracle_scores(oracle, m, m, planes, thr)))


def test_explicit_channel_options(oracle, dev):
    """FACE80 scored on the toolbox defaults' channels (what Detector::evaluate(const cv::Mat&) computes), not its own"""
    dfl = synth.make_model(seed=3, name="TINY", nTrees=16, isLuv=0)
    batch = cs.crops(80, 80, "rgb")
    both_regimes(oracle, dev, dict(name="FACE80"), batch, chns=dfl)
    m = cs.model(name="FACE80")
    dev.set_model(m)
    a, b = dev.evaluate_crops(batch, dfl, cs.FULL), dev.evaluate_crops(batch, None, cs.FULL)
    assert not (cs.bits(a) == cs.bits(b)).any()


@pytest.mark.parametrize("shape", [(128, 64), (160, 80)], ids=["fused", "staged"])
def test_reference_arithmetic(oracle, shape):
    from acf_amd.detector import HipDetector
    H, W = shape
    m = cs.model(name="INRIA")
    batch = cs.crops(H, W, "rgb", n=8)
    oracle.set_x86_tables(*oracle.x86_fixture())
    oracle.set_approx(3)
    try:
        want = cs.oracle_scores(oracle, m, m, batch, cs.FULL)
    finally:
        oracle.set_approx(0)
    d = HipDetector()
    try:
        d.set_x86_tables(*oracle.x86_fixture())
        d.set_option("arith", 1)
        d.set_option("profile", 1)
        d.set_model(m)
        got = d.evaluate_crops(batch, None, cs.FULL)
        assert ("k_crop_score" if shape == (128, 64) else "k_evaluate_windows") in d.profile()
    finally:
        d.close()
    assert np.array_equal(cs.bits(got), cs.bits(want))
    if shape == (128, 64):   # (on the eight 160 x 80 crops the two tiers' channels differ, but no tree's decision does)
        assert not np.array_equal(cs.bits(got), cs.bits(cs.oracle_scores(oracle, m, m, batch, cs.FULL)))


def test_refusals_leave_the_context_usable(oracle):
    import torch
    from acf_amd.detector import HipDetector, HipError
    d = HipDetector()
    batch = cs.crops(80, 80, "rgb", n=2)
    t = torch.from_numpy(np.array(batch)).cuda()
    out = torch.empty(2, dtype=torch.float32, device="cuda")
    u8 = torch.zeros(2 * 80 * 80 * 3, dtype=torch.uint8, device="cuda")

    def call(n=2, h=80, w=80, dd=3, chns=None, crops=t, scores=out):
        pp = C.byref(capi.make_params(chns)[0]) if chns is not None else None
        return d.lib.acf_hip_evaluate_crops(d.ctx, pp, C.c_void_p(crops.data_ptr() if crops is not None else 0), n, h, w, dd, 0.0,
                                            C.c_void_p(scores.data_ptr() if scores is not None else 0))

    def call_u8(pix, stride=0):
        return d.lib.acf_hip_evaluate_crops_u8(d.ctx, None, C.c_void_p(u8.data_ptr()), 2, 80, 80, pix, stride, 0.0, C.c_void_p(out.data_ptr()))

    try:
        assert call() == capi.E_NOMODEL and d.lib.acf_hip_last_error(d.ctx)
        m = cs.model(name="FACE80")
        d.set_model(m)
        assert call(crops=None) == capi.E_INVALID and call(scores=None) == capi.E_INVALID
        assert call(n=0) == capi.E_INVALID and call(dd=2) == capi.E_INVALID and call(dd=5) == capi.E_INVALID
        assert call(h=79) == capi.E_INVALID and call(w=76) == capi.E_INVALID              # cropped to 76: smaller than modelDsPad
        assert d.lib.acf_hip_last_error(d.ctx)
        assert call(chns=dict(m, colorEnabled=0)) == capi.E_INVALID                        # 7 channels x 400 cells < the model's fids
        assert call(chns=dict(m, softBin=1)) == capi.E_UNSUPPORTED                          # as acf_hip_chns_compute
        assert call(chns=dict(m, colorSmooth=2.0)) == capi.E_UNSUPPORTED
        assert call(chns=dict(m, colorSpace=capi.CS_HSV)) == capi.E_INVALID                # isLuv with hsv
        assert call_u8(capi.PIX_NV12) == capi.E_INVALID and call_u8(capi.PIX_NV21) == capi.E_INVALID and call_u8(17) == capi.E_INVALID
        assert call_u8(capi.PIX_RGB, stride=100) == capi.E_INVALID                          # a stride smaller than a row
        assert call_u8(capi.PIX_GRAY) == capi.E_INVALID                                     # one plane against colorSpace luv
        ldcf = synth.make_model(seed=3, nTrees=16, name="FACE80", ldcfK=2)
        d.set_model(ldcf)
        assert call() == capi.E_UNSUPPORTED
        # ... and a correct call afterwards succeeds
        d.set_model(m)
        got = d.evaluate_crops(batch, None, cs.FULL)
        assert np.array_equal(cs.bits(got), cs.bits(cs.oracle_scores(oracle, m, m, batch, cs.FULL)))
    finally:
        d.close()


# ------------------------------------------------------------------ C++ host (CLI)

@pytest.fixture(scope="module")
def cli():
    import os
    import subprocess
    host = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "acf_amd", "host")
    subprocess.check_call(["make", "-s", "-C", host])
    return os.path.join(host, "acf_hip_detect")


def run_cli(cli, tmp_path, m, batch, extra):
    import os
    import subprocess
    from acf_amd.modelio import write_model
    n, d, W, H = batch.shape
    write_model(str(tmp_path / "m.acfm"), m)
    (tmp_path / "f.raw").write_bytes(np.ascontiguousarray(batch).tobytes())
    e = dict(os.environ)
    e["ACF_HIP_LIBRARY"] = capi.LIB_PATH
    p = subprocess.run([cli, "--model", str(tmp_path / "m.acfm"), "--frames", str(tmp_path / "f.raw"), "--rows", str(W), "--cols", str(H),
                        "--channels", str(d), "--count", str(n)] + extra, env=e, stdout=subprocess.PIPE, stderr=subprocess.PIPE,
                       universal_newlines=True, timeout=120)
    assert p.returncode == 0, p.stderr
    return p.stdout.splitlines()


@pytest.mark.parametrize("defaults", [False, True])
def test_cli_score_crops(cli, oracle, tmp_path, defaults):
    """acf_hip_detect --score-crops: acf::HipDetector::evaluateCrops with the model's channel options, or (--defaults) the batch form of
    evaluate(image) with the toolbox defaults; cascThr 0 either way."""
    # (INRIA's stock channel options are the toolbox defaults: four orientations make the model's own differ from them)
    m = cs.model(early=True, name="INRIA", nOrients=4)
    batch = cs.crops(128, 64, "rgb", n=3)
    lines = run_cli(cli, tmp_path, m, batch, ["--score-crops"] + (["--defaults"] if defaults else []))
    got = np.array([int(l.split()[3], 16) for l in lines if l.startswith("crop ")], np.uint32)
    dfl = synth.make_model(seed=3, name="TINY", nTrees=16, isLuv=0)
    assert np.array_equal(got, cs.bits(cs.oracle_scores(oracle, m, dfl if defaults else m, batch, 0.0)))
    assert not np.array_equal(got, cs.bits(cs.oracle_scores(oracle, m, m if defaults else dfl, batch, 0.0)))


def test_cli_scores_a_window_sized_image_instead_of_searching(cli, oracle, tmp_path):
    """acf.cpp:350-355: acf::HipDetector::evaluate(image) — one box, the whole image, with the toolbox-default channels' score"""
    m = cs.model(early=True, name="FACE80")
    batch = cs.crops(80, 80, "rgb", n=3)
    lines = run_cli(cli, tmp_path, m, batch, [])
    dfl = synth.make_model(seed=3, name="TINY", nTrees=16, isLuv=0)
    want = cs.bits(cs.oracle_scores(oracle, m, dfl, batch, 0.0))
    assert [l for l in lines if l.startswith("frame ")] == ["frame %d 1" % f for f in range(3)]
    boxes = [l.split() for l in lines if not l.startswith("frame ")]
    assert [b[:4] for b in boxes] == [["0", "0", "80", "80"]] * 3
    assert np.array_equal(np.array([int(b[5], 16) for b in boxes], np.uint32), want)
