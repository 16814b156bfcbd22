"""k_resample_strip's two-output form (acf_hip_op_im_resample_pair: stripPlan with both descriptors, launchStrip with descB >= 0)
against two acfo_resample calls, bit for bit, at the shapes of tests/resample_pair_case.py; the returned word must say that the
pair was launched with the tiling the case names, or name the refusal — then each output ran alone and must match as well."""
import numpy as np
import pytest

from acf_amd import synth

import resample_pair_case as rp

pytestmark = pytest.mark.gpu


def bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


@pytest.fixture(scope="module")
def dev():
    from acf_amd.detector import HipDetector
    d = HipDetector()
    yield d
    d.close()


@pytest.mark.parametrize("case", list(rp.CASES))
@pytest.mark.parametrize("nrm", rp.NRMS)
def test_pair_bit_exact(dev, oracle, case, nrm):
    ha, wa, hbA, wbA, hbB, wbB, d, _, word = rp.CASES[case]
    a = (synth.uniform(ha * 7 + wbA, d * wa * ha, 3)).astype(np.float32).reshape(d, wa, ha)
    gotA, gotB, got = dev.op_im_resample_pair(a, hbA, wbA, hbB, wbB, nrm)
    print(case, got)
    errs = []
    for name, g, hb, wb in (("A", gotA, hbA, wbA), ("B", gotB, hbB, wbB)):
        want = np.zeros_like(g)
        assert oracle.lib().acfo_resample(oracle.F(a), oracle.F(want), ha, hb, wa, wb, d, np.float32(nrm)) == 0
        if not np.array_equal(bits(g), bits(want)):
            bad = np.argwhere(bits(g) != bits(want))
            errs.append((name, len(bad), "first [plane, column, row]", bad[0].tolist()))
    if got != word:
        errs.append(("word", got, word))
    assert not errs, (case, errs)
