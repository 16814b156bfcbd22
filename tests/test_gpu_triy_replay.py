"""convTri's x pass as checkpoints replayed in the y kernel (k_tri_x5v<true, true> / k_smooth_grad_tri<.., CK> -> k_triy_chns<.., CK>;
host_plan.h triCkIndex) against the oracle's pyramid, every channel cell of every level bit for bit, through the public API with the
pyramid kept — at the smallest shapes where the segment, block and tail logic can go wrong (tests/triy_replay_case.py lists them and why),
three frames each, nOrients 6 and 9.  Second leg: the same frames under ACF_HIP_FORCE_FALLBACK=triy_stored_u (today's blocked plane U)
in ONE fresh child process for all cases — the variable is read once per process — must give the same bytes.  The form itself is
asserted: the checkpoint form ran at every real scale of >= 48 rows and columns and no plane U is held there; under the fallback
it did not run and the plane is held."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import triy_replay_case as tc

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CASES = tc.cases()


@pytest.fixture(scope="module")
def stored_u():
    """{case id: {sha, forms}} of every case under the stored-U form, from one child process"""
    env = dict(os.environ)
    env["ACF_HIP_FORCE_FALLBACK"] = "triy_stored_u"
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "triy_replay_case.py")], cwd=ROOT, env=env, capture_output=True, text=True,
                       timeout=600)
    assert r.returncode == 0, (r.stdout[-1500:], r.stderr[-1500:])
    return json.loads(r.stdout.strip().splitlines()[-1])


@pytest.mark.parametrize("case", CASES, ids=[c[0] for c in CASES])
def test_replayed_x_pass_matches_the_oracle_and_the_stored_plane(case, oracle, stored_u):
    cid, H, W, nO, options = case
    pyr, forms, names = tc.run_case(case)
    plan = oracle.Plan(tc.model_of(nO), H, W, 3)
    frames = tc.frames_of(H, W)
    for f in range(tc.NF):
        want, _, _ = oracle.chns_pyramid(plan, frames[f])
        assert pyr[f].shape == want.shape
        bad = np.flatnonzero(pyr[f].view(np.uint32) != want.view(np.uint32))
        assert bad.size == 0, (cid, f, bad.size, bad[:8])
    # the form: scale 0 (H x W >= 48 x 48, multiples of 4) replayed checkpoints and holds no U; every scale either did or holds U
    assert forms[0] == 1, (cid, forms)
    assert all(v in (1, 2) for v in forms), (cid, forms)
    assert "k_triy_chns" in names, (cid, names)
    if not options:
        assert "k_tri_x" in names, (cid, names)
    else:
        assert "k_smooth_grad_tri" in names, (cid, names)  # the chain's producer at scale 0
        if min(H, W) // 2 >= 48:
            assert "k_tri_x" in names and forms[1] == 1, (cid, names, forms)  # k_tri_x's producer at scale 1
    # the stored-U leg: the same bytes, through the other form
    assert stored_u[cid]["sha"] == tc.digest(pyr), cid
    assert all(v == 2 for v in stored_u[cid]["forms"]), (cid, stored_u[cid]["forms"])
