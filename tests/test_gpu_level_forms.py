"""The level stage's plan-time forks (PlanBuild::levelJobs, PyramidRun::planLevels) against the oracle, one case on each side of each
fork (tests/level_forms_case.py): every pyramid level where the call kept floats, every rank level against the ranks of the oracle's
float level (padded border included), hits, scores and mapped boxes, as bits; then, from HipDetector.level_forms() and the profile's
kernel names, that the call took the form the case is named for.  tests/test_level_forms.py holds the CPU side."""
import os
import subprocess
import sys

import pytest

import level_forms_case as lf

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.parametrize("case", [c for c in lf.CASES if "env" not in lf.CASES[c][5]])
def test_level_form_bit_exact(oracle, case):
    lf.run_case(case)


@pytest.mark.parametrize("case", [c for c in lf.CASES if "env" in lf.CASES[c][5]])
def test_environment_selected_level_form_bit_exact(oracle, case):
    """a form only the environment selects: its own process (the environment is read once per process)"""
    env = dict(os.environ, ACF_HIP_FORCE_FALLBACK=lf.CASES[case][5]["env"])
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "level_forms_case.py"), case], cwd=ROOT, env=env, capture_output=True, text=True,
                       timeout=300)
    assert r.returncode == 0 and r.stdout.strip().endswith("ok " + case), (case, r.stdout[-1500:], r.stderr[-3000:])


def test_level_forms_before_the_first_call():
    """the query on a plan that has not run yet reports the plan's fused list and zero call-wide words"""
    lf.forms_before_the_first_call("approx_257")
