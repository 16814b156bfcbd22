"""The forks of the real-scale image resample (PlanBuild::imageStrips, stripPlan, PyramidRun::imageResample, launchStrip) against the
oracle, one case on each side of each (tests/scale_forms_case.py): every pyramid level, hit, score and mapped box as bits; then, from
HipDetector.scale_forms(), that every real scale took the route the case names, with the plan the case names.  The closing test holds
the union of what was reported against the forks.  tests/test_scale_forms.py holds the CPU side."""
import os
import subprocess
import sys

import pytest

import scale_forms_case as sf

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
REPORTED = {}


@pytest.mark.parametrize("case", [c for c in sf.CASES if "env" not in sf.CASES[c][5]])
def test_scale_form_bit_exact(oracle, case):
    try:
        REPORTED[case] = [sf.form_token(f) for f in sf.run_case(case)]
    except AssertionError:
        REPORTED[case] = None
        raise


@pytest.mark.parametrize("case", [c for c in sf.CASES if "env" in sf.CASES[c][5]])
def test_environment_selected_scale_form_bit_exact(oracle, case):
    """a route only the environment selects: its own process (the environment is read once per process)"""
    REPORTED[case] = None
    env = dict(os.environ, ACF_HIP_FORCE_FALLBACK=sf.CASES[case][5]["env"])
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "scale_forms_case.py"), case], cwd=ROOT, env=env, capture_output=True, text=True,
                       timeout=300)
    assert r.returncode == 0 and r.stdout.strip().endswith("ok " + case), (case, r.stdout[-1500:], r.stderr[-3000:])
    line = [l for l in r.stdout.splitlines() if l.startswith("forms " + case + " ")][-1]
    REPORTED[case] = line.split()[2:]


def test_reported_forms_cover_every_fork():
    """the union of the words the cases above reported (not of what the table claims): every route, SLOW 0 / 1, nty 1 and >= 2, nSplit 1
    and >= 2, every refusal reason the pipeline reaches"""
    missing = sorted(c for c in sf.CASES if not REPORTED.get(c))
    assert not missing, ("the coverage is that of the cases' own reports: run this file whole, in order and in one process; no report from", missing)
    flat = []
    for toks in REPORTED.values():
        for tok in toks:
            route, plans, nty, nsplit, why, why_pair = tok.split(":")
            route, *flags = route.split("+")
            flat.append(dict(route=route, slow="slow" in flags, nty=int(nty[1:]), n_split=int(nsplit[1:]), why=why, why_pair=why_pair))
    assert {t["route"] for t in flat} == set(sf.ROUTES)
    strips = [t for t in flat if t["route"] in ("strip", "strip_pair_a")]
    assert {t["slow"] for t in strips} == {False, True}
    assert {t["nty"] >= 2 for t in strips} == {False, True} and {t["n_split"] >= 2 for t in strips} == {False, True}
    assert {t[k] for t in flat for k in ("why", "why_pair")} - {"-"} == set(sf.REACHED)
