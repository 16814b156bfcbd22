"""The C++ host side of the bank (acf::HipDetector::setBank / joinBank, acf_hip_detect --also ... [--join OVR[:separate]]): the CLI, which
goes through both methods, prints the lines the Python path gives for the pipeline case of tests/bank_ref.py — per frame the true count,
then model, box, score bits of every joined detection in order —, and refuses what it cannot do instead of ignoring it."""
import os
import sys

import numpy as np
import pytest

import bank_ref as br
from acf_amd import capi
from acf_amd.detector import HipDetector
from acf_amd.modelio import write_model

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from test_host_cpp import cli, run  # noqa: E402,F401  (cli: the fixture that builds the host side)

MEMBERS = (1, 3, 2)                                                                           # tall, deep, walk: in this order behind the primary


def _args(tmp_path, extra):
    m = br.models()
    write_model(str(tmp_path / "m0.acfm"), m[0])
    a = ["--model", str(tmp_path / "m0.acfm"), "--frames", str(tmp_path / "f.raw"), "--rows", str(br.W), "--cols", str(br.H), "--channels", "3", "--count", "2", "--luv"]
    for i in MEMBERS:
        write_model(str(tmp_path / ("m%d.acfm" % i)), m[i])
        a += ["--also", str(tmp_path / ("m%d.acfm" % i))]
    (tmp_path / "f.raw").write_bytes(br.frames().tobytes())
    return a + extra


def _said(out):
    frames, cur = [], None
    for ln in out.splitlines():
        t = ln.split()
        if t[0] == "frame":
            cur = []
            frames.append((int(t[1]), int(t[2]), cur))
        else:
            cur.append((int(t[0]), int(t[1]), int(t[2]), int(t[3]), int(t[4]), int(t[6], 16)))
    return frames


@pytest.mark.gpu
@pytest.mark.parametrize("join", [None, "0.5", "0.5:separate"])
def test_cli_bank_prints_the_python_paths_lines(cli, tmp_path, join):
    import torch
    p = run(cli, _args(tmp_path, ["--batch"] + (["--join", join] if join else [])))
    said = _said(p.stdout)
    m = br.models()
    det = HipDetector(m[0])
    det.set_bank([m[i] for i in MEMBERS])
    det.plan(br.H, br.W, br.D, max_batch=2, max_hits=1 << 16)
    det.run(torch.from_numpy(br.frames()).cuda())
    det.detect_bank()
    q = None if join is None else capi.make_nms("maxg", overlap=0.5, ovrDnm="union")
    rec, cnt, _, _ = det.join_bank(q, join is not None and join.endswith("separate"), capi.NMS_CAP)
    det.synchronize()
    rec, cnt = rec.cpu().numpy().view(capi.BANK_DTYPE).reshape(2, capi.NMS_CAP), cnt.cpu().numpy()
    det.close()
    assert [s[0] for s in said] == [0, 1]
    raw = [sum(br.RAW_COUNTS[i][f] for i in (0,) + MEMBERS) for f in range(2)]
    for f in range(2):
        n = int(cnt[f])
        assert said[f][1] == n == len(said[f][2]) and (n == raw[f] if join is None else 0 < n < raw[f]), (f, said[f][1], n, raw[f])
        want = [(int(r["model"]), int(r["x"]), int(r["y"]), int(r["w"]), int(r["h"]), int(r["score"].view(np.uint32))) for r in rec[f, :n]]
        assert said[f][2] == want
        assert {w[0] for w in want} == {0, 1, 2, 3}                                           # every model contributes


@pytest.mark.gpu
def test_cli_says_what_it_cannot_do(cli, tmp_path):
    a = _args(tmp_path, [])
    bad = run(cli, a, ok=False)                                                               # --also without --batch
    assert bad.returncode != 0 and "--batch" in bad.stderr and not bad.stdout.strip()
    no_also = [x for i, x in enumerate(a) if x != "--also" and a[i - 1] != "--also"]
    bad = run(cli, no_also + ["--batch", "--join", "0.5"], ok=False)                          # --join without an --also
    assert bad.returncode != 0 and "--also" in bad.stderr and not bad.stdout.strip()
    bad = run(cli, a + ["--batch", "--join", "0.5:apart"], ok=False)
    assert bad.returncode != 0 and "OVR:separate" in bad.stderr
    # a member with another pyramid: setBank's refusal names the member and the field
    other = dict(br.models()[1], nPerOct=4)
    write_model(str(tmp_path / "m1.acfm"), other)
    bad = run(cli, a + ["--batch"], ok=False)
    assert bad.returncode != 0 and "member 0" in bad.stderr and "nPerOct" in bad.stderr
