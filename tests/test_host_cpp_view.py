"""acf::HipDetector::detectViews through the CLI (acf_amd/host/HipDetector.cpp, acf_hip_detect.cpp): acf_hip_detect --yuv nv12 --view
x,y,w,h,deg --view ... searches two views of one stored frame in one batch and prints every detection as its quad in the upright stored
frame — the detections of the Python path (run_view on the same bytes, which tests/test_gpu_view.py holds against the definition)
through view_quad."""
import math
import os
import sys

import numpy as np
import pytest

import resized_entry_case as rc
import view_ref as vr
from acf_amd import synth

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_cli_views_print_the_python_paths_quads(tmp_path):
    import torch
    import yuv_desc_ref as ydr
    from acf_amd.detector import HipDetector
    from acf_amd.modelio import write_model
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    from test_host_cpp import CLI, HOST, run
    import subprocess
    subprocess.check_call(["make", "-s", "-C", HOST])
    Hs, Ws, cnt, h, w, smp = 150, 170, 2, vr.H, vr.W, 2
    model = vr.model()
    write_model(str(tmp_path / "m.acfm"), model)
    d, fb = HipDetector.yuv_desc("nv12", Hs, Ws)
    buf = np.concatenate([ydr.pack("nv12", *rc.yuv_planes(80 + i, Hs, Ws, 1, 1)) for i in range(cnt)])
    (tmp_path / "f.yuv").write_bytes(buf.tobytes())
    specs = [((10, 10, 150, 112.5), 20.0, 0), ((30, 20, 110, 82.5), -35.0, 1)]
    args = ["--model", str(tmp_path / "m.acfm"), "--frames", str(tmp_path / "f.yuv"), "--yuv", "nv12", "--rows", str(Hs), "--cols", str(Ws), "--count", str(cnt), "--luv",
            "--view-size", "%dx%d" % (h, w), "--view-samples", str(smp)]
    for box, deg, frame in specs:
        args += ["--view", "%g,%g,%g,%g,%g,%d" % (box + (deg, frame))]
    p = run(CLI, args)
    said, cur = [], None
    for ln in p.stdout.splitlines():
        t = ln.split()
        if t[0] == "view":
            cur = []
            said.append((int(t[1]), int(t[2]), cur))
        else:
            cur.append(([float(v) for v in t[:8]], int(t[9], 16)))
    assert [s[0] for s in said] == [0, 1] and all(s[1] == len(s[2]) for s in said)
    # the Python path on the same bytes
    det = HipDetector(model, h, w, 3, max_batch=2, max_hits=1 << 16)
    x = torch.from_numpy(buf).cuda()
    views = np.stack([HipDetector.view_from_box(box, deg * 3.14159265358979323846 / 180.0, h, w) for box, deg, _ in specs])
    det.run_view(det.crop_source_yuv(x, cnt, d, None, Hs, Ws, 0), views, np.array([s[2] for s in specs], np.int32), smp)
    det.synchronize()
    total = 0
    for i in range(2):
        dets, _ = det.detections(i)
        assert said[i][1] == len(dets), (i, said[i][1], len(dets))
        for k in range(len(dets)):
            q = HipDetector.view_quad(views[i], [int(dets[n][k]) for n in ("x", "y", "w", "h")]).ravel()
            got, score_bits = said[i][2][k]
            assert np.array_equal(np.array(got, np.float32), q), (i, k, got, q)               # %.9g round-trips a float32
            assert score_bits == int(dets["score"][k:k + 1].view(np.uint32)[0]), (i, k)
        total += len(dets)
    assert total > 0
    det.close()
