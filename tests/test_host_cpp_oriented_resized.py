"""acf::HipDetector with setInputOrientation AND setMinObjectWidth (acf_amd/host/HipDetector.cpp: detectYuv, streamOpenYuv), through
the CLI: acf_hip_detect --yuv i420 --orient 1 --min-width 150 on a written frame file prints the boxes of the Python path
(run_yuv_resized(orient=1)) followed by unscale_boxes — in the upright full-size frame — and names the upright and the reduced size.
The two setters together used to throw ACF_HIP_E_UNSUPPORTED."""
import os
import subprocess
import sys

import numpy as np
import pytest

import resized_entry_case as rc
from acf_amd import synth

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.parametrize("mode", [[], ["--stream", "2"]], ids=["detectYuv", "streamOpenYuv"])
def test_cli_orient_and_min_width_match_the_python_path(tmp_path, mode):
    import torch
    import yuv_desc_ref as ydr
    from acf_amd.detector import HipDetector
    from acf_amd.modelio import write_model
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    from test_host_cpp import parse, run
    host = os.path.join(ROOT, "acf_amd", "host")
    subprocess.check_call(["make", "-s", "-C", host])
    H, W, cnt, min_width, code = 242, 320, 5, 150, 1
    model = synth.make_model(**rc.FACE80)
    write_model(str(tmp_path / "m.acfm"), model)
    d, fb = HipDetector.yuv_desc("i420", H, W)
    buf = np.concatenate([ydr.pack("i420", *rc.yuv_planes(60 + i, H, W, 1, 1)) for i in range(cnt)])
    (tmp_path / "f.yuv").write_bytes(buf.tobytes())
    p = run(os.path.join(host, "acf_hip_detect"), ["--model", str(tmp_path / "m.acfm"), "--frames", str(tmp_path / "f.yuv"), "--yuv", "i420",
                                                   "--rows", str(H), "--cols", str(W), "--count", str(cnt), "--min-width", str(min_width),
                                                   "--orient", str(code), "--luv"] + mode)      # (both setters: no longer refused)
    got = parse(p.stdout)
    scale = HipDetector.resize_scale(model["modelDs_w"], min_width)
    dr, dc = HipDetector.oriented_resized_dims(H, W, code, scale)
    frame_lines = [ln for ln in p.stdout.splitlines() if ln.startswith("frame")]
    assert len(frame_lines) == cnt
    assert all(" upright %dx%d orient %d reduced %dx%d" % (W, H, code, dr, dc) in ln for ln in frame_lines), frame_lines[0]
    det = HipDetector(model, dr, dc, 3, max_batch=cnt, max_hits=1 << 16)
    x = torch.from_numpy(buf).cuda()
    det.run_yuv_resized(x, cnt, d, H, W, scale, code)
    total = 0
    for f in range(cnt):
        dd, _ = det.detections(f)
        dd = HipDetector.unscale_boxes(dd, scale)
        py = [(int(r["x"]), int(r["y"]), int(r["w"]), int(r["h"]), int(np.float32(r["score"]).view(np.uint32))) for r in dd]
        assert got[f] == py, f
        total += len(py)
    assert total > 0
    det.close()
