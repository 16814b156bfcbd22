"""acf::HipDetector::cutDetections through the CLI (acf_amd/host/HipDetector.cpp, acf_hip_detect.cpp): acf_hip_detect --yuv i420
--orient 1 --min-width M --cut 32x32:2 writes, for every frame, the PPMs of its first two detections — the bytes of the Python path's
uint8 packed crops (run_yuv_resized(orient=1), then cut_detections with the same scale), which tests/test_gpu_cut_crops.py holds
against the definition."""
import os
import subprocess
import sys

import numpy as np
import pytest

import resized_entry_case as rc
from acf_amd import synth

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_cli_cut_writes_the_python_paths_crops(tmp_path):
    import torch
    import yuv_desc_ref as ydr
    from acf_amd.detector import HipDetector
    from acf_amd.modelio import write_model
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    from test_host_cpp import run
    host = os.path.join(ROOT, "acf_amd", "host")
    subprocess.check_call(["make", "-s", "-C", host])
    H, W, cnt, min_width, code, K, cw, ch = 242, 320, 3, 150, 1, 2, 32, 32
    model = synth.make_model(**rc.FACE80)
    write_model(str(tmp_path / "m.acfm"), model)
    d, fb = HipDetector.yuv_desc("i420", H, W)
    buf = np.concatenate([ydr.pack("i420", *rc.yuv_planes(60 + i, H, W, 1, 1)) for i in range(cnt)])
    (tmp_path / "f.yuv").write_bytes(buf.tobytes())
    prefix = str(tmp_path / "c")
    p = run(os.path.join(host, "acf_hip_detect"), ["--model", str(tmp_path / "m.acfm"), "--frames", str(tmp_path / "f.yuv"), "--yuv", "i420", "--rows", str(H),
                                                   "--cols", str(W), "--count", str(cnt), "--min-width", str(min_width), "--orient", str(code), "--luv",
                                                   "--cut", "%dx%d:%d" % (cw, ch, K), "--cut-prefix", prefix])
    said = {int(ln.split()[1]): int(ln.split()[2]) for ln in p.stdout.splitlines() if ln.startswith("crops ")}
    scale = HipDetector.resize_scale(model["modelDs_w"], min_width)
    dr, dc = HipDetector.oriented_resized_dims(H, W, code, scale)
    det = HipDetector(model, dr, dc, 3, max_batch=cnt, max_hits=1 << 16)
    x = torch.from_numpy(buf).cuda()
    det.run_yuv_resized(x, cnt, d, H, W, scale, code)
    crops, boxes, counts = det.cut_detections(det.crop_source_yuv(x, cnt, d, None, H, W, code), (ch, cw), K, det_scale=scale, dtype=torch.uint8, layout="packed")
    det.synchronize()
    crops, counts = crops.cpu().numpy(), counts.cpu().numpy()
    assert said == {f: int(counts[f]) for f in range(cnt)} and counts.sum() > 0, (said, counts)
    head = b"P6\n%d %d\n255\n" % (cw, ch)
    for f in range(cnt):
        for i in range(K):
            path = "%s_%d_%d.ppm" % (prefix, f, i)
            if i >= counts[f]:
                assert not os.path.exists(path), path
                continue
            assert open(path, "rb").read() == head + crops[f, i].tobytes(), path
    det.close()
