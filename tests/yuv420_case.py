"""One process per setting (ACF_HIP_FORCE_FALLBACK is read once per process): two NV12 frames of 130 x 174 (three tiles each way,
ragged edges) through run_u8 with option "profile" on, against the oracle on the restated RGB bytes.  Prints
"ok <detections> <digest of pyramids and detections> <kernel names the profile saw>"; tests/test_gpu_yuv420.py runs this file with
the defaults (k_ingest_yuv420) and with the fallback yuv_unfused (k_yuv420_to_rgb8 + k_ingest_u8) and holds the two together."""
import hashlib
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, HERE)
import yuv420_ref as yr  # noqa: E402
from acf_amd import capi, synth  # noqa: E402
from acf_amd.detector import HipDetector  # noqa: E402
from oracle import binding as ob  # noqa: E402
from test_gpu_yuv420 import make_nv, oracle_expect  # noqa: E402


def main():
    H, W, nF = 130, 174, 2
    model = synth.make_model(seed=3, name="INRIA", nTrees=64, cascThr=-3.0, nOctUp=0)
    frames = [make_nv(40 + f, H, W) for f in range(nF)]
    det = HipDetector(model, H, W, 3, max_batch=nF, max_hits=1 << 16)
    det.set_option("profile", 1)
    det.run_u8(torch.from_numpy(np.stack(frames)).cuda(), capi.PIX_NV12)
    kernels = sorted(det.profile())
    h = hashlib.sha256()
    total = 0
    for f, (plan, pyr, want, want_hits) in enumerate(oracle_expect(ob, model, [yr.nv_to_rgb(fr, H, W) for fr in frames], H, W)):
        got_pyr = det.read_pyramid(f)
        got, got_hits = det.detections(f)
        if not np.array_equal(got_pyr.view(np.uint32), pyr.view(np.uint32)):
            print("pyramid differs, frame", f)
            return 1
        if got.tobytes() != want.tobytes() or got_hits.tobytes() != want_hits.tobytes():
            print("detections differ, frame", f, len(got), len(want))
            return 1
        h.update(got_pyr.tobytes())
        h.update(got.tobytes())
        total += len(want)
    det.close()
    if total == 0:
        print("no detections: the case checks nothing")
        return 1
    print("ok", total, h.hexdigest()[:16], ",".join(kernels))
    return 0


if __name__ == "__main__":
    sys.exit(main())
