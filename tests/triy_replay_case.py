"""The cases of tests/test_gpu_triy_replay.py and the run they share: frames through acf_hip_pyramid with the pyramid kept, the fused
pyramid read back.  Run as a program it is the test's second leg: every case in THIS process — whose environment the caller set, the
form-selecting variable is read once per process — and one JSON line {case id: sha256 of the pyramids' bytes, "forms": ...}."""
import hashlib
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

NF = 3  # frames per case: the frame strides of M, O and the checkpoints

# (H, W): one real scale of exactly this size (and smaller ones below 48 rows or columns, which keep their forms).
# widths: 48 = head and tail reflection in one 64-column block; 64; 68, 76 = the tail's reflected taps reach back across a segment edge
# and across the block edge at column 64; 132 = a block with one live segment; 192 = three whole blocks.
# heights: 48; 52, 56 = (h + 8) % 16 != 0, the last 16-row step partly past h (h - J = 20 and 8 at the tail); 72 (h - J = 8 after three steps)
SHAPES = [(48, 48), (48, 64), (48, 68), (48, 76), (48, 132), (48, 192), (52, 64), (56, 64), (72, 64), (52, 76), (56, 132)]
# pyramids: scale 0 through the smoothing chain's producer (the options force it at these sizes), the next scales through k_tri_x's
PYRAMIDS = [(128, 192), (240, 320)]
CHAIN_OPTIONS = (("fused_grad", 2), ("fused_tri", 2), ("shared_device", 1))


def cases():
    out = []
    for nO in (6, 9):  # both MAXO instantiations of k_triy_chns
        for (H, W) in SHAPES:
            out.append(("s%dx%d_o%d" % (H, W, nO), H, W, nO, ()))
        for (H, W) in PYRAMIDS:
            out.append(("p%dx%d_o%d" % (H, W, nO), H, W, nO, CHAIN_OPTIONS))
    return out


def model_of(nO):
    from acf_amd import synth
    return synth.make_model(seed=5, name="TINY", nTrees=32, nOrients=nO)


def frames_of(H, W):
    from acf_amd import synth
    return np.stack([synth.make_frame(4100 + 7 * i + H + W, H, W, "luv") for i in range(NF)])


def run_case(case):
    """(the NF fused pyramids, the forms convTri took per real scale, kernel names that ran)"""
    import torch
    from acf_amd.detector import HipDetector
    _, H, W, nO, options = case
    det = HipDetector()
    for k, v in options:
        det.set_option(k, v)
    det.set_option("keep_pyramid", 1)
    det.set_option("profile", 1)
    det.set_model(model_of(nO))
    det.plan(H, W, 3, max_batch=NF, max_hits=1 << 12)
    det.pyramid(torch.from_numpy(frames_of(H, W)).cuda(), NF)
    pyr = [det.read_pyramid(f) for f in range(NF)]
    forms = det.tri_forms()
    names = sorted(det.profile())
    det.close()
    return pyr, forms, names


def digest(pyr):
    h = hashlib.sha256()
    for p in pyr:
        h.update(np.ascontiguousarray(p).view(np.uint32).tobytes())
    return h.hexdigest()


def main():
    out = {}
    for case in cases():
        pyr, forms, _ = run_case(case)
        out[case[0]] = dict(sha=digest(pyr), forms=forms)
    print(json.dumps(out))
    return 0


if __name__ == "__main__":
    sys.exit(main())
