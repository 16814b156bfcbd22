"""Crops/s of acf_hip_evaluate_crops_u8 (profiles/crop_scores.md): 4096 FACE80 80 x 80 RGB crops, 2048 trees, early-stop leaves, cascThr 0.
  python profiles/crop_scores.py                 the fused form (k_crop_score), the per-crop route it replaces, kernel times
  ACF_HIP_LIB=acf_amd/libacf_hip_staged.so python profiles/crop_scores.py     the staged form on the same batch
     (profiles/build_variant.sh staged -DACF_CROPS_FORCE_STAGED)
One process; warm-up, then medians with the spread of the repetitions."""
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402

from acf_amd import capi, synth  # noqa: E402
from acf_amd.detector import HipDetector  # noqa: E402

N, H, W, REPS, WARM = 4096, 80, 80, 15, 3


def main():
    m = synth.make_model(seed=3, nTrees=2048, name="FACE80")
    m["hs"] = (-0.05 + 0.35 * synth.uniform(6, m["hs"].size)).astype(np.float32).reshape(m["hs"].shape)
    # 4096 different crops: 64 synthetic frames' pixels, each cut 64 ways
    base = np.stack([np.moveaxis(synth.make_frame(100 + k, 2 * H, 2 * W, "rgb"), 0, 2).transpose(1, 0, 2) for k in range(64)])   # [64][2H][2W][3]
    imgs = np.stack([base[k][8 * i:8 * i + H, 8 * j:8 * j + W] for k in range(64) for i in range(8) for j in range(8)])
    imgs = np.ascontiguousarray(np.rint(imgs * 255.0).astype(np.uint8))
    dev = HipDetector()
    dev.set_model(m)
    dev.set_option("profile", 1)
    t = torch.from_numpy(imgs).cuda()
    out = torch.empty(N, dtype=torch.float32, device="cuda")
    import ctypes as C

    def call():
        rc = dev.lib.acf_hip_evaluate_crops_u8(dev.ctx, None, C.c_void_p(t.data_ptr()), N, H, W, capi.PIX_RGB, 0, 0.0, C.c_void_p(out.data_ptr()))
        assert rc == 0, dev.lib.acf_hip_last_error(dev.ctx)
        dev.synchronize()

    for _ in range(WARM):
        call()
    dev.profile()
    wall = []
    for _ in range(REPS):
        t0 = time.perf_counter()
        call()
        wall.append(time.perf_counter() - t0)
    prof = dev.profile()
    wall = np.array(wall)
    res = {"lib": os.path.basename(capi.LIB_PATH), "crops": N, "wall_ms_median": float(np.median(wall) * 1e3), "wall_ms_min": float(wall.min() * 1e3),
           "wall_ms_max": float(wall.max() * 1e3), "crops_per_s_median": float(N / np.median(wall)),
           "kernel_ms_per_call": {k: v[0] / REPS for k, v in prof.items()}}
    scores = out.cpu().numpy()
    res["early_stops"] = int((scores <= 0).sum())
    # the only route before these entries: chns_compute + op_evaluate per crop, host planes in, over 64 crops
    from oracle import binding as ob
    planes = [np.array(ob.ingest_u8(imgs[i], capi.PIX_RGB)) for i in range(64)]
    for _ in range(2):
        old = np.array([dev.op_evaluate(dev.chns_compute(p), 0.0) for p in planes[:8]], np.float32)
    per = []
    for _ in range(5):
        t0 = time.perf_counter()
        old = np.array([dev.op_evaluate(dev.chns_compute(p), 0.0) for p in planes], np.float32)
        per.append((time.perf_counter() - t0) / 64)
    per = np.array(per)
    res["per_crop_route_crops_per_s_median"] = float(1.0 / np.median(per))
    res["per_crop_route_us_min_max"] = [float(per.min() * 1e6), float(per.max() * 1e6)]
    res["same_bits_as_per_crop_route"] = bool(np.array_equal(old.view(np.uint32), scores[:64].view(np.uint32)))
    print(json.dumps(res))
    dev.close()


if __name__ == "__main__":
    main()
