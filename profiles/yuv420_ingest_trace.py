"""k_ingest_yuv420 beside k_ingest_u8: the workload for a kernel trace, and the reader of what the trace wrote.

  rocprofv3 --kernel-trace --stats -d OUT/kt -o trace --output-format csv -- python profiles/yuv420_ingest_trace.py [--frames 96] [--reps 8]
  rocprofv3 --pmc SQ_LDS_BANK_CONFLICT SQ_LDS_IDX_ACTIVE -d OUT/pmc -o pmc --output-format csv -- python profiles/yuv420_ingest_trace.py --reps 1
  python profiles/yuv420_ingest_trace.py --summarise OUT

The workload: one context, `frames` frames of 1080p, a model that asks for LUV; acf_hip_pyramid_u8 on packed RGB and on NV12 frames
of the same pictures, alternating, `reps` times each after one warm-up of both.  The two ingest kernels write the same planes
(3 x f32 per pixel) and differ in what they read (3 against 1.5 bytes per pixel) and in the integer conversion.
--summarise prints, per ingest kernel, launches, median / min / max microseconds (the spread of the repeated launches of that one
run) and, where a counter run is there, LDS bank-conflict cycles over LDS-active cycles."""
import argparse
import collections
import csv
import glob
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def workload(args):
    import numpy as np
    import torch
    from acf_amd import capi, synth
    from acf_amd.detector import HipDetector
    from stream_bench import to_nv12
    H, W, B = 1080, 1920, args.frames
    model = synth.make_model(seed=1, name="FACE80", isLuv=0)
    rgb = synth.make_frame(7, H, W, "rgb")
    up = np.ascontiguousarray(np.clip(np.rint(rgb.transpose(2, 1, 0) * 255.0), 0, 255).astype(np.uint8))
    frames = [np.roll(up, (13 * i, 29 * i), axis=(0, 1)) for i in range(8)]
    x_rgb = torch.from_numpy(np.stack([frames[i % 8] for i in range(B)])).cuda()
    x_nv = torch.from_numpy(np.stack([to_nv12(frames[i % 8]) for i in range(B)])).cuda()
    det = HipDetector(model, H, W, 3, max_batch=B, max_hits=8192)
    for _ in range(1 + args.reps):
        det.pyramid_u8(x_rgb, capi.PIX_RGB)
        det.pyramid_u8(x_nv, capi.PIX_NV12)
    det.synchronize()
    det.close()


def find(root, suffix):
    return sorted(glob.glob(os.path.join(root, "**", "*" + suffix), recursive=True))


def summarise(out):
    times = collections.defaultdict(list)
    for path in find(os.path.join(out, "kt"), "kernel_trace.csv"):
        for r in csv.DictReader(open(path)):
            if "k_ingest" in r["Kernel_Name"]:
                times[r["Kernel_Name"].split("(")[0]].append((int(r["End_Timestamp"]) - int(r["Start_Timestamp"])) / 1e3)
    for k, t in sorted(times.items()):
        t = t[1:]  # (the warm-up launch)
        print("%-60s launches %3d  median %8.1f us  min %8.1f  max %8.1f" % (k, len(t), statistics.median(t), min(t), max(t)))
    ctr = collections.defaultdict(lambda: collections.defaultdict(float))
    for path in find(os.path.join(out, "pmc"), "counter_collection.csv"):
        for r in csv.DictReader(open(path)):
            if "k_ingest" in r["Kernel_Name"]:
                ctr[r["Kernel_Name"].split("(")[0]][r["Counter_Name"]] += float(r["Counter_Value"])
    for k, v in sorted(ctr.items()):
        print("%-60s %s" % (k, "  ".join("%s %.4g" % kv for kv in sorted(v.items()))))


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=96)
    ap.add_argument("--reps", type=int, default=8)
    ap.add_argument("--summarise")
    a = ap.parse_args()
    sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
    summarise(a.summarise) if a.summarise else workload(a)
