"""Writes tests/golden/yuv420_rgb.npz: a few small NV12 / NV21 frames and the R, G, B bytes tests/yuv420_ref.py gives for them, frozen,
so that the CPU suite and the GPU box check the same bytes (tests/test_yuv420.py, tests/test_gpu_yuv420.py).

    python tests/golden/make_yuv420.py
"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
import yuv420_ref as yr  # noqa: E402

# name: rows, cols, nv21, row stride, chroma offset (0 = tight)
CASES = {
    "nv12_2x2": (2, 2, False, 0, 0),
    "nv12_16x24": (16, 24, False, 0, 0),
    "nv21_16x24": (16, 24, True, 0, 0),
    "nv12_10x14_stride19_off203": (10, 14, False, 19, 203),   # odd stride, chroma off the dword grid
    "nv21_66x70_stride72_off4800": (66, 70, True, 72, 4800),  # two tiles each way, padded luma plane
}


def main():
    out = {}
    for i, (name, (rows, cols, nv21, stride, off)) in enumerate(sorted(CASES.items())):
        buf = yr.random_frame(1000 + i, rows, cols, nv21, stride, off)
        out[name + "/frame"] = buf
        out[name + "/geom"] = np.array([rows, cols, int(nv21), stride, off], np.int32)
        out[name + "/rgb"] = yr.nv_to_rgb(buf, rows, cols, nv21, stride, off)
    np.savez_compressed(os.path.join(HERE, "yuv420_rgb.npz"), **out)


if __name__ == "__main__":
    main()
