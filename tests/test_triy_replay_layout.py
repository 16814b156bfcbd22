"""The checkpoint buffer of convTri's replayed x pass (acf_amd/csrc/host_plan.h triCkIndex / triCkFloats, through
acf_hip_tri_ck_layout) without a GPU, at the widths and heights tests/test_gpu_triy_replay.py runs: the index is the documented
[x >> 6][(y + 8) >> 4][(x >> 4) & 3][(y + 8) & 15][2], every (row, segment) has a pair of its own inside the frame, and the 16 rows x 4
segments of one step of the y kernel (rows J + 8 .. J + 23 of a 64-column block) are one contiguous 512-byte run."""
import ctypes as C

import pytest

from acf_amd import capi

WIDTHS = [48, 64, 68, 76, 132, 192]
HEIGHTS = [48, 52, 56, 72]


def layout(h, w, x, y):
    out = (C.c_int64 * 2)()
    assert capi.load().acf_hip_tri_ck_layout(h, w, x, y, out) == 0
    return int(out[0]), int(out[1])


@pytest.mark.parametrize("w", WIDTHS)
@pytest.mark.parametrize("h", HEIGHTS)
def test_checkpoint_index_and_buffer_size(h, w):
    nyb = (h + 8 + 15) // 16
    _, floats = layout(h, w, 0, 0)
    assert floats == ((w + 63) // 64) * nyb * 128                  # an eighth of the blocked plane U: [w / 64][nyb] blocks of 64 x 16
    assert floats * 8 == ((w + 63) // 64) * nyb * 1024
    seen = {}
    for y in range(h):
        for x in range(w):
            idx, f2 = layout(h, w, x, y)
            assert f2 == floats
            want = ((((x >> 6) * nyb + ((y + 8) >> 4)) * 4 + ((x >> 4) & 3)) * 16 + ((y + 8) & 15)) * 2
            assert idx == want and idx % 2 == 0 and 0 <= idx and idx + 2 <= floats, (x, y, idx)
            seen.setdefault(idx, set()).add((x >> 4, y))
    # one pair per (segment, row): the columns of a segment share it, nothing else does
    assert all(len(v) == 1 for v in seen.values())
    assert len(seen) == ((w + 15) // 16) * h
    # a step of the y kernel: rows J + 8 .. J + 23 (inside the plane) x the 4 segments of a block = one aligned 128-float run
    for xb in range((w + 63) // 64):
        for kb in range(nyb):
            idxs = [layout(h, w, xb * 64 + 16 * s, y)[0] for s in range(4) if xb * 64 + 16 * s < w
                    for y in range(16 * kb - 8, 16 * kb + 8) if 0 <= y < h]
            if idxs:
                base = (xb * nyb + kb) * 128
                assert min(idxs) >= base and max(idxs) + 2 <= base + 128
                assert sorted(idxs) == sorted(base + 32 * s + 2 * r for s in range(4) if xb * 64 + 16 * s < w
                                              for r in range(16) if 0 <= 16 * kb - 8 + r < h)


def test_layout_refuses_points_outside_the_plane():
    out = (C.c_int64 * 2)()
    lib = capi.load()
    for (h, w, x, y) in [(48, 48, 48, 0), (48, 48, 0, 48), (48, 48, -1, 0), (0, 48, 0, 0)]:
        assert lib.acf_hip_tri_ck_layout(h, w, x, y, out) != 0
