"""The resized tensor and YUV entries without a GPU: the header and the bindings, the case table of tests/resized_entry_case.py
against itself, and the precondition of tests/test_gpu_resized_entries.py — that the oracle finds something in every case."""
import os
import re

import numpy as np
import pytest

import resized_entry_case as rc
import yuv_desc_ref as ydr
from acf_amd import capi
from acf_amd.detector import HipDetector

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRIES = ["acf_hip_pyramid_yuv_resized", "acf_hip_run_yuv_resized", "acf_hip_pyramid_image_resized", "acf_hip_run_image_resized",
           "acf_hip_stream_open_yuv_resized"]


def test_entries_are_declared_and_bound_and_the_abi_stays():
    hdr = open(os.path.join(ROOT, "include", "acf_hip.h")).read()
    lib = capi.load()
    for e in ENTRIES:
        assert re.search(r"ACF_HIP_API int %s\(acf_hip_ctx\* ctx," % e, hdr), e
        assert e in capi.DECLARED_SYMBOLS, e
        assert getattr(lib, e).argtypes is not None and getattr(lib, e).restype is not None, e
    assert re.search(r"#define ACF_HIP_ABI_VERSION 9\b", hdr)
    assert lib.acf_hip_abi_version() == 9
    for host in ("acf_hip_loader.h", "acf_hip_loader.cpp"):
        src = open(os.path.join(ROOT, "acf_amd", "host", host)).read()
        for e in ENTRIES:
            assert "ACF_HIP_FN(%s)" % e in src, (host, e)


def test_case_table_is_self_consistent(oracle):
    assert len(rc.CASES) == 11 and len(set(rc.IDS)) == 11
    assert rc.form_of(rc.S150) == "area" and rc.form_of(rc.S64) == "linear" and rc.S64 == 1.25
    for case in rc.CASES:
        name, H, W, dr, dc, scale, form, inp, model, d_in = case
        assert HipDetector.resize_dims(H, W, scale) == (dr, dc) == oracle.resize_dims(H, W, scale), name
        assert rc.form_of(scale) == form, name
        b = rc.built(case)
        assert b.packed.shape == (rc.NF, H, W, d_in) and b.packed.dtype == np.uint8, name
        if b.kind == "yuv":
            lo, hi = HipDetector.yuv_extent(b.desc, H, W, rc.NF)
            assert b.base + min(lo) >= 0 and b.base + max(hi) < b.buf.size, name
            ydr.gather(b.buf, b.desc, H, W, rc.NF, b.base)                # (asserts every addressed byte inside the buffer)
        else:
            lo, hi = HipDetector.image_extent(b.desc, H, W, rc.NF)
            assert b.base + lo >= 0 and b.base + hi < b.buf.size, name
            d = b.desc
            idx = (b.base + d.stride_n * np.arange(rc.NF)[:, None, None, None] + d.stride_y * np.arange(H)[None, :, None, None] +
                   d.stride_x * np.arange(W)[None, None, :, None] + d.stride_c * np.arange(d.channels)[None, None, None, :])
            assert idx.min() == b.base + lo and idx.max() == b.base + hi
            assert np.array_equal(b.buf[idx], b.packed), name              # `packed` is the addressed bytes, interleaved
    # the forks the table names
    by = {c[0]: c for c in rc.CASES}
    assert by["planes_odd_037"][3] * by["planes_odd_037"][4] % 4 != 0       # the scalar rgb2luv body, no float4 stores
    assert by["planes_odd_037"][3] % 4 != 0
    assert by["i444_odd_third"][1] % 3 != 0 and by["i444_odd_third"][2] % 3 != 0   # partial cells at both edges
    t = rc.built(by["planes_odd_037"])
    assert t.desc.u.offset < 0 and t.desc.v.offset < 0
    assert by["i420_area_frac"][4] % 64 != 0 and by["nv12_linear_up"][3] % 64 != 0 and by["nv12_linear_up"][3] > 256


@pytest.mark.parametrize("case", rc.CASES, ids=rc.IDS)
def test_the_oracle_finds_something_in_every_case(oracle, case):
    """Else the GPU comparison of detections would pass emptily."""
    plan, out = rc.expected(oracle, case)
    assert sum(len(det) for _, det, _ in out) > 0, case[0]
