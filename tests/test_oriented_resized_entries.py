"""The oriented resized entries, the part that needs no GPU (include/acf_hip.h: acf_hip_oriented_resized_dims and the definition the
GPU tests compare against; tests/oriented_resized_case.py holds the case table).
  1. acf_hip_oriented_resized_dims is acf_hip_resize_dims of acf_hip_oriented_dims, and refuses what either refuses
  2. every case detects something in every frame by the oracle alone — so that no GPU comparison is vacuous
  3. orient-then-resize and resize-then-orient give different bytes for a case of every resize form — so that the GPU tests tell the
     defined order from the other one
  4. the case table reaches every resize form in all eight orientations, and reduced frames that are no multiple of the tile"""
import ctypes as C

import numpy as np
import pytest

import orient_ref as orf
import oriented_resized_case as orc
import resized_entry_case as rc
from acf_amd import capi
from acf_amd.detector import HipDetector, HipError


def test_dims_are_the_two_host_functions_composed():
    for code in range(8):
        for rows, cols in ((240, 320), (241, 321), (299, 401), (1, 1), (2160, 3840), (37, 1023)):
            for scale in (orc.S150, orc.S64, 0.5, 1.0 / 3.0, 0.37, 0.2, 1.0, 2.0):
                up = HipDetector.oriented_dims(rows, cols, code)
                try:
                    want = HipDetector.resize_dims(up[0], up[1], scale)
                except HipError:
                    with pytest.raises(HipError):
                        HipDetector.oriented_resized_dims(rows, cols, code, scale)
                    continue
                assert HipDetector.oriented_resized_dims(rows, cols, code, scale) == want, (code, rows, cols, scale)
    for c in orc.CASES:
        assert HipDetector.oriented_resized_dims(c.H, c.W, c.code, c.scale) == orc.reduced_dims(c), c.id


def test_dims_refuse_bad_arguments():
    lib = capi.load()
    h, w = C.c_int(), C.c_int()
    ok = lambda *a: lib.acf_hip_oriented_resized_dims(*a)
    assert ok(240, 320, 1, C.c_double(0.5), C.byref(h), C.byref(w)) == capi.OK and (h.value, w.value) == (160, 120)
    for rows, cols, code, scale in ((240, 320, 8, 0.5), (240, 320, -1, 0.5), (0, 320, 1, 0.5), (240, 0, 1, 0.5), (-2, 320, 1, 0.5), (240, 320, 1, 0.0),
                                    (240, 320, 1, -0.5), (240, 320, 1, float("nan")), (240, 320, 1, float("inf")), (1, 1, 1, 0.2)):
        assert ok(rows, cols, code, C.c_double(scale), C.byref(h), C.byref(w)) == capi.E_INVALID, (rows, cols, code, scale)
    assert ok(240, 320, 1, C.c_double(0.5), None, C.byref(w)) == capi.E_INVALID
    assert ok(240, 320, 1, C.c_double(0.5), C.byref(h), None) == capi.E_INVALID


@pytest.mark.parametrize("case", orc.CASES, ids=orc.IDS)
def test_every_case_detects_something_in_every_frame(oracle, case):
    plan, want = orc.expected(oracle, case)
    counts = [len(w[1]) for w in want]
    assert min(counts) > 0, (case.id, counts)


@pytest.mark.parametrize("cid", orc.ORDER_CASES)
def test_the_two_orders_give_different_bytes(oracle, cid):
    case = orc.by_id(cid)
    stored, up = orc.built(case).packed, orc.upright(case)
    for f in range(orc.NF):
        first = oracle.resize_u8(up[f], case.scale)                                   # the definition: orient, then resize
        other = orf.orient(oracle.resize_u8(np.ascontiguousarray(stored[f]), case.scale), case.code)
        assert first.shape != other.shape or not np.array_equal(first, other), (cid, f)


def test_the_case_table_covers_what_it_claims():
    forms = {}
    for c in orc.CASES:
        forms.setdefault((orc.input_of(c), rc.form_of(c.scale)), set()).add(c.code)
        dr, dc = orc.reduced_dims(c)
        assert dr > 64 and dc > 64 and (dr % 64 or dc % 64), c.id
    for inp in ("i420", "nchw"):
        for form in ("area", "area_int", "linear"):
            assert forms[(inp, form)] >= set(range(1, 8)), (inp, form)                # (code 0 forwards: the GPU test's own case)
    for cid in ("i420_frac_o1", "i420_half_o1", "i420_up_o7"):
        dr, dc = orc.reduced_dims(orc.by_id(cid))
        assert dr % 64 and dc % 64, cid
    classes = {orc.input_of(c) for c in orc.CASES if c.src[0] == "rc" and c.code in (1, 6)}
    assert classes == {c[7] for c in rc.CASES}
    assert {rc.form_of(orc.by_id(cid).scale) for cid in orc.ORDER_CASES} == {"area", "area_int", "linear"}
    assert any(c.form == "generic" and c.scale < 0.25 for c in orc.CASES) and any(c.arith for c in orc.CASES)
    assert any(c.src[0] == "own" and c.src[2] % 4 for c in orc.CASES)
