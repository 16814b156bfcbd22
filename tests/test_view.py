"""Affine views of the stored frame without a GPU (include/acf_hip.h: "affine views of the stored frame"): the declarations, the
host-only entries acf_hip_view_from_box / view_quad / view_box / view_form against the numpy restatement (tests/view_ref.py), the
properties of that restatement which the GPU test (tests/test_gpu_view.py) then relies on — the identity and the integer translation
reproduce the pixels — and the precondition that every general GPU case detects something."""
import ctypes as C
import math
import os
import re

import numpy as np
import pytest

import view_ref as vr
from acf_amd import capi
from acf_amd.detector import HipDetector, HipError

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F = np.float32
ENTRIES = ["acf_hip_pyramid_view", "acf_hip_run_view", "acf_hip_view_from_box", "acf_hip_view_quad", "acf_hip_view_box", "acf_hip_view_form"]


def bits(a):
    return np.ascontiguousarray(a, dtype=F).view(np.uint32)


def test_header_declares_the_entries_and_the_abi_stays_9():
    text = open(os.path.join(ROOT, "include", "acf_hip.h")).read()
    assert re.search(r"#define ACF_HIP_ABI_VERSION 9\b", text)
    lib = capi.load()
    assert lib.acf_hip_abi_version() == 9
    for name in ENTRIES:
        assert re.search(r"ACF_HIP_API int %s\(" % name, text), name
        assert name in capi.DECLARED_SYMBOLS and getattr(lib, name).argtypes is not None


def test_view_from_box_exact_cases_bit_for_bit():
    """Angle 0 and exact halvings: no libm in the way (cos 0 = 1, sin 0 = 0), so the formula in float64 rounded to float32 is the answer."""
    n = 0
    for (h, w) in ((96, 128), (64, 64), (37, 53)):
        for b in ((0, 0, w, h), (0, 0, w / 2, h / 2), (10, 10, 150, 112.5), (-10, -10, 190, 170), (3.25, 7.5, w / 4, h / 8), (1e6, -1e6, 0.125, 3e5)):
            got, want = HipDetector.view_from_box(b, 0.0, h, w), vr.from_box(b, 0.0, h, w)
            assert got.dtype == F and np.array_equal(bits(got), bits(want)), (h, w, b, got, want)
            n += 1
    assert n == 18
    assert np.array_equal(HipDetector.view_from_box((0, 0, 128, 96), 0.0, 96, 128), vr.IDENTITY)          # the frame itself: the identity
    assert np.array_equal(HipDetector.view_from_box((7, 5, 128, 96), 0.0, 96, 128), vr.translation(7, 5))
    assert np.array_equal(HipDetector.view_from_box((0, 0, 64, 48), 0.0, 96, 128), np.array([0.5, 0, 0, 0, 0.5, 0], dtype=F))


def test_view_from_box_other_angles_within_an_ulp_of_libm():
    """relative 1e-6: half an ulp of float32 is 6e-8; the margin covers an ulp of cos / sin between libms"""
    for d in (20, -35, 5, 40, -40, 90, 180, 123.456):
        a = vr.deg(d)
        for b in ((10, 10, 150, 112.5), (30, 20, 110, 82.5), (40, 30, 64, 48)):
            got, want = HipDetector.view_from_box(b, a, vr.H, vr.W).astype(np.float64), vr.from_box(b, a, vr.H, vr.W).astype(np.float64)
            scale = np.abs(want).max()
            assert np.all(np.abs(got - want) <= 1e-6 * scale), (d, b, got, want)
    # a turn about the centre keeps the centre
    m = HipDetector.view_from_box((30, 20, 110, 82.5), vr.deg(-35), vr.H, vr.W).astype(np.float64)
    cx, cy = m[0] * vr.W / 2 + m[1] * vr.H / 2 + m[2], m[3] * vr.W / 2 + m[4] * vr.H / 2 + m[5]
    assert abs(cx - 85) < 1e-4 and abs(cy - 61.25) < 1e-4


def test_view_quad_and_box_follow_the_same_affine_map():
    dets = [(0, 0, 1, 1), (3, 4, 20, 30), (-9, 4, 80, 80), (100, 60, 28, 36), (0, 0, vr.W, vr.H)]
    for name, (m, _) in vr.VIEWS.items():
        for d in dets:
            q, b = HipDetector.view_quad(m, d), HipDetector.view_box(m, d)
            wq, wb = vr.quad(m, d), vr.box(m, d)
            assert q.dtype == F and q.shape == (4, 2) and np.array_equal(bits(q), bits(wq.astype(F))), (name, d)
            assert np.array_equal(bits(b), bits(wb)), (name, d)
            # the box bounds the quad
            assert b[0] <= q[:, 0].min() and b[1] <= q[:, 1].min() and b[0] + b[2] >= q[:, 0].max() - 1e-3 and b[1] + b[3] >= q[:, 1].max() - 1e-3
    # an un-rotated view: the box of a detection is the box from_box was given, scaled — the whole frame gives the box back
    for bx in ((10, 10, 150, 112.5), (-10, -10, 190, 170), (40, 30, 64, 48)):
        m = HipDetector.view_from_box(bx, 0.0, vr.H, vr.W)
        assert np.allclose(HipDetector.view_box(m, (0, 0, vr.W, vr.H)), np.array(bx, dtype=F), rtol=0, atol=1e-4), bx
        sx, sy = bx[2] / vr.W, bx[3] / vr.H
        assert np.allclose(HipDetector.view_box(m, (32, 24, 64, 48)), [bx[0] + 32 * sx, bx[1] + 24 * sy, 64 * sx, 48 * sy], rtol=0, atol=1e-4), bx
    lib, q = capi.load(), np.zeros(8, F)
    det = (C.c_int32 * 4)(1, 2, 3, 4)
    assert lib.acf_hip_view_quad(None, det, capi.fptr(q)) == capi.E_INVALID
    assert lib.acf_hip_view_quad(capi.fptr(vr.IDENTITY.copy()), None, capi.fptr(q)) == capi.E_INVALID
    assert lib.acf_hip_view_box(capi.fptr(vr.IDENTITY.copy()), det, None) == capi.E_INVALID
    assert lib.acf_hip_view_from_box(None, 0.0, 4, 4, capi.fptr(q)) == capi.E_INVALID
    assert lib.acf_hip_view_from_box(capi.fptr(q), 0.0, 0, 4, capi.fptr(q)) == capi.E_INVALID


def test_view_form_table_and_the_gpu_cases_take_both_forms():
    """The rule on a table of tiles, and which form the GPU cases' tiles take: a rule change cannot silently drop a form."""
    Hu, Wu = vr.HS, vr.WS
    # an upright tile stages 67 x 67 code values of every source but three f32 channels (3 * 67 * 67 * 4 bytes > 32 KiB)
    for (ch, sb, want) in ((3, 1, 0), (1, 1, 0), (3, 2, 0), (1, 4, 0), (1, 2, 0), (3, 4, 1)):
        assert vr.form(vr.IDENTITY, 1, 0, 0, vr.H, vr.W, Hu, Wu, ch, sb) == want, (ch, sb)
    # more than four stored pixels a sample: a reduction by 2.5 gathers whatever the codes; by 1.5 it stages bytes; samples do not change
    # the rectangle, only the count
    big = HipDetector.view_from_box((0, 0, 2.5 * 128, 2.5 * 96), 0.0, 96, 128)
    mid = HipDetector.view_from_box((0, 0, 1.5 * 128, 1.5 * 96), 0.0, 96, 128)
    assert vr.form(big, 1, 0, 0, 96, 128, 1000, 1000, 3, 1) == 1 and vr.form(big, 1, 0, 0, 96, 128, 1000, 1000, 1, 1) == 1
    assert vr.form(big, 2, 0, 0, 96, 128, 1000, 1000, 1, 1) == 0                       # four times the samples under the same rectangle
    assert vr.form(mid, 1, 0, 0, 96, 128, 1000, 1000, 3, 1) == 0 and vr.form(mid, 1, 0, 0, 96, 128, 1000, 1000, 3, 2) == 1
    # a view wholly outside the frame clamps to one pixel: staged, of every source
    assert vr.form(vr.translation(1e9, -1e9), 1, 1, 1, 96, 128, Hu, Wu, 3, 4) == 0
    # NaN and infinite coefficients have a form too (the coordinates clamp)
    for bad in (np.array([np.nan] * 6, F), np.array([np.inf, -np.inf, 0, 1, 1, np.nan], F)):
        assert vr.form(bad, 2, 0, 0, 96, 128, Hu, Wu, 3, 1) in (0, 1)
    seen = {"u8": set(), "f32": set(), "nv12": set()}
    for name, (m, s) in vr.VIEWS.items():
        seen["u8"] |= set(vr.forms(m, s, vr.H, vr.W, Hu, Wu, 3, 1))
        seen["nv12"] |= set(vr.forms(m, s, vr.H, vr.W, Hu, Wu, 3, 1))
        seen["f32"] |= set(vr.forms(m, s, vr.H, vr.W, Hu, Wu, 3, 4))
    assert seen["u8"] == {0} and seen["f32"] == {0, 1}, seen                          # bytes stage every tile here; f32 x 3 gathers by size
    assert 1 in set(vr.forms(vr.IDENTITY, 1, 130, 136, 130, 136, 3, 4))                # the identity cases: f32 / 16-bit gathers and stages
    assert set(vr.forms(vr.IDENTITY, 1, 96, 128, 96, 128, 3, 2)) == {0}
    # the arguments
    lib, out, m = capi.load(), C.c_int(), capi.fptr(vr.IDENTITY.copy())
    assert lib.acf_hip_view_form(m, 1, 1, 1, 96, 128, Hu, Wu, 3, 1, C.byref(out)) == 0
    for args in ((None, 1, 0, 0, 96, 128, Hu, Wu, 3, 1, C.byref(out)), (m, 0, 0, 0, 96, 128, Hu, Wu, 3, 1, C.byref(out)), (m, 5, 0, 0, 96, 128, Hu, Wu, 3, 1, C.byref(out)),
                 (m, 1, 2, 0, 96, 128, Hu, Wu, 3, 1, C.byref(out)), (m, 1, 0, 2, 96, 128, Hu, Wu, 3, 1, C.byref(out)), (m, 1, -1, 0, 96, 128, Hu, Wu, 3, 1, C.byref(out)),
                 (m, 1, 0, 0, 96, 128, 0, Wu, 3, 1, C.byref(out)), (m, 1, 0, 0, 96, 128, Hu, Wu, 2, 1, C.byref(out)), (m, 1, 0, 0, 96, 128, Hu, Wu, 3, 3, C.byref(out)),
                 (m, 1, 0, 0, 96, 128, Hu, Wu, 3, 1, None)):
        assert lib.acf_hip_view_form(*args) == capi.E_INVALID, args[1:10]


def test_refusals_that_need_no_device():
    lib = capi.load()
    desc = capi.ImageDesc(capi.T_U8, 3, 0, 1, 3 * 8, 3)
    src = capi.CropSource(C.c_void_p(256), 1, C.pointer(desc), None, None, 8, 8, 0)
    views = C.c_void_p(256)
    for fn in (lib.acf_hip_pyramid_view, lib.acf_hip_run_view):
        assert fn(None, C.byref(src), views, None, 1, 1) == capi.E_INVALID             # no context
        assert fn(None, None, views, None, 1, 1) == capi.E_INVALID
        assert fn(None, C.byref(src), None, None, 1, 1) == capi.E_INVALID
        assert fn(None, C.byref(src), views, None, 1, 0) == capi.E_INVALID
        assert fn(None, C.byref(src), views, None, 1, 5) == capi.E_INVALID


# ---------------------------------------------------------------- the numpy restatement's own properties

def _frame(seed, h, w, c=3):
    return np.random.RandomState(seed).randint(0, 256, (h, w, c)).astype(F)


def test_ref_identity_reproduces_the_pixels():
    U = _frame(1, 37, 53)
    assert np.array_equal(vr.sample(U, vr.IDENTITY, 37, 53, 1), U)
    Uf = (np.random.RandomState(2).rand(37, 53, 1) * 1.5 - 0.25).astype(F)
    assert np.array_equal(bits(vr.sample(Uf, vr.IDENTITY, 37, 53, 1)), bits(Uf))       # (no negative zero in it)
    u, v = vr.coords(vr.IDENTITY, 37, 53, 1, 37, 53)
    assert np.array_equal(u, np.broadcast_to(np.arange(53, dtype=F), (37, 53))) and np.array_equal(v[:, 0], np.arange(37, dtype=F))


def test_ref_integer_translation_is_the_slice():
    """The consequence the GPU test checks through acf_hip_run_image on the strided sub-view: restated sampling == the slice, every bit."""
    U8 = vr.stored_u8()[1][0]
    Uf = vr.stored_f32()[1][1]
    for U in (U8, Uf):
        for (tx, ty) in ((7, 5), (0, 0), (vr.WS - vr.W, vr.HS - vr.H), (1, 53)):
            got = vr.sample(U, vr.translation(tx, ty), vr.H, vr.W, 1)
            assert np.array_equal(bits(got), bits(U[ty:ty + vr.H, tx:tx + vr.W])), (tx, ty)


def test_ref_border_nan_and_bad_frames():
    U = _frame(3, 37, 53)
    for m, want in ((vr.translation(1e9, 1e9), U[36, 52]), (vr.translation(-1e9, -1e9), U[0, 0]), (vr.translation(1e9, -1e9), U[0, 52]),
                    (np.array([np.nan] * 6, F), U[0, 0]), (np.array([np.inf, -np.inf, 0, 0, 0, np.inf], F), U[36, 0])):
        val = vr.sample(U, m, 9, 11, 2)
        assert np.array_equal(val, np.broadcast_to(want, val.shape)), m
    img = vr.image(U[None], [vr.IDENTITY, vr.IDENTITY, vr.IDENTITY], [-1, 0, 1], 9, 11, 1, F(1 / 255.0))
    assert img.shape == (3, 3, 9, 11) and not img[0].any() and not img[2].any() and img[1].any()
    # samples: the s x s mean, accumulated in order, times float(1 / (s * s)): a reduction by 2 with 2 samples (float(1 / 2) is exact)
    # reads every pixel once
    U1 = _frame(4, 12, 12, 1)
    val = vr.sample(U1, np.array([2, 0, 0, 0, 2, 0], F), 6, 6, 2)
    acc = np.zeros((6, 6, 1), dtype=F)
    for a in range(2):
        for b in range(2):
            acc = acc + U1[a::2, b::2]
    assert np.array_equal(val, acc * F(0.25))


@pytest.mark.parametrize("kind", ["u8", "f32"])
def test_every_general_gpu_case_detects_something(oracle, kind):
    """The precondition against vacuous GPU comparisons: the restatement's image of every general view through the CPU oracle."""
    for name in vr.DETECTING:
        n = vr.oracle_hits(kind, name)
        assert 0 < n <= vr.MAX_HITS, (kind, name, n)
