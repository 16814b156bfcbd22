"""Affine views of the stored frame (include/acf_hip.h: acf_hip_pyramid_view / run_view / view_from_box / view_quad / view_box /
view_form; kernel k_ingest_view): the header's definition restated in numpy, and the views and sources the CPU and GPU tests share.
Helper of tests/test_view.py, tests/test_gpu_view.py and tests/test_host_cpp_view.py.

Every operation is a float32 operation rounded once, as the header says: numpy's float32 arithmetic is exactly that, so the GPU tests
compare raw bits.  The restatement takes the UPRIGHT frame U [Hu][Wu][C] as exact float32 code values (cut_crops_ref's convention) and
gives the tight planar float32 image [C][h][w] the call is defined to be acf_hip_run_image on."""
import functools
import math

import numpy as np

from acf_amd import capi, synth

F = np.float32
TILE = 64
IDENTITY = np.array([1, 0, 0, 0, 1, 0], dtype=F)


def translation(tx, ty):
    return np.array([1, 0, tx, 0, 1, ty], dtype=F)


def from_box(box, angle, h, w):
    """acf_hip_view_from_box: in float64 from the float32 box, rounded to float32."""
    bx, by, bw, bh = (float(F(v)) for v in box)
    sx, sy, ca, sa = bw / w, bh / h, math.cos(angle), math.sin(angle)
    m0, m1, m3, m4 = sx * ca, -sy * sa, sx * sa, sy * ca
    cx, cy = bx + bw / 2, by + bh / 2
    return np.array([m0, m1, cx - (m0 * w + m1 * h) / 2, m3, m4, cy - (m3 * w + m4 * h) / 2], dtype=np.float64).astype(F)


def quad(m, det):
    """acf_hip_view_quad: the corners TL, TR, BR, BL of a detection (x, y, w, h) of the view's frame in U, float32 [4][2]."""
    m = np.asarray(m, dtype=F).astype(np.float64)
    x, y, w, h = (float(int(v)) for v in det)
    pts = [(x, y), (x + w, y), (x + w, y + h), (x, y + h)]
    return np.array([[m[0] * px + m[1] * py + m[2], m[3] * px + m[4] * py + m[5]] for px, py in pts], dtype=np.float64)


def box(m, det):
    """acf_hip_view_box: the quad's bounding box (x, y, w, h) in U, from the unrounded corners."""
    q = quad(m, det)
    lo, hi = q.min(axis=0), q.max(axis=0)
    return np.array([lo[0], lo[1], hi[0] - lo[0], hi[1] - lo[1]], dtype=np.float64).astype(F)


def coords(m, h, w, s, Hu, Wu):
    """The clamped sample coordinates (u, v) [h * s][w * s] float32 of a view."""
    m = np.asarray(m, dtype=F)
    inv = F(1.0 / s)
    py = ((np.arange(h * s).astype(F) + F(0.5)) * inv)[:, None]
    px = ((np.arange(w * s).astype(F) + F(0.5)) * inv)[None, :]
    with np.errstate(all="ignore"):
        u = (((m[0] * px) + (m[1] * py)) + m[2]) - F(0.5)
        v = (((m[3] * px) + (m[4] * py)) + m[5]) - F(0.5)
    assert u.dtype == F and v.dtype == F
    u = np.where(u > F(0), u, F(0))                       # (NaN becomes 0)
    u = np.where(u < F(Wu - 1), u, F(Wu - 1))
    v = np.where(v > F(0), v, F(0))
    v = np.where(v < F(Hu - 1), v, F(Hu - 1))
    return u, v


def sample(U, m, h, w, s):
    """val [h][w][C] float32 of one view of the upright frame U [Hu][Wu][C] float32 (not yet scaled by unit)."""
    U = np.asarray(U)
    assert U.dtype == F and U.ndim == 3
    Hu, Wu, C = U.shape
    u, v = coords(m, h, w, s, Hu, Wu)
    c0 = np.clip(np.floor(u).astype(np.int64), 0, Wu - 1)
    r0 = np.clip(np.floor(v).astype(np.int64), 0, Hu - 1)
    c1, r1 = np.minimum(c0 + 1, Wu - 1), np.minimum(r0 + 1, Hu - 1)
    fx, fy = (u - c0.astype(F))[..., None], (v - r0.astype(F))[..., None]
    p00, p01, p10, p11 = U[r0, c0], U[r0, c1], U[r1, c0], U[r1, c1]
    with np.errstate(all="ignore"):
        top = p00 + fx * (p01 - p00)
        bot = p10 + fx * (p11 - p10)
        smp = (top + fy * (bot - top)).reshape(h, s, w, s, C)
        acc = np.zeros((h, w, C), dtype=F)
        for a in range(s):
            for b in range(s):
                acc = acc + smp[:, a, :, b, :]
        val = acc * F(1.0 / (s * s))
    assert val.dtype == F
    return val


def image(Us, views, frames, h, w, s, unit):
    """The tight planar float32 image [n][C][h][w] of views[i] of upright frame frames[i] (None: i) of Us [nF][Hu][Wu][C]; a frame index
    outside [0, nF) gives the frame of all-zero code values."""
    out = []
    for i, m in enumerate(views):
        f = i if frames is None else int(frames[i])
        U = Us[f] if 0 <= f < len(Us) else np.zeros_like(Us[0])
        with np.errstate(all="ignore"):
            out.append((sample(U, m, h, w, s) * F(unit)).transpose(2, 0, 1))
    return np.ascontiguousarray(np.stack(out), dtype=F)


def form(m, s, tx, ty, h, w, Hu, Wu, C, sb):
    import ctypes as Ct
    out = Ct.c_int(-1)
    mm = np.ascontiguousarray(m, dtype=F)
    rc = capi.load().acf_hip_view_form(capi.fptr(mm), s, tx, ty, h, w, Hu, Wu, C, sb, Ct.byref(out))
    assert rc == 0, rc
    return out.value


def forms(m, s, h, w, Hu, Wu, C, sb):
    """the forms of every tile of one view"""
    return [form(m, s, tx, ty, h, w, Hu, Wu, C, sb) for ty in range(-(-h // TILE)) for tx in range(-(-w // TILE))]


# ---------------------------------------------------------------- the general GPU cases (the CPU test holds the preconditions on them)

H, W = 96, 128            # the plan
HS, WS = 150, 170         # the stored frames
NF = 2
SEEDS = (40, 41)
MODEL_KW = dict(seed=3, name="TINY", nTrees=96, cascThr=-3.0)
MAX_HITS = 4096


def model():
    return synth.make_model(**MODEL_KW)


def deg(d):
    return d * math.pi / 180.0


# name -> (view, samples): the issue's five, a mirror-and-shear and a view lying wholly outside the frame
VIEWS = {
    "integer cut (7, 5)": (translation(7, 5), 1),
    "tilt 20, s 1": (from_box((10, 10, 150, 112.5), deg(20), H, W), 1),
    "tilt -35, s 2": (from_box((30, 20, 110, 82.5), deg(-35), H, W), 2),
    "zoom-out over the border, s 2": (from_box((-10, -10, 190, 170), 0.0, H, W), 2),
    "zoom-in tilt 5, s 1": (from_box((40, 30, 64, 48), deg(5), H, W), 1),
    "mirror and shear, s 1": (np.array([-1.0, 0.25, 160.5, 0.125, 1.125, 3.25], dtype=F), 1),
    "wholly outside, s 1": (translation(400, -300), 1),
}
# the views of VIEWS that must detect something (a view outside the frame is one colour: nothing to find)
DETECTING = [k for k in VIEWS if not k.startswith("wholly outside")]


@functools.lru_cache(maxsize=None)
def stored_values():
    """[NF][3][HS][WS] float32 in [0, 1]: synth frames, upright"""
    return np.stack([synth.make_frame(sd, HS, WS, "luv").transpose(0, 2, 1) for sd in SEEDS]).astype(F)


@functools.lru_cache(maxsize=None)
def stored_u8():
    """(elements uint8 [NF][HS][WS][3] as an NHWC tensor holds them, U [NF][HS][WS][3]: their exact float32 code values)"""
    e = np.clip(np.rint(stored_values().astype(np.float64) * 255.0), 0, 255).astype(np.uint8).transpose(0, 2, 3, 1)
    e = np.ascontiguousarray(e)
    return e, e.astype(F)


@functools.lru_cache(maxsize=None)
def stored_f32():
    """(elements float32 [NF][3][HS][WS] (NCHW), U [NF][HS][WS][3])"""
    e = np.ascontiguousarray(stored_values())
    return e, np.ascontiguousarray(e.transpose(0, 2, 3, 1))


def frame_choice(name):
    """which stored frame a general case reads when frame indices are given"""
    return list(VIEWS).index(name) % NF


@functools.lru_cache(maxsize=None)
def oracle_hits(kind, name):
    """hits of the CPU oracle on the restatement's image of one general view (frame_choice), kind "u8" or "f32" """
    from oracle import binding as ob
    m, s = VIEWS[name]
    U, unit = (stored_u8()[1], F(1 / 255.0)) if kind == "u8" else (stored_f32()[1], F(1))
    img = image(U, [m], [frame_choice(name)], H, W, s, unit)[0]          # [3][H][W]
    plan = ob.Plan(model(), H, W, 3)
    pyr, _, _ = ob.chns_pyramid(plan, np.ascontiguousarray(img.transpose(0, 2, 1)))
    _, hits = ob.detect(plan, pyr)
    return len(hits)
