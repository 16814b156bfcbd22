"""The oriented resized tensor and YUV entries (include/acf_hip.h: acf_hip_pyramid_image_oriented_resized / run_image_oriented_resized /
pyramid_yuv_oriented_resized / run_yuv_oriented_resized / stream_open_yuv_oriented_resized; kernel k_ingest_oriented_resized): the case
table and what the CPU and GPU tests share.  Helper of tests/test_oriented_resized_entries.py and tests/test_gpu_oriented_resized_entries.py.

A case is a stored input (two frames, so that stride_n matters), an orientation code and a scale.  The definition: the stored bytes
(`packed` of tests/resized_entry_case.py: for YUV the R, G, B of the numpy restatement, chroma chosen in SOURCE coordinates) are turned
upright (tests/orient_ref.py) and THEN reduced: upright(case) is the tight upright u8 image [NF][rows][cols][cn] the existing
acf_hip_run_image_resized takes; expected(oracle, case) is the oracle chain on it (oracle.resize_u8 -> acfo_ingest_u8 -> chnsPyramid ->
acfDetect), computed once per process and shared.

Shapes: stored frames of about 240 x 320 (odd: 241 x 321, 299 x 401), so that the reduced frame is more than one 64 x 64 tile and no
multiple of 64 on either axis (tile edges in x and in y, in the reduced frame and — through the footprint — in the stored one).
Every resize form (resized_entry_case.form_of): `area` fractional at resize_scale(80, 150) and 0.37; `area_int` at 0.5 (the 2 x 2
shortcut) and 1 / 3 on sources whose last cells are partial; `linear` at 1.25 (the second-tap flag at xmax).  One case at 0.2 (under
1 / 4: the footprint of eight reduced rows does not fit the stage) on a source of 480 x 640, so that the reduced frame still holds a
window, lands in the generic form by footprint.

Run as a program it prints, for every case, "<id> <sha256 of every level, detection and hit byte> <kernel names>" — the GPU test
starts it ONCE in a fresh child under ACF_HIP_FORCE_FALLBACK=oriented_resized_generic (the variable is read once per process)."""
import collections
import hashlib
import os
import sys

import numpy as np

if __name__ == "__main__":
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import orient_ref as orf
import resized_entry_case as rc
import yuv_desc_ref as ydr
from acf_amd import capi, synth
from acf_amd.detector import HipDetector

NF = rc.NF
S150, S64 = rc.S150, rc.S64
FACE80 = dict(rc.FACE80)
FACE80_RGB = dict(rc.FACE80_RGB)

# id; src: ("rc", a name of resized_entry_case.CASES) or ("own", input, lead bytes in front of the base); stored rows, cols; scale;
# code; model; input planes; option "arith"; form: the kernel form the library must choose ("staged" / "generic"), None: not asserted
Case = collections.namedtuple("Case", "id src H W scale code model d_in arith form")

# all 8 codes x all resize forms on one YUV input (I420: the planar dword loads) and one image input (uint8 NCHW: the row-vector loads)
SWEEP = [
    ("frac", S150, (242, 320), (242, 320)),          # 129 x 171
    ("037", 0.37, (240, 320), (241, 321)),           # 89 x 118 / 89 x 119
    ("half", 0.5, (240, 320), (240, 320)),           # 120 x 160: 2 x 2
    ("third", 1.0 / 3.0, (242, 320), (299, 401)),    # 81 x 107 / 100 x 134: the last cells reach past the source on both axes
    ("up", S64, (240, 320), (240, 320)),             # 300 x 400
]


def _form(wide, code, scale=1.0):
    """planOrientedResized's rule: staged for quarter turns where the footprint fits (scales from 1 / 4), whatever the load form"""
    return "staged" if scale >= 0.25 and code & 1 else "generic"


def _cases():
    out = []
    for tag, scale, yuv_size, img_size in SWEEP:
        for code in range(1, 8):
            # (the tight I420 frames are 4-aligned plane by plane; a tight NCHW tensor has 4-aligned rows only at a width of 4k)
            out.append(Case("i420_%s_o%d" % (tag, code), ("own", "i420", 0), yuv_size[0], yuv_size[1], scale, code, FACE80, 3, 0, _form(True, code)))
            out.append(Case("nchw_%s_o%d" % (tag, code), ("own", "nchw", 0), img_size[0], img_size[1], scale, code, FACE80_RGB, 3, 0,
                            _form(img_size[1] % 4 == 0, code)))
    # every input class of the resized entries, a quarter turn and a mirrored half turn (wide load forms: the aligned planar I420, the
    # NCHW and the grey tensor; i444_odd and three_planes lie off 4-byte alignment)
    wide = ("i420", "nchw", "gray")
    for c in rc.CASES:
        name, H, W, dr, dc, scale, form, inp, model, d_in = c
        for code in (1, 6):
            out.append(Case("%s_o%d" % (name, code), ("rc", name), H, W, scale, code, model, d_in, 0, _form(inp in wide, code)))
    # odd sizes WITH the wide loads: padded 4-aligned rows of 321 (161) samples, so that a row ends inside a quad
    for code in (1, 2, 7):
        out.append(Case("i420_padded_odd_037_o%d" % code, ("own", "i420_padded_odd", 0), 241, 321, 0.37, code, FACE80_RGB, 3, 0, _form(True, code)))
    # the base pointer off 4-byte alignment: the byte loads of the staged form (a quarter turn); no turn: the generic form
    out.append(Case("i420_lead1_half_o3", ("own", "i420", 1), 240, 320, 0.5, 3, FACE80, 3, 0, "staged"))
    out.append(Case("i420_lead1_frac_o4", ("own", "i420", 1), 242, 320, S150, 4, FACE80, 3, 0, "generic"))
    # option "arith" = 1: rgb2luv_sse's reciprocal from the CPU tables
    out.append(Case("nchw_frac_o5_arith", ("own", "nchw", 0), 242, 320, S150, 5, FACE80_RGB, 3, 1, "staged"))
    # under 1 / 4: generic by footprint
    out.append(Case("i420_fifth_o1", ("own", "i420", 0), 480, 640, 0.2, 1, FACE80, 3, 0, "generic"))
    out.append(Case("nchw_fifth_o6", ("own", "nchw", 0), 480, 640, 0.2, 6, FACE80_RGB, 3, 0, "generic"))
    return out


CASES = _cases()
IDS = [c.id for c in CASES]
# one case per resize form whose two orders differ (checked on the CPU), and the cases the GPU test names
ORDER_CASES = ["i420_frac_o1", "nchw_037_o3", "i420_third_o2", "nchw_third_o5", "i420_up_o7"]   # (2 x 2 cells on an even source commute)


def by_id(cid):
    return CASES[IDS.index(cid)]


def upright_dims(case):
    return orf.dims(case.H, case.W, case.code)


def reduced_dims(case):
    """cvRound of the upright size times scale (host_plan.cpp resizeDims), in numpy"""
    h, w = upright_dims(case)
    return int(np.rint(h * case.scale)), int(np.rint(w * case.scale))


def _build_own(case):
    _, inp, lead = case.src
    H, W = case.H, case.W
    seed0 = 300 + 11 * (H % 17) + (5 if inp == "nchw" else 0) + 3 * lead
    if inp == "i420_padded_odd":
        import oriented_case as oc
        buf, desc, fb = oc.planar_buffer([rc.yuv_planes(seed0 + f, H, W, 1, 1) for f in range(NF)], 324, 164, (1, 1))
        assert fb % 4 == 0
        return rc.Built(kind="yuv", desc=desc, buf=buf, base=0, packed=ydr.desc_to_rgb(buf, desc, H, W, NF), pix=capi.PIX_RGB, frame_bytes=fb)
    if inp == "i420":
        desc, fb = HipDetector.yuv_desc("i420", H, W)
        buf = np.concatenate([np.full(lead, 0x5A, np.uint8)] + [ydr.pack("i420", *rc.yuv_planes(seed0 + f, H, W, 1, 1)) for f in range(NF)])
        return rc.Built(kind="yuv", desc=desc, buf=buf, base=lead, packed=ydr.desc_to_rgb(buf, desc, H, W, NF, lead), pix=capi.PIX_RGB, frame_bytes=fb)
    rgb = np.stack([rc.rgb_u8(seed0 + f, H, W) for f in range(NF)])
    buf = np.ascontiguousarray(rgb.transpose(0, 3, 1, 2))
    desc = capi.ImageDesc(capi.T_U8, 3, 3 * H * W, H * W, W, 1)
    return rc.Built(kind="image", desc=desc, buf=buf.ravel(), base=0, packed=rgb, pix=capi.PIX_RGB, shape=buf.shape, layout="nchw")


_BUILT, _EXPECT = {}, {}


def input_of(case):
    """the input class: a name of resized_entry_case's (i420, nv12, yuyv_padded, ..., nchw, bgr, rgba, gray)"""
    return rc.CASES[rc.IDS.index(case.src[1])][7] if case.src[0] == "rc" else case.src[1]


def built(case):
    """resized_entry_case.Built of the STORED frames (shared by the cases of one source)"""
    key = case.src + (case.H, case.W)
    if key not in _BUILT:
        _BUILT[key] = rc.built(rc.CASES[rc.IDS.index(case.src[1])]) if case.src[0] == "rc" else _build_own(case)
    return _BUILT[key]


def upright(case):
    """uint8 [NF][rows][cols][cn]: the stored bytes turned upright, tight"""
    return np.ascontiguousarray(orf.orient(built(case).packed, case.code, axes=(1, 2)))


def expected(oracle, case):
    """(plan, per frame (pyramid, detections, hits)) of the oracle chain on upright(case); once per case"""
    if case.id not in _EXPECT:
        dr, dc = reduced_dims(case)
        plan = oracle.Plan(synth.make_model(**case.model), dr, dc, case.d_in)
        up = upright(case)
        if case.arith:
            oracle.set_x86_tables(*oracle.x86_fixture())
            oracle.set_approx(3)
        try:
            out = []
            for f in range(NF):
                red = oracle.resize_u8(up[f], case.scale)
                assert red.shape == (dr, dc, up.shape[3]), (red.shape, dr, dc)
                pyr, _, _ = oracle.chns_pyramid(plan, rc.oracle_planar(oracle, red))
                out.append((pyr,) + oracle.detect(plan, pyr))
        finally:
            if case.arith:
                oracle.set_approx(0)
        _EXPECT[case.id] = (plan, out)
    return _EXPECT[case.id]


# ---------------------------------------------------------------- what the GPU test and the child process share (torch from here on)

def bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def dev(buf):
    import torch
    return torch.from_numpy(np.ascontiguousarray(buf)).cuda()


def detector(case, oracle=None, **kw):
    dr, dc = reduced_dims(case)
    det = HipDetector(synth.make_model(**case.model), dr, dc, case.d_in, max_batch=NF, max_hits=1 << 17, **kw)
    if case.arith:
        det.set_x86_tables(*oracle.x86_fixture())
        det.set_option("arith", 1)
    return det


def run_entry(det, case, x, pyramid_only=False):
    """The case's stored frames (x: the device copy of built(case).buf) through the entry, by the Python method a caller would use."""
    b, inp = built(case), input_of(case)
    H, W, scale, code = case.H, case.W, case.scale, case.code
    if inp == "three_planes" and not pyramid_only:
        y, u, v = (x[at:at + int(np.prod(shape))].view(shape) for at, shape in b.planes)
        return det.run_yuv_planes(y, u, v, 1, 1, scale=scale, orient=code)
    if b.kind == "yuv":
        fn = det.pyramid_yuv_resized if pyramid_only else det.run_yuv_resized
        return fn(x.data_ptr() + b.base, NF, b.desc, H, W, scale, code)
    if inp in ("nchw", "gray"):
        fn = det.pyramid_tensor_resized if pyramid_only else det.run_tensor_resized
        return fn(x.view(b.shape), scale, orient=code)
    if inp == "rgba":
        fn = det.pyramid_tensor_resized if pyramid_only else det.run_tensor_resized
        return fn(x.view(NF, H, W, 4)[..., :3], scale, layout="nhwc", orient=code)
    fn = det.pyramid_image_resized if pyramid_only else det.run_image_resized          # bgr: a negative channel stride, no torch view
    return fn(x.data_ptr() + b.base, NF, b.desc, H, W, scale, code)


def snapshot(det):
    """Per frame (levels as uint32, detection bytes, hit bytes) of the last run."""
    out = []
    for f in range(NF):
        d, h = det.detections(f)
        out.append(([bits(det.read_level(f, i)) for i in range(len(det.levels))], d.tobytes(), h.tobytes()))
    return out


def digest(snap):
    m = hashlib.sha256()
    for levels, d, h in snap:
        for lv in levels:
            m.update(lv.tobytes())
        m.update(d)
        m.update(h)
    return m.hexdigest()


def ingest_names(det, fn):
    """the ingest kernels option "profile" names for one call of fn()"""
    det.set_option("profile", 1)
    det.profile()
    fn()
    names = [n for n in det.profile() if n.startswith("k_ingest") or n in ("k_yuv_to_rgb8", "k_yuv420_to_rgb8", "k_resize_u8")]
    det.set_option("profile", 0)
    return sorted(set(names))


def main():
    from oracle import binding as ob
    for case in CASES:
        det = detector(case, ob)
        x = dev(built(case).buf)
        names = ingest_names(det, lambda: run_entry(det, case, x))
        print(case.id, digest(snapshot(det)), ",".join(names), flush=True)
        det.close()


if __name__ == "__main__":
    main()
