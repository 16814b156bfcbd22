"""YUV 4:2:0 (NV12 / NV21) video frames in the 8-bit and streaming entries, on the GPU (include/acf_hip.h "YUV 4:2:0 input").

The expected result of a YUV frame is the oracle's result on the R, G, B bytes the restated conversion gives (tests/yuv420_ref.py:
cvtColor(COLOR_YUV2RGB_NV12 / _NV21) from OpenCV's published source, parity with OpenCV's bits unpinned): acfo_ingest_u8 ->
chnsPyramid -> acfDetect, as tests/test_gpu_ingest.py does for the packed layouts.  Every comparison is an equality of bytes or of
uint32 views.
"""
import os
import subprocess
import sys

import numpy as np
import pytest

import yuv420_ref as yr
from acf_amd import capi, synth

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "yuv420_rgb.npz")


def bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def make_nv(seed, H, W, nv21=False, stride=0, chroma_offset=0, total=0):
    """A video-like NV12 / NV21 frame (flat uint8 buffer) from the synthetic RGB frame of `seed`."""
    rgb = synth.make_frame(seed, H, W, "rgb")                                              # [3][W][H]
    up = np.clip(np.rint(rgb.transpose(2, 1, 0) * 255.0), 0, 255).astype(np.uint8)        # [H][W][3]
    return yr.from_rgb(up, nv21, stride, chroma_offset, total)


def oracle_planar(oracle, rgb, H, W):
    """The oracle's image entry on tight RGB bytes [H][W][3] -> planar f32 [3][W][H]."""
    rgb = np.ascontiguousarray(rgb)
    out = oracle.aligned((3, W, H))
    oracle.lib().acfo_ingest_u8(rgb.ctypes.data, H, W, 3, 0, 1, 2, W * 3, oracle.F(out), 3)
    return out


def _det():
    from acf_amd.detector import HipDetector
    return HipDetector(synth.make_model(seed=3, name="TINY", nTrees=8), 96, 128, 3, max_batch=1)


# ---------------------------------------------------------------- the conversion alone: acf_hip_op_yuv420_to_rgb = restatement

def test_op_equals_the_frozen_fixture():
    det = _det()
    z = np.load(GOLDEN)
    for n in sorted({k.split("/")[0] for k in z.files}):
        rows, cols, nv21, stride, off = (int(x) for x in z[n + "/geom"])
        got = det.yuv420_to_rgb(z[n + "/frame"], rows, cols, capi.PIX_NV21 if nv21 else capi.PIX_NV12, stride, off)
        assert np.array_equal(got, z[n + "/rgb"]), n
    det.close()


@pytest.mark.parametrize("nv21", [False, True], ids=["nv12", "nv21"])
@pytest.mark.parametrize("rows,cols,stride,off", [(2, 2, 0, 0), (66, 130, 0, 0), (240, 320, 0, 0), (1080, 1920, 0, 0),
                                                  (66, 130, 192, 0), (66, 130, 131, 0), (240, 320, 320, 240 * 320 + 4096), (66, 130, 133, 66 * 133 + 7)])
def test_op_equals_the_restatement(rows, cols, stride, off, nv21):
    det = _det()
    buf = yr.random_frame(rows * 7 + cols + stride, rows, cols, nv21, stride, off)
    got = det.yuv420_to_rgb(buf, rows, cols, capi.PIX_NV21 if nv21 else capi.PIX_NV12, stride, off)
    assert np.array_equal(got, yr.nv_to_rgb(buf, rows, cols, nv21, stride, off))
    det.close()


def test_op_on_every_triple():
    """A 4096 x 4096 frame whose 2 x 2 blocks enumerate every (Y, U, V) once."""
    det = _det()
    buf = yr.all_triples_frame()
    got = det.yuv420_to_rgb(buf, 4096, 4096, capi.PIX_NV12)
    assert np.array_equal(got, yr.nv_to_rgb(buf, 4096, 4096))
    det.close()


# ---------------------------------------------------------------- run_u8(NV12 / NV21) against the oracle

YUV_CASES = [
    # name, H, W, nv21, row stride, chroma offset, frame stride, unaligned base, model kwargs, arith
    ("inria_luv", 240, 320, False, 0, 0, 0, 0, dict(name="INRIA", nTrees=128, cascThr=-2.5), 0),                # fused rgb2luv_sse body
    ("face64_gray", 120, 160, False, 0, 0, 0, 0, dict(name="FACE64", nTrees=128, cascThr=-4.0, minDs_h=32, minDs_w=32), 0),  # rgb2gray
    ("tiny_isluv", 96, 128, False, 0, 0, 0, 0, dict(name="TINY", nTrees=96, cascThr=-3.0), 0),                  # planes taken as they are
    ("inria_hsv", 120, 160, False, 0, 0, 0, 0, dict(name="INRIA", nTrees=64, cascThr=-3.0, nOctUp=0, colorSpace=capi.CS_HSV), 0),  # planar, then k_rgb2hsv
    ("inria_arith", 120, 160, False, 0, 0, 0, 0, dict(name="INRIA", nTrees=64, cascThr=-3.0, nOctUp=0), 1),     # the reference's rcpps bits
    ("ragged_tiles", 130, 174, False, 0, 0, 0, 0, dict(name="INRIA", nTrees=64, cascThr=-3.0, nOctUp=0), 0),    # 3 x 3 tiles, ragged edges, H % 4 == 2
    ("padded_layout", 130, 174, False, 192, 192 * 136, 192 * 208, 0, dict(name="INRIA", nTrees=64, cascThr=-3.0, nOctUp=0), 0),
    ("byte_loads", 130, 174, False, 175, 175 * 130 + 3, 0, 1, dict(name="INRIA", nTrees=64, cascThr=-3.0, nOctUp=0), 0),  # odd stride, odd base
    ("nv21", 240, 320, True, 0, 0, 0, 0, dict(name="INRIA", nTrees=128, cascThr=-2.5), 0),
    ("nv21_padded", 130, 174, True, 176, 176 * 132, 0, 0, dict(name="INRIA", nTrees=64, cascThr=-3.0, nOctUp=0), 0),
    # the other two conversions of the shared store phase on 3 x 3 ragged tiles (a ragged width of 6: not a multiple of 16), through both load forms
    ("gray_bytes_ragged", 130, 134, False, 135, 135 * 130 + 3, 0, 1, dict(name="FACE64", nTrees=128, cascThr=-4.0, minDs_h=32, minDs_w=32), 0),  # H % 4 == 2
    ("isluv_bytes_ragged", 132, 134, False, 135, 135 * 132 + 3, 0, 1, dict(name="TINY", nTrees=96, cascThr=-3.0), 0),       # H % 4 == 0: float4 stores
    ("gray_dwords_ragged", 132, 134, False, 136, 0, 0, 0, dict(name="FACE64", nTrees=128, cascThr=-4.0, minDs_h=32, minDs_w=32), 0),
    ("isluv_dwords_ragged", 130, 134, False, 136, 0, 0, 0, dict(name="TINY", nTrees=96, cascThr=-3.0), 0),
]


def case_batch(case, nF=3):
    """-> (flat uint8 batch buffer incl. `base` leading bytes, frame stride, per-frame RGB [H][W][3] of the restatement)."""
    name, H, W, nv21, stride, off, fs, base, kw, arith = case
    per = fs or yr.frame_bytes(H, W, stride, off)
    buf = np.full(base + per * nF, 0x5A, np.uint8)
    rgbs = []
    for f in range(nF):
        fr = make_nv(30 + f, H, W, nv21, stride, off)
        buf[base + f * per: base + f * per + fr.size] = fr
        rgbs.append(yr.nv_to_rgb(fr, H, W, nv21, stride, off))
    return buf, per, rgbs


def oracle_expect(oracle, model, rgbs, H, W, arith=0):
    """-> per frame (plan, pyramid, detections, hits) of the oracle on the restated RGB bytes."""
    plan = oracle.Plan(model, H, W, 3)
    out = []
    if arith:
        oracle.set_x86_tables(*oracle.x86_fixture())
        oracle.set_approx(3)
    try:
        for rgb in rgbs:
            pyr, _, _ = oracle.chns_pyramid(plan, oracle_planar(oracle, rgb, H, W))
            want, want_hits = oracle.detect(plan, pyr)
            out.append((plan, pyr, want, want_hits))
    finally:
        if arith:
            oracle.set_approx(0)
    return out


@pytest.mark.parametrize("case", YUV_CASES, ids=[c[0] for c in YUV_CASES])
def test_run_u8_yuv_bit_exact(oracle, case):
    import torch
    from acf_amd.detector import HipDetector
    name, H, W, nv21, stride, off, fs, base, kw, arith = case
    pix = capi.PIX_NV21 if nv21 else capi.PIX_NV12
    model = synth.make_model(seed=3, **kw)
    nF = 3
    buf, per, rgbs = case_batch(case, nF)
    det = HipDetector(model, H, W, 3, max_batch=nF, max_hits=1 << 16)
    if arith:
        det.set_x86_tables(*oracle.x86_fixture())
        det.set_option("arith", 1)
    if off or fs:
        det.set_yuv_layout(off, fs)
    dev = torch.from_numpy(buf).cuda()
    det.run_u8(dev.data_ptr() + base, pix, stride, n=nF)
    total = 0
    for f, (plan, pyr, want, want_hits) in enumerate(oracle_expect(oracle, model, rgbs, H, W, arith)):
        for i in range(plan.nScales):
            assert np.array_equal(bits(det.read_level(f, i)), bits(plan.level_view(pyr, i))), (name, f, "level", i)
        got, got_hits = det.detections(f)
        assert len(got) == len(want)
        assert got.tobytes() == want.tobytes() and got_hits.tobytes() == want_hits.tobytes(), (name, f)
        total += len(want)
    assert total > 0, "no detections: the cascade comparison would be vacuous"
    det.close()


def test_yuv_and_restated_rgb_give_the_same_records_through_the_library():
    import torch
    from acf_amd.detector import HipDetector
    H, W, nF, cap = 240, 320, 3, 1024
    model = synth.make_model(seed=3, name="INRIA", nTrees=128, cascThr=-2.5)
    det = HipDetector(model, H, W, 3, max_batch=nF, max_hits=1 << 16)
    frames = [make_nv(50 + f, H, W) for f in range(nF)]
    recs = []
    for pix, batch in ((capi.PIX_NV12, np.stack(frames)), (capi.PIX_RGB, np.stack([yr.nv_to_rgb(fr, H, W) for fr in frames]))):
        det.run_u8(torch.from_numpy(batch).cuda(), pix)
        dst = torch.zeros((nF, 1 + 6 * cap), dtype=torch.int32, device="cuda")
        torch.cuda.synchronize()                                          # (torch fills dst on its own stream: before the export writes it)
        det.export_detections(dst, cap)
        det.synchronize()
        recs.append((dst.cpu().numpy(), [det.read_pyramid(f) for f in range(nF)]))
    (a, pa), (b, pb) = recs
    assert int(a[:, 0].sum()) > 0 and int(a[:, 0].max()) <= cap
    for f in range(nF):
        assert np.array_equal(bits(pa[f]), bits(pb[f])), f
        n = int(a[f, 0])
        assert np.array_equal(a[f, :1 + 6 * n], b[f, :1 + 6 * n]), f
    det.close()


# ---------------------------------------------------------------- the fused kernel against its fallback (one process each)

def _case(setting):
    env = dict(os.environ)
    if setting:
        k, v = setting.split("=", 1)
        env[k] = v
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "yuv420_case.py")], cwd=ROOT, env=env, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and r.stdout.strip().startswith("ok"), (setting, r.stdout[-1500:], r.stderr[-1500:])
    _, total, digest, kernels = r.stdout.strip().split()
    return int(total), digest, set(kernels.split(","))


def test_fused_kernel_and_unfused_fallback_agree_and_are_the_forms_named():
    total, digest, kernels = _case("")
    assert total > 0
    assert "k_ingest_yuv420" in kernels and "k_ingest_u8" not in kernels and "k_yuv420_to_rgb8" not in kernels, kernels
    total_fb, digest_fb, kernels_fb = _case("ACF_HIP_FORCE_FALLBACK=yuv_unfused")
    assert "k_ingest_yuv420" not in kernels_fb and "k_ingest_u8" in kernels_fb and "k_yuv420_to_rgb8" in kernels_fb, kernels_fb
    assert (total_fb, digest_fb) == (total, digest)


# ---------------------------------------------------------------- the input resize in front: convert -> resize -> ingest

@pytest.mark.parametrize("min_width", [150, 64], ids=["reduce", "enlarge"])
def test_input_resize_of_yuv_equals_input_resize_of_the_restated_rgb(oracle, min_width):
    import torch
    from acf_amd.detector import HipDetector
    H, W, nF = 240, 320, 2
    model = synth.make_model(seed=3, name="FACE80", nTrees=64, cascThr=-4.0)
    scale = HipDetector.resize_scale(model["modelDs_w"], min_width)
    assert (scale < 1) == (min_width == 150)
    dr, dc = HipDetector.resize_dims(H, W, scale)
    det = HipDetector(model, dr, dc, 3, max_batch=nF, max_hits=1 << 17)
    det.set_input_resize(H, W, scale)
    frames = [make_nv(80 + f, H, W) for f in range(nF)]
    rgbs = [yr.nv_to_rgb(fr, H, W) for fr in frames]
    got = []
    for pix, batch in ((capi.PIX_NV12, np.stack(frames)), (capi.PIX_RGB, np.stack(rgbs))):
        det.run_u8(torch.from_numpy(batch).cuda(), pix)
        got.append([(det.read_pyramid(f),) + det.detections(f) for f in range(nF)])
    plan = oracle.Plan(model, dr, dc, 3)
    total = 0
    for f in range(nF):
        (pa, da, ha), (pb, db, hb) = got[0][f], got[1][f]
        assert np.array_equal(bits(pa), bits(pb)) and da.tobytes() == db.tobytes() and ha.tobytes() == hb.tobytes(), f
        # and against the oracle's resize + entry + pyramid, so that the pair above is not self-referential
        red = oracle.resize_u8(rgbs[f], scale)
        pyr, _, _ = oracle.chns_pyramid(plan, oracle_planar(oracle, red, dr, dc))
        want, _ = oracle.detect(plan, pyr)
        assert np.array_equal(bits(pa), bits(pyr)) and da.tobytes() == want.tobytes(), f
        total += len(want)
    assert total > 0
    det.close()


# ---------------------------------------------------------------- streaming

@pytest.mark.parametrize("depth", [2, 3])
def test_stream_of_yuv_frames_matches_blocking_calls(oracle, depth):
    """Five NV12 batches (one short) through submit / collect give the records of run_u8 + export of each batch."""
    import torch
    from acf_amd.detector import HipDetector, PinnedBuffer
    H, W, pix, cap, nB = 120, 160, capi.PIX_NV12, 512, 4
    model = synth.make_model(seed=3, name="INRIA", nTrees=64, cascThr=-3.0, nOctUp=0)
    det = HipDetector(model, H, W, 3, max_batch=nB, max_hits=4096)
    per = HipDetector.u8_frame_bytes(pix, H, W)
    assert per == H * W * 3 // 2
    batches = []
    for b in range(5):
        n = nB if b != 3 else 2
        batches.append(np.stack([make_nv(100 + 10 * b + i, H, W) for i in range(n)]))
    want = []
    for x in batches:
        det.run_u8(torch.from_numpy(x).cuda(), pix)
        dst = torch.zeros((x.shape[0], 1 + 6 * cap), dtype=torch.int32, device="cuda")
        torch.cuda.synchronize()                                          # (torch fills dst on its own stream: before the export writes it)
        det.export_detections(dst, cap)
        det.synchronize()
        want.append(dst.cpu().numpy())
    assert sum(int(w[:, 0].sum()) for w in want) > 0
    # the first frame against the oracle, so that the reference above is not self-referential
    (_, _, odet, _), = oracle_expect(oracle, model, [yr.nv_to_rgb(batches[0][0], H, W)], H, W)
    assert want[0][0, 0] == len(odet) > 0
    assert np.array_equal(want[0][0, 1:1 + 6 * len(odet)].reshape(-1, 6)[:, 4].view(np.uint32), bits(odet["score"]))

    pins = [PinnedBuffer(nB * per) for _ in range(depth)]
    det.stream_open(pix, 0, cap, depth)
    got, inflight = [], []
    for b, x in enumerate(batches):
        if len(inflight) == depth:
            got.append(det.stream_collect(inflight.pop(0)))
        pin = pins[b % depth]
        pin.array[:x.size] = x.ravel()
        inflight.append(det.stream_submit(pin.ptr.value, x.shape[0]))
    while inflight:
        got.append(det.stream_collect(inflight.pop(0)))
    for b in range(5):
        assert got[b].shape == want[b].shape, b
        for f in range(want[b].shape[0]):
            n = want[b][f, 0]
            assert got[b][f, 0] == n
            assert np.array_equal(got[b][f, :1 + 6 * n], want[b][f, :1 + 6 * n]), (b, f)
    det.stream_close()
    det.close()
    for p in pins:
        p.close()


# ---------------------------------------------------------------- what is refused

def test_yuv_argument_checks():
    import torch
    from acf_amd.detector import HipDetector, HipError
    model = synth.make_model(seed=3, name="TINY", nTrees=16)
    x = torch.zeros(4 * 128 * 128 * 3, dtype=torch.uint8).cuda()      # room for every call below, were it not refused

    def refused(fn):
        with pytest.raises(HipError) as e:
            fn()
        assert e.value.code == capi.E_INVALID, e.value
    for H, W in ((97, 128), (96, 127)):                                # odd H, odd W
        det = HipDetector(model, H, W, 3, max_batch=1)
        refused(lambda: det.run_u8(x, capi.PIX_NV12, n=1))
        refused(lambda: det.stream_open(capi.PIX_NV12, 0, 64, 2))
        det.close()
    g = HipDetector(synth.make_model(seed=3, name="FACE64", nTrees=16), 96, 128, 1, max_batch=1)   # a d = 1 plan
    refused(lambda: g.run_u8(x, capi.PIX_NV12, n=1))
    refused(lambda: g.stream_open(capi.PIX_NV21, 0, 64, 2))
    g.close()
    det = HipDetector(model, 96, 128, 3, max_batch=2)
    refused(lambda: det.run_u8(x, capi.PIX_NV12, row_stride=120, n=1))           # stride < W
    refused(lambda: det.run_u8(x, 9, n=1))                                        # layout 9
    refused(lambda: det.run_u8(x, 7, n=1))
    det.set_yuv_layout(96 * 128 - 128, 0)                                         # chroma offset inside the luma plane
    refused(lambda: det.run_u8(x, capi.PIX_NV12, n=1))
    refused(lambda: det.stream_open(capi.PIX_NV12, 0, 64, 2))
    det.set_yuv_layout(96 * 160, 0)                                               # ... fine for stride 128, inside the plane for stride 192
    det.run_u8(x, capi.PIX_NV12, row_stride=128, n=1)
    refused(lambda: det.run_u8(x, capi.PIX_NV12, row_stride=192, n=1))
    det.set_yuv_layout(0, 96 * 128 * 3 // 2 - 2)                                  # frames would overlap
    refused(lambda: det.run_u8(x, capi.PIX_NV12, n=2))
    refused(lambda: det.stream_open(capi.PIX_NV21, 0, 64, 2))
    refused(lambda: det.set_yuv_layout(-4, 0))
    det.set_yuv_layout(0, 0)
    det.run_u8(x, capi.PIX_NV12, n=2)                                             # tight again: accepted
    det.run_u8(x, capi.PIX_RGB, n=2)                                              # the packed layouts are untouched by the layout call
    # the input resize on: the unreduced frame must be even
    sc = 0.5
    small = HipDetector(model, *HipDetector.resize_dims(191, 256, sc), 3, max_batch=1)
    small.set_input_resize(191, 256, sc)
    refused(lambda: small.run_u8(x, capi.PIX_NV12, n=1))
    small.close()
    # the operator entry
    refused(lambda: det.yuv420_to_rgb(np.zeros(64, np.uint8), 4, 4, capi.PIX_RGB))
    refused(lambda: det.yuv420_to_rgb(np.zeros(64, np.uint8), 3, 4, capi.PIX_NV12))
    refused(lambda: det.yuv420_to_rgb(np.zeros(64, np.uint8), 4, 4, capi.PIX_NV12, row_stride=3))
    refused(lambda: det.yuv420_to_rgb(np.zeros(64, np.uint8), 4, 4, capi.PIX_NV12, chroma_offset=12))
    det.close()


# ---------------------------------------------------------------- the C++ host

@pytest.mark.parametrize("mode", [[], ["--stream", "2"]], ids=["image", "stream"])
def test_cli_nv12_matches_the_python_path(oracle, tmp_path, mode):
    """acf::HipDetector::operator()(packed, ..., ACF_HIP_PIX_NV12) and streamOpen / streamSubmit through the CLI."""
    import torch
    from acf_amd.detector import HipDetector
    from acf_amd.modelio import write_model
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    from test_host_cpp import parse, run
    host = os.path.join(ROOT, "acf_amd", "host")
    subprocess.check_call(["make", "-s", "-C", host])
    H, W, cnt = 120, 160, 5
    model = synth.make_model(seed=3, name="INRIA", nTrees=64, cascThr=-3.0, nOctUp=0)
    write_model(str(tmp_path / "m.acfm"), model)
    frames = np.stack([make_nv(60 + i, H, W) for i in range(cnt)])
    (tmp_path / "f.nv12").write_bytes(frames.tobytes())
    p = run(os.path.join(host, "acf_hip_detect"), ["--model", str(tmp_path / "m.acfm"), "--frames", str(tmp_path / "f.nv12"), "--u8", "nv12",
                                                   "--rows", str(H), "--cols", str(W), "--count", str(cnt)] + mode)
    got = parse(p.stdout)
    det = HipDetector(model, H, W, 3, max_batch=cnt, max_hits=1 << 16)
    det.run_u8(torch.from_numpy(frames).cuda(), capi.PIX_NV12)
    expect = oracle_expect(oracle, model, [yr.nv_to_rgb(fr, H, W) for fr in frames], H, W)
    total = 0
    for f in range(cnt):
        d, _ = det.detections(f)
        py = [(int(r["x"]), int(r["y"]), int(r["w"]), int(r["h"]), int(np.float32(r["score"]).view(np.uint32))) for r in d]
        assert got[f] == py, f
        assert d.tobytes() == expect[f][2].tobytes(), f
        total += len(py)
    assert total > 0
    det.close()
