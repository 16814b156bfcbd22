"""acf_hip_read_tap on EVERY frame of a batch, not only frame 0 of a one-frame batch: each stage tap of each real scale and the raw
channels of each level against the oracle's chnsPyramid of that frame, bit for bit, for every kind of input plane set (1-plane gray
and orig, 3-plane luv passed through and converted, 5-plane image + M, O passed through and converted) and with the batch cut into
sub-batch children (option "streams") or not.  With five planes the first real scale's M and O came with the frame: nothing is
computed there, so those taps must be refused, not read from buffers nothing wrote (chnsCompute.cpp:265-269)."""
import numpy as np
import pytest

from acf_amd import capi, synth
from test_luvmo_input import _with_own_mo

pytestmark = pytest.mark.gpu

NF = 3

INPUTS = {
    # name: (H, W, frame kind, d_in, model kwargs)
    "gray1": (120, 160, "gray", 1, dict(name="FACE64", nApprox=3)),                       # FACE64: 1-plane gray, colour off; 2 real scales
    "orig1": (96, 128, "gray", 1, dict(name="TINY", colorSpace=capi.CS_ORIG, isLuv=0)),   # replicated to three planes
    "luv3_isluv": (120, 160, "luv", 3, dict(name="TINY")),                                # colour passes through
    "rgb3_to_luv": (112, 144, "rgb", 3, dict(name="TINY", isLuv=0)),                      # colour converted
    "luv5_isluv": (120, 160, "luv", 5, dict(name="TINY")),                                # the caller's frames are the image taps
    "rgb5_to_luv": (96, 128, "rgb", 5, dict(name="TINY", isLuv=0)),
}

MO_TAPS = (capi.TAP_M, capi.TAP_O, capi.TAP_S, capi.TAP_MNORM)


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def make_frames(oracle, model, H, W, kind, d_in):
    """NF distinct frames; five-plane frames as tests/test_luvmo_input.py makes them: frame 0 with its own M, O, frames 1 and 2
    with M, O that differ from the image's (another frame's magnitude, scaled; a shifted orientation)."""
    frames = []
    for f in range(NF):
        frame = synth.make_frame(31 + f, H, W, kind)
        if d_in == 5:
            _, frame = _with_own_mo(oracle, model, frame, H, W)
            if f:
                frame[3] = np.roll(frame[3], 7 * f, axis=0) * np.float32(1.0 + 0.25 * f)
                frame[4] = np.roll(frame[4], 5 * f, axis=1)
        frames.append(frame)
    return np.stack(frames)


@pytest.mark.parametrize("streams", [1, 2])
@pytest.mark.parametrize("name", list(INPUTS))
def test_every_tap_of_every_frame_equals_the_oracle(oracle, name, streams):
    import torch
    from acf_amd.detector import HipDetector, HipError
    H, W, kind, d_in, kw = INPUTS[name]
    model = synth.make_model(seed=3, nTrees=16, **kw)
    frames = make_frames(oracle, model, H, W, kind, d_in)
    plan = oracle.Plan(model, H, W, d_in)
    det = HipDetector(model, H, W, d_in, max_batch=NF, max_hits=1 << 14, taps=True, streams=streams)
    det.run(torch.from_numpy(frames).cuda())
    d = 1 if model["colorSpace"] == capi.CS_GRAY else 3
    for f in range(NF):
        _, taps, chns = oracle.chns_pyramid(plan, frames[f], want_taps=True, want_chns=True)
        for k in range(len(plan.real)):
            t = taps[k]
            w1, h1 = t["M"].shape
            for tname, tap, shape in (("image", capi.TAP_IMAGE, (d, w1, h1)), ("smoothed", capi.TAP_SMOOTHED, (d, w1, h1)),
                                      ("M", capi.TAP_M, (w1, h1)), ("O", capi.TAP_O, (w1, h1)), ("S", capi.TAP_S, (w1, h1)),
                                      ("Mnorm", capi.TAP_MNORM, (w1, h1))):
                where = (name, streams, "frame", f, "real scale", k, tname)
                if d_in == 5 and k == 0 and tap in MO_TAPS:
                    with pytest.raises(HipError) as e:
                        det.read_tap(f, tap, k, shape)
                    assert e.value.code == capi.E_INVALID, where
                    continue
                got = det.read_tap(f, tap, k, shape)
                assert np.any(got), where
                assert np.array_equal(bits(got), bits(t[tname])), where
        for i in range(plan.nScales):
            l = plan.levels[i]
            got = det.read_tap(f, capi.TAP_CHNS, i, (plan.nChns, l.wC, l.hC))
            assert np.any(got), (name, streams, f, "level", i)
            assert np.array_equal(bits(got), bits(chns[i])), (name, streams, f, "level", i)
    det.close()
