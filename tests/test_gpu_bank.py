"""A bank of classifiers on one pyramid, on the GPU (include/acf_hip.h: acf_hip_set_bank, acf_hip_detect_bank, acf_hip_join_bank,
acf_hip_op_join_bank; kernel k_join_bank).  Every comparison is of raw bytes:
  1. every designed case of tests/bank_ref.py through acf_hip_op_join_bank, on outputs pre-filled with a sentinel byte, against the numpy
     restatement of the header's rule; the refusals of a bad spec;
  2. the pipeline case: after run + detect_bank every member's detections and hits against the CPU oracle (the member's plan on the
     primary's pyramid) and against a context that holds the member as its only model, under the default options, rank_cells = 0 and
     cascade_tiles = 0, the form of every member's cascade read from acf_hip_get_bank_forms; the primary's lists untouched;
  3. join_bank for types 0 / 1 / 2 x separate 0 / 1 against the restatement fed with the device lists, then acf_hip_cut_crops on
     boxes_out / frames_out against the host route;
  4. state: a second, smaller batch; the bank after run_u8 and after run_view; the device NMS on the primary; a list over max_hits;
  5. lifecycle and refusals, a captured graph, the profile names, device memory over re-plans.
tests/test_bank.py holds the preconditions: the oracle's counts of the pipeline case and the restatement against the oracle's bbNms."""
import ctypes as C

import numpy as np
import pytest

import bank_ref as br
from acf_amd import capi, synth
from acf_amd.detector import HipDetector, HipError

pytestmark = pytest.mark.gpu
F = np.float32
NAMES = ("records", "counts", "boxes", "frame indices")


def dev(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def assert_bytes(got, want, tag):
    for name, g, w in zip(NAMES, got, want):
        g, w = np.ascontiguousarray(g), np.ascontiguousarray(w)
        assert g.shape == w.shape, (tag, name, g.shape, w.shape)
        if g.tobytes() != w.tobytes():
            bad = np.flatnonzero(g.view(np.uint8).ravel() != w.view(np.uint8).ravel())
            raise AssertionError((tag, name, "bytes that differ", len(bad), "first at", int(bad[0]), "counts", list(np.ravel(got[1])), list(np.ravel(want[1]))))


def lists_of(det, model, n):
    return [(det.bank_detections(model, f), det.bank_hits(model, f)) for f in range(n)]


def same_lists(got, want, tag):
    assert len(got) == len(want), tag
    for f, ((gd, gh), (wd, wh)) in enumerate(zip(got, want)):
        assert len(gd) == len(wd) and gd.tobytes() == wd.tobytes() and gh.tobytes() == wh.tobytes(), (tag, "frame", f, len(gd), len(wd))


def as_u8(frames):
    """planar float frames [n][3][W][H] in [0, 1] as packed 8-bit frames [n][H][W][3]"""
    return np.ascontiguousarray((np.clip(frames, 0, 1) * 255 + 0.5).astype(np.uint8).transpose(0, 3, 2, 1))


def form_of(rec):
    """(path, rank cells, tile kernel) of a cascade record: rank = tile kernel on rank cells, float-tile = a tile kernel on floats,
    staged = no tile kernel"""
    return rec["path"], rec["rank"], rec["kernel"]


# ---------------------------------------------------------------- 1. the designed cases through the op entry

@pytest.fixture(scope="module")
def bare():
    det = HipDetector()                                                                       # a context: no model, no plan
    yield det
    det.close()


@pytest.mark.parametrize("name", list(br.cases()))
def test_designed_case_equals_the_restatement(bare, name):
    c = br.cases()[name]
    got = bare.op_join_bank(c["dets"], c["counts"], c["nms"], c.get("separate", 0), c.get("k", 8), c.get("grow", 1.0), c.get("det_scale"), fill=br.FILL)
    assert_bytes(got, br.expected(name), name)


def test_bad_specs_and_arguments_are_refused_and_optional_outputs_may_be_null(bare):
    c = br.cases()["two models"]
    want = br.expected("two models")
    dets, counts = np.ascontiguousarray(c["dets"]), np.ascontiguousarray(c["counts"], np.int32)
    k = c["k"]
    rec, cnt = np.full((1, k, 32), br.FILL, np.uint8), np.zeros(1, np.int32)
    p = lambda a: C.c_void_p(a.ctypes.data) if a is not None else None
    good = br.spec_of(k=k)
    op = lambda d=dets, cn=counts, nm=2, nf=1, mh=dets.shape[2], spec=good, out=rec, co=cnt: bare.lib.acf_hip_op_join_bank(
        bare.ctx, p(d), p(cn), nm, nf, mh, C.byref(spec) if spec else None, p(out), p(co), None, None)
    pipe = lambda spec=good, out=rec, co=cnt: bare.lib.acf_hip_join_bank(bare.ctx, C.byref(spec) if spec else None, p(out), p(co), None, None)
    assert op() == 0 and rec.tobytes() == want[0].tobytes() and cnt.tolist() == want[1].tolist()
    for fn in (op, pipe):
        for kw in (dict(out=None), dict(co=None), dict(spec=None)):
            assert fn(**kw) == capi.E_INVALID, kw
        for kw in br.BAD_SPECS:
            assert fn(spec=br.spec_of(**kw)) == capi.E_INVALID, kw
    for kw in (dict(d=None), dict(cn=None), dict(mh=0), dict(nm=0), dict(nm=capi.BANK_MAX + 2), dict(nf=0)):
        assert op(**kw) == capi.E_INVALID, kw
    assert pipe() == capi.E_INVALID and b"acf_hip_detect_bank first" in bare.lib.acf_hip_last_error(bare.ctx)   # good arguments: only the lists are missing
    assert bare.lib.acf_hip_detect_bank(bare.ctx) == capi.E_INVALID and b"no bank" in bare.lib.acf_hip_last_error(bare.ctx)
    prm, keep = capi.make_params(br.models()[1])
    assert bare.lib.acf_hip_set_bank(bare.ctx, C.byref(prm), 1) == capi.E_NOMODEL             # a bank needs a model
    assert op() == 0                                                                          # the context still works


# ---------------------------------------------------------------- 2. the pipeline case

@pytest.fixture(scope="module")
def pipe():
    m = br.models()
    det = HipDetector(m[0])
    det.set_bank(m[1:])
    det.plan(br.H, br.W, br.D, max_batch=2, max_hits=br.MAX_HITS)
    solo = [HipDetector(mm, br.H, br.W, br.D, max_batch=2, max_hits=br.MAX_HITS) for mm in m]   # one context per model: the way of before
    yield det, solo, dev(br.frames())
    for d in [det] + solo:
        d.close()


def test_plan_builds_every_members_window_grid(pipe, oracle):
    det, solo, _ = pipe
    for i, m in enumerate(br.models()):
        plan = oracle.Plan(m, br.H, br.W, br.D)
        got = det.bank_levels(i)
        assert len(got) == plan.nScales == len(solo[i].levels)
        for a, b, c in zip(got, solo[i].levels, plan.levels):
            assert bytes(a) == bytes(b), (i, a.nWinR, b.nWinR)
            assert all(getattr(a, t) == getattr(c, t) for t in ("hP", "wP", "nWinR", "nWinC", "offset")), (i, a.nWinR, c.nWinR)
    assert [(l.nWinR, l.nWinC) for l in det.bank_levels(4)][12:] == [(3, 0), (2, 0), (1, 0), (0, 0), (0, 0)]   # levels smaller than the wide window
    with pytest.raises(HipError):
        det.bank_levels(5)


@pytest.mark.parametrize("options", [{}, dict(rank_cells=0), dict(cascade_tiles=0)], ids=["default", "rank_cells 0", "cascade_tiles 0"])
def test_members_equal_the_oracle_and_a_context_of_their_own(pipe, options):
    det, solo, fr = pipe
    want = br.oracle_lists()
    for d in [det] + solo:
        for k, v in options.items():
            d.set_option(k, v)
    try:
        det.run(fr)
        det.synchronize()
        before = [(det.detections(f), det.raw_detections(f)) for f in range(2)]
        det.detect_bank()
        forms = []
        for i in range(1, 5):
            got = lists_of(det, i, 2)
            assert tuple(len(g[0]) for g in got) == br.RAW_COUNTS[i]
            same_lists(got, want[i], (options, br.NAMES[i], "oracle"))
            solo[i].run(fr)
            same_lists(got, [solo[i].detections(f) for f in range(2)], (options, br.NAMES[i], "a context of its own"))
            rec, own = det.bank_forms(i), solo[i].cascade_forms()
            assert rec["frames"] == 2 and form_of(rec) == form_of(own), (options, br.NAMES[i], rec, own)
            forms.append(form_of(rec))
        # what the member and the options admit: rank cells for the depth-2 members on whole-cell strides, floats for the child walk
        # (depth 0) and for stride < shrink; no tile kernel with cascade_tiles = 0; float tiles with rank_cells = 0
        tiles, rank = options.get("cascade_tiles", 1), options.get("rank_cells", 1)
        depth2 = ("tiled2", bool(rank), "tile3") if tiles else ("staged", False, None)
        assert forms[0] == depth2 and forms[3] == depth2, (options, forms)
        assert forms[1] == ("staged", False, None) and forms[2][0] == "staged" and not forms[2][1], (options, forms)
        # the primary: untouched by detect_bank, and what a context without a bank gives
        after = [(det.detections(f), det.raw_detections(f)) for f in range(2)]
        solo[0].run(fr)
        for f in range(2):
            assert before[f][0][0].tobytes() == after[f][0][0].tobytes() and before[f][0][1].tobytes() == after[f][0][1].tobytes()
            assert before[f][1].tobytes() == after[f][1].tobytes() == solo[0].raw_detections(f).tobytes() == want[0][f][0].tobytes()
            assert det.bank_detections(0, f).tobytes() == want[0][f][0].tobytes() and det.bank_hits(0, f).tobytes() == want[0][f][1].tobytes()
    finally:
        for d in [det] + solo:
            for k in options:
                d.set_option(k, 1)


# ---------------------------------------------------------------- 3. the join on the device lists

def test_join_equals_the_restatement_and_feeds_cut_crops(pipe):
    import torch
    det, _, fr = pipe
    det.run(fr)
    det.detect_bank()
    det.synchronize()
    lists = [[det.bank_detections(m, f) for f in range(2)] for m in range(5)]
    assert tuple(tuple(len(l) for l in ll) for ll in lists) == br.RAW_COUNTS
    dets, counts = br.lists_to_arrays(lists, br.MAX_HITS)
    x = dev(np.random.RandomState(5).randint(0, 256, (2, br.H, br.W, 3)).astype(np.uint8))        # the stored frames the crops are cut from
    src = det.crop_source_tensor(x, layout="nhwc")
    k = 200
    for typ, ovr, overlap in ((None, None, None), ("max", "min", 0.65), ("maxg", "union", 0.5)):
        for sep in (0, 1):
            q = None if typ is None else br.nms_of(typ, ovr=ovr, overlap=overlap)
            grow, scale = (1.0, None) if typ != "maxg" else (1.25, 0.8)
            rec, cnt, boxes, fidx = det.join_bank(q, sep, k, grow, scale)
            det.synchronize()
            want = list(br.join(dets, counts, q, sep, k, grow, scale, fill=0))
            got = [rec.cpu().numpy().view(capi.BANK_DTYPE).reshape(2, k).copy(), cnt.cpu().numpy(), boxes.cpu().numpy(), fidx.cpu().numpy()]
            for f in range(2):                                                                # record slots beyond the count are undefined here
                m = max(min(int(want[1][f]), k), 0)
                got[0][f, m:] = want[0][f, m:]
            assert_bytes(got, want, (typ, sep))
            if typ is not None:
                assert tuple(got[1]) == br.JOINT_KEPT[(typ, ovr, overlap)][sep]
            else:
                assert got[1].tolist() == [715, 629]
            if typ != "maxg":
                continue
            # the device-only route to crops against the host's: crop_box on the restatement's survivors
            crops = det.cut_crops(src, boxes.view(-1, 4), fidx.view(-1), (20, 16), samples=2)
            hb, hf = np.zeros((2, k, 4), F), np.full((2, k), -1, np.int32)
            for f in range(2):
                for s in range(min(int(want[1][f]), k)):
                    r = want[0][f, s]
                    d = lists[r["model"]][f][r["index"]]
                    hb[f, s], hf[f, s] = HipDetector.crop_box([int(d[t]) for t in ("x", "y", "w", "h")], scale, grow), f
            assert np.array_equal(hb.view(np.uint32), got[2].view(np.uint32)) and np.array_equal(hf, got[3])
            want_crops = det.cut_crops(src, hb.reshape(-1, 4), hf.reshape(-1), (20, 16), samples=2)
            det.synchronize()
            gc, wc = crops.cpu().numpy(), want_crops.cpu().numpy()
            assert gc.tobytes() == wc.tobytes()
            for f in range(2):
                m = min(int(got[1][f]), k)
                assert gc[f * k:f * k + m].any() and not gc[f * k + m:(f + 1) * k].any()


# ---------------------------------------------------------------- 4. state

def test_a_second_smaller_batch_and_the_device_nms_on_the_primary(pipe):
    det, _, fr = pipe
    det.run(fr)
    det.detect_bank()
    seeds = (43,)
    want = br.oracle_lists(seeds)
    det.run(dev(br.frames(seeds)))
    with pytest.raises(HipError) as e:                                                        # a new pyramid: the lists of the bank are the last batch's
        det.join_bank(None, 0, 8)
    assert e.value.code == capi.E_INVALID
    with pytest.raises(HipError):
        det.bank_detections(1, 0)
    det.detect_bank()
    for i in range(1, 5):
        same_lists(lists_of(det, i, 1), want[i], ("second batch", br.NAMES[i]))
        with pytest.raises(HipError):
            det.bank_detections(i, 1)                                                         # outside the batch
    rec, cnt, _, _ = det.join_bank(None, 0, 8)
    assert cnt.shape[0] == 1 and int(cnt.cpu()[0]) == sum(len(want[m][0][0]) for m in range(5)) > 0
    # device NMS on the primary: detections() are its survivors, the join still takes the raw list
    det.set_nms(capi.make_nms("maxg", overlap=0.3, ovrDnm="union"))
    try:
        det.run(fr)
        det.detect_bank()
        det.synchronize()
        assert len(det.detections(0)[0]) < len(det.raw_detections(0)) == br.RAW_COUNTS[0][0]
        rec, cnt, _, _ = det.join_bank(None, 0, 400)
        rec = rec.cpu().numpy().view(capi.BANK_DTYPE).reshape(2, 400)
        assert cnt.cpu().numpy().tolist() == [715, 629]
        n0 = br.RAW_COUNTS[0][0]
        assert (rec[0, :n0]["model"] == 0).all() and rec[0, n0]["model"] == 1
        raw = det.raw_detections(0)
        assert all(rec[0, :n0][t].tobytes() == raw[t].tobytes() for t in ("x", "y", "w", "h", "score", "scale"))
    finally:
        det.set_nms(None)


def test_the_bank_after_run_u8_and_after_run_view(pipe):
    det, solo, _ = pipe
    x = dev(as_u8(br.frames()))
    det.run_u8(x)
    det.detect_bank()
    for i in (1, 3):
        solo[i].run_u8(x)
        want = [solo[i].detections(f) for f in range(2)]
        same_lists(lists_of(det, i, 2), want, ("run_u8", br.NAMES[i]))
        assert sum(len(w[0]) for w in want) > 0
    big = dev(as_u8(synth.make_frame(44, 150, 170, "luv")[None]))
    views = np.stack([HipDetector.view_from_box((10, 12, 128, 96), 0.1, br.H, br.W), HipDetector.view_from_box((30, 20, 96, 72), -0.2, br.H, br.W)])
    frames = np.zeros(2, np.int32)
    dv, df = dev(views), dev(frames)
    det.run_view(det.crop_source_tensor(big, layout="nhwc"), dv, df, 2)
    det.detect_bank()
    for i in (2, 4):
        solo[i].run_view(solo[i].crop_source_tensor(big, layout="nhwc"), dv, df, 2)
        want = [solo[i].detections(f) for f in range(2)]
        same_lists(lists_of(det, i, 2), want, ("run_view", br.NAMES[i]))
        assert sum(len(w[0]) for w in want) > 0


def test_a_list_over_max_hits_reports_its_count_and_the_frame_joins_to_minus_one():
    m = br.models()
    det = HipDetector(m[0])
    det.set_bank([m[3]])                                                                      # deep: 246 / 80 raw detections
    det.plan(br.H, br.W, br.D, max_batch=2, max_hits=330)                                      # the primary's 192 / 319 fit
    det.run(dev(br.frames()))
    det.detect_bank()
    assert len(det.bank_detections(1, 1)) == 80
    n = C.c_int()
    out = (capi.Detection * 330)()
    assert det.lib.acf_hip_get_bank_detections(det.ctx, 1, 0, out, 330, C.byref(n)) == capi.OK and n.value == 246
    det.close()
    det = HipDetector(m[0])
    det.set_bank([m[3]])
    det.plan(br.H, br.W, br.D, max_batch=2, max_hits=245)                                      # deep overflows on frame 0, the primary on frame 1
    det.run(dev(br.frames()))
    det.detect_bank()
    assert det.lib.acf_hip_get_bank_detections(det.ctx, 1, 0, out, 245, C.byref(n)) == capi.E_CAPACITY and n.value == 246   # the true count
    assert det.lib.acf_hip_get_bank_detections(det.ctx, 0, 1, out, 245, C.byref(n)) == capi.E_CAPACITY and n.value == 319
    rec, cnt, boxes, fidx = det.join_bank(br.nms_of(), 0, 16)
    assert cnt.cpu().numpy().tolist() == [-1, -1] and not boxes.cpu().numpy().any() and (fidx.cpu().numpy() == -1).all()
    det.close()


# ---------------------------------------------------------------- 5. lifecycle, refusals, a graph, the profile, memory

def test_lifecycle_and_refusals():
    m = br.models()
    fr = dev(br.frames())
    det = HipDetector(m[0], br.H, br.W, br.D, max_batch=2, max_hits=br.MAX_HITS)

    def refused(fn, *a):
        with pytest.raises(HipError) as e:
            fn(*a)
        return e.value.code, str(e.value)
    det.run(fr)
    assert refused(det.detect_bank)[0] == capi.E_INVALID                                      # no bank
    det.set_bank(m[1:3])
    assert refused(det.run, fr)[0] == capi.E_NOPLAN                                           # set_bank dropped the plan
    assert refused(det.detect_bank)[0] == capi.E_INVALID
    det.plan(br.H, br.W, br.D, max_batch=2, max_hits=br.MAX_HITS)
    code, text = refused(det.detect_bank)
    assert code == capi.E_INVALID and "no pyramid" in text
    det.pyramid(fr)
    det.detect_bank()                                                                         # after a pyramid alone
    assert len(det.bank_detections(1, 0)) == br.RAW_COUNTS[1][0]
    assert refused(det.join_bank, None, 0, 8)[0] == capi.E_INVALID                            # the primary has no list yet
    det.detect()
    det.join_bank(None, 0, 8)
    det.run(fr)
    assert refused(det.join_bank, None, 0, 8)[0] == capi.E_INVALID                            # no detect_bank since the last pyramid
    bad = dict(m[1], shrink=2)
    assert refused(det.set_bank, [m[2], bad])[0] == capi.E_INVALID and "member 1" in refused(det.set_bank, [m[2], bad])[1]
    det.detect_bank()                                                                         # a refused bank left the context as it was
    assert len(det.bank_detections(2, 1)) == br.RAW_COUNTS[2][1]
    assert refused(det.set_bank, list(m[1:]) * 3)[0] == capi.E_INVALID                        # more than ACF_HIP_BANK_MAX
    det.set_model(m[0])                                                                       # clears the bank
    det.plan(br.H, br.W, br.D, max_batch=2, max_hits=br.MAX_HITS)
    det.run(fr)
    code, text = refused(det.detect_bank)
    assert code == capi.E_INVALID and "no bank" in text
    det.set_bank(m[1:2])
    det.set_bank([])                                                                          # n = 0 clears it as well
    det.plan(br.H, br.W, br.D, max_batch=2, max_hits=br.MAX_HITS)
    det.run(fr)
    assert "no bank" in refused(det.detect_bank)[1]
    det.close()
    # an LDCF primary takes no bank
    det = HipDetector(synth.make_model(name="TINY", seed=9, nTrees=8, ldcfK=2))
    assert refused(det.set_bank, [m[1]])[0] == capi.E_UNSUPPORTED
    det.close()
    # option "streams" > 1
    det = HipDetector(m[0], streams=2)
    det.set_bank(m[1:2])
    det.plan(br.H, br.W, br.D, max_batch=4, max_hits=br.MAX_HITS)
    det.run(dev(np.concatenate([br.frames(), br.frames()])))
    assert refused(det.detect_bank)[0] == capi.E_UNSUPPORTED
    det.close()


def test_without_the_float_pyramid_detect_bank_says_so():
    H, W = 200, 264
    model = synth.make_model(seed=3, name="TINY", nTrees=256, cascThr=-1.0)
    det = HipDetector(model)
    det.set_bank([synth.make_model(seed=4, name="TINY", nTrees=32, cascThr=-1.0)])
    det.plan(H, W, 3, max_batch=1, max_hits=1 << 15)
    det.set_option("keep_pyramid", 0)
    det.run(dev(synth.make_frame(11, H, W, "luv")[None]))
    with pytest.raises(HipError):
        det.read_level(0, 0)                                                                  # the primary ran on rank cells: no float pyramid
    with pytest.raises(HipError) as e:
        det.detect_bank()
    assert e.value.code == capi.E_INVALID and "keep_pyramid" in str(e.value)
    det.set_option("keep_pyramid", 1)
    det.run(dev(synth.make_frame(11, H, W, "luv")[None]))
    det.detect_bank()
    assert len(det.bank_detections(1, 0)) > 0
    det.close()


def test_a_captured_graph_stays_valid_and_the_profile_names_the_members_kernels(pipe):
    det, solo, fr = pipe
    det.set_option("graph", 1)
    try:
        for _ in range(3):                                                                    # plain, captured, replayed
            det.run(fr)
        det.synchronize()
        want = [tuple(a.tobytes() for a in det.detections(f)) for f in range(2)]
        det.detect_bank()
        bank = [lists_of(det, i, 2) for i in range(1, 5)]
        det.join_bank(br.nms_of(), 0, 32)
        det.run(fr)                                                                           # the captured graph, replayed
        det.synchronize()
        assert [tuple(a.tobytes() for a in det.detections(f)) for f in range(2)] == want and sum(len(w[0]) for w in want) > 0
        det.detect_bank()
        for i in range(1, 5):
            same_lists(lists_of(det, i, 2), bank[i - 1], ("after the replay", i))
            assert tuple(len(b[0]) for b in bank[i - 1]) == br.RAW_COUNTS[i]
    finally:
        det.set_option("graph", 0)
    det.set_option("profile", 1)
    try:
        det.profile()
        det.run(fr)
        det.detect_bank()
        det.join_bank(br.nms_of(), 1, 32)
        names = det.profile()
    finally:
        det.set_option("profile", 0)
    assert names["k_join_bank"][1] == 1 and "k_nms" not in names, names
    # the primary + four members; three depth-2 tile kernels; a k_rank launch for each of the two rank members (tall, wide: the forms
    # asserted above) and what the primary launches in a context without a bank (none where its level kernels write the rank cells)
    solo[0].set_option("profile", 1)
    try:
        solo[0].profile()
        solo[0].run(fr)
        own_rank = solo[0].profile().get("k_rank", (0.0, 0))[1]
    finally:
        solo[0].set_option("profile", 0)
    assert own_rank in (0, 1)
    assert names["k_sort_map"][1] == 5 and names["k_cascade_tile"][1] == 3 and names["k_rank"][1] == 2 + own_rank, names


def test_replanning_and_destroying_a_bank_returns_its_memory():
    import torch
    m = br.models()

    def cycle():
        det = HipDetector(m[0])
        det.set_bank(m[1:])
        for _ in range(2):
            det.plan(br.H, br.W, br.D, max_batch=8, max_hits=1 << 16)                           # every member: 8 x 65536 x (24 + 16 + 16) bytes of lists
        det.run(dev(np.concatenate([br.frames()] * 4)))
        det.detect_bank()
        det.synchronize()
        assert len(det.bank_detections(4, 7)) == br.RAW_COUNTS[4][1]
        det.close()
    cycle()
    torch.cuda.synchronize()
    torch.cuda.empty_cache()
    free0 = torch.cuda.mem_get_info()[0]
    for _ in range(3):
        cycle()
    torch.cuda.synchronize()
    torch.cuda.empty_cache()
    # members left behind would cost six plans x four members x at least 29 MB of lists = 700 MB; the figure is the device's, so
    # other processes may move it: a third of the leak's size is the bound
    assert free0 - torch.cuda.mem_get_info()[0] < 233 << 20
