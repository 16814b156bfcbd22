"""A bank of classifiers on one pyramid, without a GPU (include/acf_hip.h: acf_hip_bank_check, acf_hip_set_bank .. acf_hip_op_join_bank):
  1. the preconditions of tests/test_gpu_bank.py, from the CPU oracle, so that no GPU comparison there is vacuous: the five models of
     the pipeline case share one pyramid bit for bit, their raw counts, the levels the wide model has windows on, repeated scores,
     suppression across the models;
  2. acf_hip_bank_check: one deviating pyramid / channel field at a time, LDCF, a bad child[], an out-of-range feature id;
  3. what the entries answer to a null context;
  4. the restatement (tests/bank_ref.py): separate = 1 against the union of the oracle's per-model bbNms, separate = 0 with one model
     against the oracle's bbNms, and that the designed cases exercise what their names say.
The two tests of group 1 that ask only the oracle (one pyramid for the five models; counts, levels and ties) state preconditions: they
pass without the feature as well.  Every other test here needs the new entries or the new binding."""
import ctypes as C

import numpy as np
import pytest

import bank_ref as br
from acf_amd import capi, synth
from acf_amd.detector import HipDetector

F = np.float32


# ---------------------------------------------------------------- 1. preconditions of the pipeline case

def test_the_five_models_share_one_pyramid(oracle):
    plans = [oracle.Plan(m, br.H, br.W, br.D) for m in br.models()]
    for fr in br.frames():
        pyrs = [oracle.chns_pyramid(p, fr)[0] for p in plans]
        assert all(p.tobytes() == pyrs[0].tobytes() for p in pyrs[1:])
    assert len({p.nScales for p in plans}) == 1 and len({p.nChns for p in plans}) == 1


def test_raw_counts_levels_and_ties_of_the_pipeline_case(oracle):
    lists = br.oracle_lists()
    assert tuple(tuple(len(lists[m][f][0]) for f in range(2)) for m in range(5)) == br.RAW_COUNTS
    totals = [sum(br.RAW_COUNTS[m][f] for m in range(5)) for f in range(2)]
    assert totals == [715, 629] and max(totals) <= capi.NMS_CAP
    wide = oracle.Plan(br.models()[4], br.H, br.W, br.D)
    # levels smaller than a member's window: the wide model has windows on levels 0 .. 11 of the 17, the tall one on 0 .. 12
    assert [i for i in range(wide.nScales) if wide.levels[i].nWinR * wide.levels[i].nWinC > 0] == list(range(12))
    tall = oracle.Plan(br.models()[1], br.H, br.W, br.D)
    assert [i for i in range(tall.nScales) if tall.levels[i].nWinR * tall.levels[i].nWinC > 0] == list(range(13)) and tall.nScales == 17
    repeats = []
    for f in range(2):
        sc = np.concatenate([lists[m][f][0]["score"] for m in range(5)])
        repeats.append(len(sc) - len(np.unique(sc.view(np.uint32))))
    assert repeats == [183, 60]                                                               # tie order is exercised


def test_suppression_across_the_models_really_happens(oracle):
    dets, counts = br.lists_to_arrays([[l[f][0] for f in range(2)] for l in br.oracle_lists()], br.MAX_HITS)
    for (typ, ovr, overlap), (joint, sep) in br.JOINT_KEPT.items():
        q = br.nms_of(typ, ovr=ovr, overlap=overlap)
        assert tuple(br.join(dets, counts, q, 0, k=4)[1]) == joint
        assert tuple(br.join(dets, counts, q, 1, k=4)[1]) == sep


# ---------------------------------------------------------------- 2. acf_hip_bank_check

DEVIATIONS = dict(nPerOct=4, nOctUp=1, nApprox=3, pad_h=4, pad_w=4, minDs_h=20, minDs_w=20, smooth=0.5, shrink=2, colorEnabled=0, colorSmooth=0.5,
                  colorSpace=capi.CS_RGB, gradMagEnabled=0, colorChn=1, normRad=3, normConst=0.01, full=1, gradHistEnabled=0, binSize=4, nOrients=4,
                  softBin=1, isLuv=0)


def test_bank_check_accepts_the_pipeline_members():
    m = br.models()
    for member in m[1:]:
        assert HipDetector.bank_check(m[0], member) == (capi.OK, "")


@pytest.mark.parametrize("field", list(DEVIATIONS) + ["nLambdas", "lambdas[i]"])
def test_bank_check_refuses_one_deviating_field(field):
    primary, member = br.models()[0], dict(br.models()[1])
    if field == "nLambdas":
        member["lambdas"] = []
    elif field == "lambdas[i]":
        member["lambdas"] = [0.0, 0.2, 0.1083]
    else:
        assert member[field] != DEVIATIONS[field]
        member[field] = DEVIATIONS[field]
    rc, why = HipDetector.bank_check(primary, member)
    assert rc == capi.E_INVALID and ("member's %s differs" % field) in why, (rc, why)
    rc, why = HipDetector.bank_check(member, primary)                                         # either way round
    assert rc == capi.E_INVALID and ("member's %s differs" % field) in why, (rc, why)


def test_bank_check_refuses_ldcf_bad_children_and_feature_ids():
    primary = br.models()[0]
    ldcf = synth.make_model(name="TINY", seed=9, nTrees=8, ldcfK=2)
    assert HipDetector.bank_check(primary, ldcf)[0] == capi.E_UNSUPPORTED
    assert HipDetector.bank_check(ldcf, primary)[0] == capi.E_UNSUPPORTED
    walk = dict(br.models()[2])
    walk["child"] = walk["child"].copy()
    walk["child"][5, 1] = walk["child"].shape[1]                                              # outside the tree
    rc, why = HipDetector.bank_check(primary, walk)
    assert rc == capi.E_INVALID and "child[] of tree 5, node 1" in why
    walk["child"][5, 1] = 1                                                                   # a backward reference
    assert HipDetector.bank_check(primary, walk)[0] == capi.E_INVALID
    tall = dict(br.models()[1])
    nF = synth.n_channels(tall) * (tall["modelDsPad_h"] // 4) * (tall["modelDsPad_w"] // 4)
    tall["fids"] = tall["fids"].copy()
    assert tall["fids"].max() == nF - 1 or tall["fids"].max() < nF
    tall["fids"][7, 0] = nF                                                                   # one past the member's own window cells
    rc, why = HipDetector.bank_check(primary, tall)
    assert rc == capi.E_INVALID and "feature id out of range" in why and "tree 7, node 0" in why
    tall["fids"][7, 0] = nF - 1
    assert HipDetector.bank_check(primary, tall)[0] == capi.OK
    lib = capi.load()
    p, keep = capi.make_params(primary)
    assert lib.acf_hip_bank_check(None, C.byref(p), None, 0) == capi.E_INVALID
    assert lib.acf_hip_bank_check(C.byref(p), None, None, 0) == capi.E_INVALID
    assert lib.acf_hip_bank_check(C.byref(p), C.byref(p), None, 0) == capi.OK                 # no room for a reason: none is written
    empty = capi.Params()
    C.memmove(C.byref(empty), C.byref(p), C.sizeof(capi.Params))
    empty.nTrees = 0
    assert lib.acf_hip_bank_check(C.byref(p), C.byref(empty), None, 0) == capi.E_INVALID


# ---------------------------------------------------------------- 3. a null context

def test_null_context_refusals():
    lib = capi.load()
    p, keep = capi.make_params(br.models()[0])
    n = C.c_int()
    det = (capi.Detection * 4)()
    hit = (capi.Hit * 4)()
    lv = (capi.Level * 64)()
    words = (C.c_int32 * capi.CF_WORDS)()
    spec = br.spec_of()
    rec, cnt = np.zeros((1, 8, 32), np.uint8), np.zeros(1, np.int32)
    dets, counts = br.pack(br.TWIN)
    v = lambda a: C.c_void_p(a.ctypes.data)
    assert lib.acf_hip_set_bank(None, C.byref(p), 1) == capi.E_INVALID
    assert lib.acf_hip_detect_bank(None) == capi.E_INVALID
    assert lib.acf_hip_get_bank_levels(None, 0, lv, 64) != capi.OK
    assert lib.acf_hip_get_bank_detections(None, 0, 0, det, 4, C.byref(n)) == capi.E_INVALID
    assert lib.acf_hip_get_bank_hits(None, 1, 0, hit, 4, C.byref(n)) == capi.E_INVALID
    assert lib.acf_hip_get_bank_forms(None, 0, words, capi.CF_WORDS, C.byref(n)) == capi.E_INVALID
    assert lib.acf_hip_join_bank(None, C.byref(spec), v(rec), v(cnt), None, None) == capi.E_INVALID
    assert lib.acf_hip_op_join_bank(None, v(dets), v(counts), 2, 1, dets.shape[2], C.byref(spec), v(rec), v(cnt), None, None) == capi.E_INVALID
    assert C.sizeof(capi.BankDetection) == capi.BANK_DTYPE.itemsize == 32 and C.sizeof(capi.BankSpec) == 72


# ---------------------------------------------------------------- 4. the restatement

@pytest.mark.parametrize("typ,ovr,overlap", [("maxg", "union", 0.5), ("max", "min", 0.65), ("maxg", "min", 0.3)])
def test_separate_survivors_are_the_union_of_the_oracles_per_model_nms(oracle, typ, ovr, overlap):
    lists = [[l[f][0] for f in range(2)] for l in br.oracle_lists()]
    dets, counts = br.lists_to_arrays(lists, br.MAX_HITS)
    q = br.nms_of(typ, ovr=ovr, overlap=overlap)
    rec, cnt, _, _ = br.join(dets, counts, q, 1, k=1024)
    for f in range(2):
        want = set()
        for m in range(5):
            d = lists[m][f]
            boxes = np.stack([d[t] for t in ("x", "y", "w", "h")], axis=1)
            want |= {(m, int(i)) for i in oracle.nms(boxes, d["score"].astype(np.float64), q)}
        got = [(int(r["model"]), int(r["index"])) for r in rec[f, :cnt[f]]]
        assert len(got) == len(set(got)) and set(got) == want
        sc = rec[f, :cnt[f]]["score"]
        assert (np.diff(sc) <= 0).all()                                                       # the joint score order
        # one model alone, separate or not: the oracle's bbNms, order included
        for m in (0, 3):
            d = lists[m][f]
            boxes = np.stack([d[t] for t in ("x", "y", "w", "h")], axis=1)
            alone = br.join(dets[m:m + 1], counts[m:m + 1], q, 0, k=1024)
            assert [int(r["index"]) for r in alone[0][f, :alone[1][f]]] == list(oracle.nms(boxes, d["score"].astype(np.float64), q))


def test_designed_cases_exercise_what_they_name():
    e = br.expected
    assert [int(e("the same box from two models, separate %d" % s)[1][0]) for s in (0, 1)] == [1, 2]
    assert e("total 2048")[1][0] > 64 and e("total 2049")[1][0] == -1 and e("a list over max_hits")[1][0] > 0 and e("a list over max_hits")[1][1] == -1
    assert e("a count of -1")[1][0] == -1 and e("a count of -1")[1][1] > 0
    assert e("K 1 below the survivors")[1][0] == 5 and e("K 1 below the survivors")[3].tolist() == [[0]]
    assert sorted(set(e("thr removes a whole model")[0][0, :3]["model"].tolist())) == [0, 1] and e("thr removes a whole model")[1][0] == 3
    assert e("thr drops everything")[1][0] == 0 and e("prune maxCount 0")[1][0] == 1 and e("prune maxCount 3")[1][0] == 3
    assert {int(m) for m in e("nine models, separate 0")[0][0, :e("nine models, separate 0")[1][0]]["model"]} <= {0, 2, 3, 5, 6, 7, 8}
    assert e("nine models, separate 1")[1][0] >= e("nine models, separate 0")[1][0]
    both = [e("empty lists at every place, two frames, separate 0")[1].tolist(), br.cases()["empty lists at every place, two frames, separate 0"]["counts"].tolist()]
    assert both[1] == [[0, 3], [4, 0], [0, 0], [5, 2], [0, 4]] and min(both[0]) > 0
    assert e("chain, maxg, separate 0")[1][0] == 2 and e("chain, max, separate 0")[1][0] == 1 and e("chain, max, separate 1")[1][0] == 3
    assert e("chain in one model, maxg")[1][0] == 2
    g = e("grow 1.5, det_scale 0.5")
    d = g[0][0, 0]
    assert np.array_equal(g[2][0, 0], HipDetector.crop_box([int(d[t]) for t in ("x", "y", "w", "h")], 0.5, 1.5))
