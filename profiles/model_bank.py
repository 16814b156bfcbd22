"""A second classifier on the pyramid that is already there against a second context (profiles/model_bank.md): cfg 2 of bench.py
(1920 x 1080 planar LUV frames, FACE80-shaped models of 2048 trees), 96 frames a batch, the primary (seed 1) and one member (seed 2).
  python profiles/model_bank.py [frames] [iterations]
    (a) run alone                                  one context, the primary
    (b) run + detect_bank + join_bank              one context, the primary and the member
    (c) two contexts, one model each, same frames  the way of before
Wall time per batch from the first call to acf_hip_synchronize, the median of the iterations after two warm-up batches; then the
per-kernel profile (option "profile") of one batch of (b), and k_rank's share of the member's cascade."""
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np


def med(fn, sync, it):
    ts = []
    for _ in range(it + 2):
        sync()
        t0 = time.perf_counter()
        fn()
        sync()
        ts.append(time.perf_counter() - t0)
    ts = sorted(ts[2:])
    return 1e3 * ts[len(ts) // 2], 1e3 * ts[0], 1e3 * ts[-1]


def main():
    import torch
    from acf_amd import capi, synth
    from acf_amd.detector import HipDetector
    B = int(sys.argv[1]) if len(sys.argv) > 1 else 96
    it = int(sys.argv[2]) if len(sys.argv) > 2 else 20
    H, W = 1080, 1920
    primary, member = synth.make_model(seed=1, name="FACE80"), synth.make_model(seed=2, name="FACE80")
    assert HipDetector.bank_check(primary, member)[0] == capi.OK
    base = [torch.from_numpy(synth.make_frame(i + 1, H, W, "luv")) for i in range(4)]           # (bench.py repeats a few frames as well)
    fr = torch.stack([base[i % 4] for i in range(B)]).cuda()
    q = capi.make_nms("maxg", overlap=0.65, ovrDnm="min")
    one = HipDetector(primary, H, W, 3, max_batch=B, max_hits=8192)
    a = med(lambda: one.run(fr), one.synchronize, it)
    two = HipDetector(member, H, W, 3, max_batch=B, max_hits=8192)

    def both():
        one.run(fr)
        two.run(fr)
        one.synchronize()
    c = med(both, two.synchronize, it)
    raw = [[len(d.raw_detections(f)) for f in range(4)] for d in (one, two)]
    one.close()
    two.close()
    bank = HipDetector(primary)
    bank.set_bank([member])
    bank.plan(H, W, 3, max_batch=B, max_hits=8192)

    def joined():
        bank.run(fr)
        bank.detect_bank()
        bank.join_bank(q, 0, 64)
    b = med(joined, bank.synchronize, it)
    rec, cnt, _, _ = bank.join_bank(q, 0, 64)
    bank.synchronize()
    print("frames %d, iterations %d; raw detections of frames 0 .. 3: primary %s, member %s; joined %s" % (B, it, raw[0], raw[1], cnt.cpu().numpy()[:4].tolist()))
    for name, t in (("(a) run alone", a), ("(b) run + detect_bank + join_bank", b), ("(c) two contexts", c)):
        print("%-36s median %.3f ms  (min %.3f, max %.3f)" % (name, t[0], t[1], t[2]))
    print("a second classifier costs (b) - (a) = %.3f ms on the bank, (c) - (a) = %.3f ms as a context: ratio %.2f" % (b[0] - a[0], c[0] - a[0], (b[0] - a[0]) / (c[0] - a[0])))
    bank.set_option("profile", 1)
    tot = {}
    for _ in range(5):
        bank.profile()
        joined()
        for k, (ms, n) in bank.profile().items():
            tot.setdefault(k, []).append((ms, n))
    print("per-kernel profile of one batch of (b), median of 5 (the kernels run one after another under the profile's markers):")
    for k, v in tot.items():
        ms = sorted(x[0] for x in v)
        print("  %-22s %8.3f ms  %d launches" % (k, ms[len(ms) // 2], v[0][1]))
    print("  member's forms:", bank.bank_forms(1)["path"], "rank" if bank.bank_forms(1)["rank"] else "float")
    bank.close()


if __name__ == "__main__":
    main()
