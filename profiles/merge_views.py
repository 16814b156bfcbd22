"""k_merge_views beside k_nms on N concatenated boxes of one stored frame, and the two routes of the pipeline case (profiles/merge_views.md).
  python profiles/merge_views.py profile             k_merge_views from option "profile" (N = 360, 2048), then the wall times of the pipeline
                                                     case's host route and of merge_views
  rocprofv3 --kernel-trace --stats -d OUT -o NAME --output-format csv -- python profiles/merge_views.py kernels N [LIB]
                                                     40 calls each of op_nms and op_merge_views on the same N boxes and parameters; with LIB
                                                     (another build's libacf_hip.so, e.g. the parent commit's): its op_nms only"""
import ctypes as C
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np

SPLIT = {360: [72] * 5, 2048: [256] * 8}
ITER = 40


def boxes_of(N):
    import merge_views_ref as mr
    lists = mr.random_lists(N, SPLIT[N], span=250 if N > 1000 else 110)
    dets, counts = mr.pack(lists)
    views = mr.shifts(len(lists))
    flat = [(v, i) for v in range(len(lists)) for i in range(len(lists[v]))]
    ib = np.array([[dets[v, i]["x"] + int(views[v][2]), dets[v, i]["y"] + int(views[v][5]), dets[v, i]["w"], dets[v, i]["h"]] for v, i in flat], np.int32)
    sc = np.array([dets[v, i]["score"] for v, i in flat], np.float64)
    return dets, counts, views, ib, sc, mr.nms_of("maxg", "union", 0.5)


def kernels(N, parent):
    dets, counts, views, ib, sc, q = boxes_of(N)
    if parent:
        import torch  # noqa: F401  (its HIP runtime first)
        lib = C.CDLL(parent)
        ctx = C.c_void_p()
        assert lib.acf_hip_create(0, None, C.byref(ctx)) == 0
        keep, cnt = np.zeros(N, np.int32), C.c_int(0)
        for _ in range(ITER):
            assert lib.acf_hip_op_nms(ctx, C.c_void_p(ib.ctypes.data), C.c_void_p(sc.ctypes.data), N, C.byref(q), C.c_void_p(keep.ctypes.data), C.byref(cnt)) == 0
        print(parent, "k_nms N", N, "survivors", cnt.value)
        lib.acf_hip_destroy(ctx)
        return
    from acf_amd.detector import HipDetector
    det = HipDetector()
    for _ in range(ITER):
        keep = det.op_nms(ib, sc, q)
        got = det.op_merge_views(dets, counts, views, [0] * len(views), 1, q, 64)
    assert got[1][0] == len(keep), (got[1], len(keep))
    print("N", N, "survivors", len(keep))
    det.close()


def profile():
    import torch
    import merge_views_ref as mr
    import view_ref as vr
    from acf_amd import capi
    from acf_amd.detector import HipDetector
    det = HipDetector()
    det.set_option("profile", 1)
    for N in SPLIT:
        dets, counts, views, ib, sc, q = boxes_of(N)
        ms = []
        for _ in range(ITER):
            det.profile()
            det.op_merge_views(dets, counts, views, [0] * len(views), 1, q, 64)
            ms.append(det.profile()["k_merge_views"][0])
        ms = sorted(ms[5:])
        print("profile k_merge_views N %d: median %.1f us, min %.1f, max %.1f (%d calls)" % (N, 1e3 * ms[len(ms) // 2], 1e3 * ms[0], 1e3 * ms[-1], len(ms)))
    det.close()
    # the pipeline case: the host route of before against merge_views, wall time from the end of run_view to boxes on the device
    views, frames, k = mr.pipe_views(), mr.PIPE_FRAMES, mr.PIPE_K
    n = len(views)
    det = HipDetector(vr.model(), vr.H, vr.W, 3, max_batch=n, max_hits=vr.MAX_HITS)
    x = torch.from_numpy(vr.stored_u8()[0]).cuda()
    src = det.crop_source_tensor(x, layout="nhwc")
    dv, df = torch.from_numpy(views).cuda(), torch.from_numpy(frames).cuda()
    q = mr.nms_of("maxg", **mr.PIPE_NMS)
    host, devr = [], []
    for it in range(12):
        det.run_view(src, dv, df, mr.PIPE_SAMPLES)
        det.synchronize()
        t0 = time.perf_counter()
        boxes, fidx = np.zeros((2, k, 4), np.float32), np.full((2, k), -1, np.int32)
        for f in range(2):
            ent = [(v, d) for v in range(n) if frames[v] == f for d in det.detections(v)[0]]
            bx = np.array([HipDetector.view_box(views[v], [int(d[t]) for t in ("x", "y", "w", "h")]) for v, d in ent], np.float32)
            # (op_nms takes int boxes: the host route of before rounds the mapped boxes)
            keep = det.op_nms(np.rint(bx).astype(np.int32), np.array([d["score"] for _, d in ent], np.float64), q)
            for s, t in enumerate(keep[:k]):
                boxes[f, s], fidx[f, s] = bx[t], f
        b2, f2 = torch.from_numpy(boxes).cuda(), torch.from_numpy(fidx).cuda()
        torch.cuda.synchronize()
        host.append(time.perf_counter() - t0)
        det.run_view(src, dv, df, mr.PIPE_SAMPLES)
        det.synchronize()
        t0 = time.perf_counter()
        out = det.merge_views(dv, df, 2, q, k)
        det.synchronize()
        devr.append(time.perf_counter() - t0)
    host, devr = sorted(host[2:]), sorted(devr[2:])
    print("pipeline case (%d views, %s raw detections): host route median %.2f ms (min %.2f), merge_views + synchronize median %.3f ms (min %.3f)" %
          (n, [len(det.detections(v)[0]) for v in range(n)], 1e3 * host[len(host) // 2], 1e3 * host[0], 1e3 * devr[len(devr) // 2], 1e3 * devr[0]))
    det.close()


if __name__ == "__main__":
    if sys.argv[1] == "kernels":
        kernels(int(sys.argv[2]), sys.argv[3] if len(sys.argv) > 3 else None)
    else:
        profile()
