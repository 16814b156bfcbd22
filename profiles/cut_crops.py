"""Measurement for profiles/cut_crops.md: acf_hip_cut_detections against the composition that exists without it (acf_hip_video_to_rgb of
the whole frames, the boxes read back, the crops by torch), 96 NV12 frames of 2160 x 3840 detected at min-width reduction, K = 8,
112 x 112 f16.  Prints one JSON line; `python profiles/cut_crops.py [out.json]` also writes it to a file."""
import ctypes as C
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np
import torch
import torch.nn.functional as Fn

import cut_crops_ref as ccr
import resized_entry_case as rc
import yuv_desc_ref as ydr
from acf_amd import capi, synth
from acf_amd.detector import HipDetector

H, W, NF, K, OUT, MINW = 2160, 3840, 96, 8, 112, 300
REPS, WARM = 20, 3


def frames():
    out = []
    for i in range(4):
        Y, U, V = rc.yuv_planes(900 + i, H // 2, W // 2, 1, 1)
        Y, U, V = (np.repeat(np.repeat(p, 2, 0), 2, 1) for p in (Y, U, V))      # 4K frames with the 1080p frames' structure
        out.append(ydr.pack("nv12", Y, U, V))
    return np.stack([out[i % 4] for i in range(NF)])


def timed(stream, fn, reps=REPS, warm=WARM):
    ev, wall = [], []
    for i in range(warm + reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        stream.synchronize()
        t0 = time.perf_counter()
        a.record(stream)
        fn()
        b.record(stream)
        stream.synchronize()
        t1 = time.perf_counter()
        if i >= warm:
            ev.append(a.elapsed_time(b))
            wall.append((t1 - t0) * 1e3)
    return dict(event_ms_median=float(np.median(ev)), event_ms_min=float(np.min(ev)), event_ms_max=float(np.max(ev)), wall_ms_median=float(np.median(wall)))


def main():
    model = synth.make_model(seed=3, name="FACE80", nTrees=64, cascThr=-1.0)     # ~550 raw, ~100 surviving detections a frame (CPU oracle)
    scale = HipDetector.resize_scale(model["modelDs_w"], MINW)
    dr, dc = HipDetector.oriented_resized_dims(H, W, 0, scale)
    stream = torch.cuda.Stream()
    det = HipDetector(model, dr, dc, 3, max_batch=NF, max_hits=1 << 13, stream=stream.cuda_stream)
    det.set_nms(capi.make_nms(type="maxg", overlap=0.65, ovrDnm="min"))
    desc, fb = HipDetector.yuv_desc("nv12", H, W)
    x = torch.from_numpy(frames()).cuda()
    torch.cuda.synchronize()
    det.run_yuv_resized(x, NF, desc, H, W, scale, 0)
    det.synchronize()
    dets = [det.detections(f)[0] for f in range(NF)]
    counts = [len(d) for d in dets]
    src = det.crop_source_yuv(x, NF, desc, None, H, W, 0)
    spec = HipDetector.crop_spec(OUT, 1, torch.float16, "planar", K, 1.0)
    out = torch.zeros((NF, K, 3, OUT, OUT), dtype=torch.float16, device="cuda")
    boxes = torch.zeros((NF, K, 4), dtype=torch.float32, device="cuda")
    cnt = torch.zeros((NF,), dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()
    res = {"frames": NF, "size": [H, W], "scale": scale, "plan": [dr, dc], "K": K, "out": OUT, "detections_per_frame_min_median_max": [int(np.min(counts)), float(np.median(counts)), int(np.max(counts))]}

    def cut():
        det.cut_detections(src, OUT, K, det_scale=scale, dtype=torch.float16, out=out, boxes_out=boxes, counts_out=cnt)
    res["cut_detections"] = timed(stream, cut)
    n_crops = int(cnt.clamp(min=0).sum().item())
    res["crops"] = n_crops
    # the forms and the bytes, by arithmetic (NV12: 1.5 bytes a pixel)
    bx = boxes.cpu().numpy()
    cn = cnt.cpu().numpy()
    forms, staged_px, gather_fetch_px, foot_px, widths = {0: 0, 1: 0}, 0, 0, 0, []
    for f in range(NF):
        for i in range(max(int(cn[f]), 0)):
            b = bx[f, i]
            fm = HipDetector.crop_form(spec, b, H, W, 3, 1)
            forms[fm] += 1
            x0, x1 = max(int(np.floor(b[0])), 0), min(int(np.ceil(b[0] + b[2])) + 1, W)
            y0, y1 = max(int(np.floor(b[1])), 0), min(int(np.ceil(b[1] + b[3])) + 1, H)
            px = max(x1 - x0, 0) * max(y1 - y0, 0)
            foot_px += px
            widths.append(float(b[2]))
            if fm == 0:
                staged_px += px
            else:
                gather_fetch_px += 4 * OUT * OUT
    res["forms"] = {"staged": forms[0], "gather": forms[1]}
    res["box_width_min_median_max"] = [float(np.min(widths)), float(np.median(widths)), float(np.max(widths))] if widths else []
    res["bytes"] = {
        "cut_staged_read": int(staged_px * 1.5), "cut_gather_fetched_upper": int(gather_fetch_px * 3), "cut_gather_distinct_upper": int(min(gather_fetch_px, foot_px - staged_px) * 1.5),
        "cut_written": n_crops * 3 * OUT * OUT * 2, "composition_read_frames": NF * fb, "composition_written_rgb": NF * H * W * 3,
        "composition_crop_read_upper": int(foot_px * 3)}

    # the composition that exists without the entry: the whole frames to RGB, the boxes read back, the crops by a tensor library
    rgb = torch.empty((NF, H, W, 3), dtype=torch.uint8, device="cuda")
    out2 = torch.zeros((NF, K, 3, OUT, OUT), dtype=torch.float16, device="cuda")
    torch.cuda.synchronize()

    def composition():
        det._chk(det.lib.acf_hip_video_to_rgb(det.ctx, C.c_void_p(x.data_ptr()), NF, H, W, C.byref(desc), None, C.c_void_p(rgb.data_ptr())))
        with torch.cuda.stream(stream):
            for f in range(NF):
                d, _ = det.detections(f)                                        # the read-back (waits for the stream)
                for i in range(min(len(d), K)):
                    b = HipDetector.crop_box([d["x"][i], d["y"][i], d["w"][i], d["h"][i]], scale, 1.0)
                    x0, y0 = int(np.clip(np.floor(b[0]), 0, W - 1)), int(np.clip(np.floor(b[1]), 0, H - 1))
                    x1, y1 = int(np.clip(np.ceil(b[0] + b[2]), x0 + 1, W)), int(np.clip(np.ceil(b[1] + b[3]), y0 + 1, H))
                    c = rgb[f, y0:y1, x0:x1].permute(2, 0, 1)[None].float()
                    out2[f, i] = (Fn.interpolate(c, size=(OUT, OUT), mode="bilinear", align_corners=False)[0] * (1.0 / 255.0)).half()
    res["composition"] = timed(stream, composition, reps=5, warm=1)

    def to_rgb_only():
        det._chk(det.lib.acf_hip_video_to_rgb(det.ctx, C.c_void_p(x.data_ptr()), NF, H, W, C.byref(desc), None, C.c_void_p(rgb.data_ptr())))
    res["composition_video_to_rgb_alone"] = timed(stream, to_rgb_only, reps=5, warm=1)
    if len(sys.argv) > 1:
        with open(sys.argv[1], "w") as fh:
            json.dump(res, fh, indent=1)
    print(json.dumps(res))
    det.close()


if __name__ == "__main__":
    main()
