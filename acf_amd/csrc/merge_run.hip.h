// merge_run.hip.h — part of acf_hip.hip (included there and nowhere else): the detections of a batch of views merged into their stored
// frames (the header's "merging the views' detections" section; kernel k_merge_views, kernels_merge.hip.h).
//   mergeChecked             what a call states, checked on the host before anything touches the device: the refusal, or the kernel's
//                            arguments without its lists and outputs
//   launchMerge              the one launch, under the profile name k_merge_views
//   acf_hip_merge_views      the lists of the context's last acf_hip_run_view (d_nmsDets / d_nmsCounts or cs.d_dets / cs.d_counts, as
//                            acf_hip_cut_detections reads them); acf_hip_op_merge_views: a caller's host lists through a Scratch
// The pipeline entry allocates nothing, never waits for the device and changes nothing acf_hip_run_view left behind (a captured graph
// stays valid).
#pragma once

namespace
{

const size_t kMergeLds = size_t(NMS_CAP) * (8 + 16 + 4 + 1); // (k_nms's; the offsets are the kernel's own static LDS)

const char* mergeSpecBad(const acf_hip_merge_spec* s)
{
    if (!s)
    {
        return "null spec";
    }
    if (s->max_per_frame < 1 || s->max_per_frame > ACF_HIP_NMS_CAP)
    {
        return "max_per_frame must be 1 .. ACF_HIP_NMS_CAP";
    }
    if (!(s->grow > 0.f && std::isfinite(s->grow)))
    {
        return "grow must be a positive finite number";
    }
    if (s->reserved[0] != 0 || s->reserved[1] != 0)
    {
        return "reserved must be 0";
    }
    const acf_hip_nms_params& q = s->nms;
    if (q.type < 0 || q.type > 2 || !(q.overlap == q.overlap) || (q.prune && q.maxCount < 0))
    {
        return "nms: type 0..2, overlap a number, maxCount >= 0";
    }
    return nullptr;
}

int mergeChecked(acf_hip_ctx* c, const std::string& who, const void* views, int nViews, int nFrames, const acf_hip_merge_spec* spec, const void* out,
    const void* countsOut, MergeArgs& a)
{
    if (!views || !out || !countsOut)
    {
        return fail(c, ACF_HIP_E_INVALID, who + "null views, records or counts");
    }
    if (nViews < 1 || nViews > MERGE_VIEWS_MAX || nFrames < 1)
    {
        return fail(c, ACF_HIP_E_INVALID, who + "n_views must be 1 .. 1024, n_frames >= 1");
    }
    if (const char* bad = mergeSpecBad(spec))
    {
        return fail(c, ACF_HIP_E_INVALID, who + bad);
    }
    if (!c->kids.empty())
    {
        return fail(c, ACF_HIP_E_UNSUPPORTED, who + "not available with option \"streams\" > 1");
    }
    a.nViews = nViews;
    a.nFrames = nFrames;
    a.type = spec->nms.type;
    a.ovrUnion = spec->nms.ovrDnmUnion != 0;
    a.doPrune = spec->nms.prune != 0;
    a.maxCount = spec->nms.maxCount;
    a.overlap = spec->nms.overlap;
    a.thr = spec->nms.thr;
    a.pruneRatio = spec->nms.pruneRatio;
    a.K = spec->max_per_frame;
    a.grow = spec->grow;
    return ACF_HIP_OK;
}

int launchMerge(acf_hip_ctx* c, const MergeArgs& a)
{
    HIPCHK(c, hipSetDevice(c->device));
    prof(c, c->stream, "k_merge_views");
    hipLaunchKernelGGL(k_merge_views, dim3(unsigned(a.nFrames)), dim3(1024), kMergeLds, c->stream, a);
    LAUNCHCHK(c, "k_merge_views");
    prof(c, c->stream, "(end)");
    return ACF_HIP_OK;
}

} // namespace

int acf_hip_merge_views(acf_hip_ctx* c, const float* views, const int32_t* frames, int nViews, int nFrames, const acf_hip_merge_spec* spec,
    acf_hip_merged_detection* out, int32_t* countsOut, float* boxesOut, int32_t* framesOut, float* quadsOut)
{
    if (int rc = needCtx(c)) return rc;
    const std::string who = "merge_views: ";
    MergeArgs a{};
    if (int rc = mergeChecked(c, who, views, nViews, nFrames, spec, out, countsOut, a)) return rc;
    if (!c->hasPlan || !c->detectValid || !c->viewRun)
    {
        return fail(c, ACF_HIP_E_INVALID, who + "no detections of views (call acf_hip_run_view first)");
    }
    if (nViews != c->lastBatch)
    {
        return fail(c, ACF_HIP_E_INVALID, who + "n_views must be the last acf_hip_run_view's");
    }
    const bool nms = nmsActive(c);
    a.dets = nms ? c->d_nmsDets : c->cs.d_dets;
    a.counts = nms ? c->d_nmsCounts : c->cs.d_counts;
    a.maxHits = c->maxHits;
    a.views = views;
    a.frame = frames;
    a.out = out;
    a.countsOut = countsOut;
    a.boxesOut = boxesOut;
    a.framesOut = framesOut;
    a.quadsOut = quadsOut;
    return launchMerge(c, a);
}

int acf_hip_op_merge_views(acf_hip_ctx* c, const acf_hip_detection* dets, const int32_t* counts, int maxHits, const float* views, const int32_t* frames, int nViews,
    int nFrames, const acf_hip_merge_spec* spec, acf_hip_merged_detection* out, int32_t* countsOut, float* boxesOut, int32_t* framesOut, float* quadsOut)
{
    if (int rc = needCtx(c)) return rc;
    const std::string who = "op_merge_views: ";
    MergeArgs a{};
    if (int rc = mergeChecked(c, who, views, nViews, nFrames, spec, out, countsOut, a)) return rc;
    if (!dets || !counts || maxHits < 1)
    {
        return fail(c, ACF_HIP_E_INVALID, who + "null lists or counts, or max_hits < 1");
    }
    const size_t slots = size_t(nFrames) * size_t(a.K);
    if (slots > 0x7fffffffu / 8 || size_t(nViews) * size_t(maxHits) > 0x7fffffffu)
    {
        return fail(c, ACF_HIP_E_INVALID, who + "more than 2^31 - 1 list entries or output floats");
    }
    HIPCHK(c, hipSetDevice(c->device));
    Scratch s;
    a.dets = s.upload(dets, size_t(nViews) * size_t(maxHits));
    a.counts = s.upload(counts, size_t(nViews));
    a.maxHits = maxHits;
    a.views = s.upload(views, size_t(nViews) * 6);
    a.frame = frames ? s.upload(frames, size_t(nViews)) : nullptr;
    // (the caller's outputs go over first: a slot the kernel does not write keeps what the caller had there)
    a.out = s.upload(out, slots);
    a.countsOut = s.upload(countsOut, size_t(nFrames));
    a.boxesOut = boxesOut ? s.upload(boxesOut, slots * 4) : nullptr;
    a.framesOut = framesOut ? s.upload(framesOut, slots) : nullptr;
    a.quadsOut = quadsOut ? s.upload(quadsOut, slots * 8) : nullptr;
    if (!a.dets || !a.counts || !a.views || (frames && !a.frame) || !a.out || !a.countsOut || (boxesOut && !a.boxesOut) || (framesOut && !a.framesOut) ||
        (quadsOut && !a.quadsOut))
    {
        (void)hipGetLastError();
        return fail(c, ACF_HIP_E_HIP, who + "device allocation or copy failed");
    }
    int rc = launchMerge(c, a);
    if (rc || (rc = Scratch::download(c, "op_merge_views", out, a.out, slots)) || (rc = Scratch::download(c, "op_merge_views", countsOut, a.countsOut, size_t(nFrames))) ||
        (boxesOut && (rc = Scratch::download(c, "op_merge_views", boxesOut, a.boxesOut, slots * 4))) ||
        (framesOut && (rc = Scratch::download(c, "op_merge_views", framesOut, a.framesOut, slots))) ||
        (quadsOut && (rc = Scratch::download(c, "op_merge_views", quadsOut, a.quadsOut, slots * 8))))
    {
        return rc;
    }
    return ACF_HIP_OK;
}
