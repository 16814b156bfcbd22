// readback.hip.h — part of acf_hip.hip (included there and nowhere else): what a caller reads back after a run.
//   fetchCounts / rawCount   the per-frame counts of the last batch on the host (after the device NMS / before it)
//   readRecords              one frame's list: acf_hip_get_detections, _get_raw_detections, _get_hits
//   acf_hip_export_detections   the batch's records into a device buffer (k_export)
//   acf_hip_read_level / _read_rank_level / _read_tap   pyramid levels, rank cells and the kept per-stage planes (tapPlane)
//   acf_hip_rank_cells_host  the rank tables' host form (what acf_hip_read_rank_level's cells mean)
//   acf_hip_profile_get      the profile markers' times by kernel name (ProfileTotals)
// On a context with sub-batch children a frame is read from the child that owns it (onFrameOwner).
#pragma once

static int fetchCounts(acf_hip_ctx* c)
{
    if (!c->detectValid)
    {
        return fail(c, ACF_HIP_E_INVALID, "no detections (call acf_hip_detect)");
    }
    if (!c->countsFetched)
    {
        HIPCHK(c, hipMemcpyAsync(c->h_counts.data(), nmsActive(c) ? c->d_nmsCounts : c->cs.d_counts, sizeof(int32_t) * c->lastBatch, hipMemcpyDeviceToHost, c->stream));
        HIPCHK(c, hipStreamSynchronize(c->stream));
        c->countsFetched = true;
    }
    return ACF_HIP_OK;
}

// raw (pre-NMS) count of one frame of the last batch
static int rawCount(acf_hip_ctx* c, int frame, int* n)
{
    if (!nmsActive(c))
    {
        *n = c->h_counts[frame];
        return ACF_HIP_OK;
    }
    int32_t v = 0;
    HIPCHK(c, hipMemcpyAsync(&v, c->cs.d_counts + frame, sizeof(v), hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    *n = v;
    return ACF_HIP_OK;
}

enum RecordList
{
    REC_DETECTIONS, // the detections, after the device NMS when it is on
    REC_RAW,        // the detections before the device NMS
    REC_HITS        // the hits behind REC_DETECTIONS, one per detection
};

// One frame's list of the last batch: *count = its length, at most min(cap, max_hits) records into out
static int readRecords(acf_hip_ctx* c, int frame, RecordList which, void* out, int cap, int* count)
{
    static const char* const entry[] = { "get_detections", "get_raw_detections", "get_hits" };
    static const char* const frameText[] = { "get_detections: frame index", "get_raw_detections: frame index", "get_hits: frame index" };
    return onFrameOwner(c, frame, frameText[which], [&](acf_hip_ctx* c, int frame) -> int {
        if (int rc = needPlanRead(c, entry[which])) return rc;
        int rc = fetchCounts(c);
        if (rc)
        {
            return rc;
        }
        if (frame < 0 || frame >= c->lastBatch)
        {
            return fail(c, ACF_HIP_E_INVALID, frameText[which]);
        }
        int n = c->h_counts[frame];
        if (which == REC_RAW && (rc = rawCount(c, frame, &n)))
        {
            return rc;
        }
        if (n < 0) // (k_nms's count for a frame with more than NMS_CAP detections; a raw count is never negative)
        {
            return fail(c, ACF_HIP_E_CAPACITY, "more than ACF_HIP_NMS_CAP detections into the device NMS: take the raw list (acf_hip_get_raw_detections) and suppress it on the host");
        }
        if (which == REC_HITS && nmsActive(c))
        {
            // hit i belongs to detection i of acf_hip_get_detections: the survivors' entries of the raw list, through k_nms's keep indices
            if (n > c->maxHits)
            {
                return fail(c, ACF_HIP_E_CAPACITY, "more hits than max_hits; re-plan with a larger capacity");
            }
            if (count)
            {
                *count = n;
            }
            const int m = std::min(n, cap);
            if (m > 0 && out)
            {
                int nRaw = 0;
                if ((rc = rawCount(c, frame, &nRaw)))
                {
                    return rc;
                }
                nRaw = std::min(nRaw, c->maxHits);
                std::vector<int32_t> keep(static_cast<size_t>(m));
                std::vector<acf_hip_hit> raw(static_cast<size_t>(std::max(nRaw, 1)));
                HIPCHK(c, hipMemcpy(keep.data(), c->d_nmsKeep + size_t(frame) * NMS_CAP, sizeof(int32_t) * m, hipMemcpyDeviceToHost));
                HIPCHK(c, hipMemcpy(raw.data(), c->cs.d_sorted + size_t(frame) * c->maxHits, sizeof(acf_hip_hit) * nRaw, hipMemcpyDeviceToHost));
                for (int i = 0; i < m; i++)
                {
                    if (keep[size_t(i)] < 0 || keep[size_t(i)] >= nRaw)
                    {
                        return fail(c, ACF_HIP_E_INVALID, "get_hits: survivor index outside the raw list");
                    }
                    static_cast<acf_hip_hit*>(out)[i] = raw[size_t(keep[size_t(i)])];
                }
            }
            return ACF_HIP_OK;
        }
        if (count)
        {
            *count = n;
        }
        const int m = std::min(std::min(n, c->maxHits), cap);
        if (m > 0 && out)
        {
            const size_t at = size_t(frame) * c->maxHits, rec = which == REC_HITS ? sizeof(acf_hip_hit) : sizeof(acf_hip_detection);
            const void* src = which == REC_HITS ? static_cast<const void*>(c->cs.d_sorted + at)
                                                : (which == REC_DETECTIONS && nmsActive(c) ? c->d_nmsDets : c->cs.d_dets) + at;
            HIPCHK(c, hipMemcpy(out, src, rec * m, hipMemcpyDeviceToHost));
        }
        if (n > c->maxHits)
        {
            return fail(c, ACF_HIP_E_CAPACITY, "more hits than max_hits; re-plan with a larger capacity");
        }
        return ACF_HIP_OK;
    });
}

int acf_hip_get_detections(acf_hip_ctx* c, int frame, acf_hip_detection* out, int cap, int* count)
{
    return readRecords(c, frame, REC_DETECTIONS, out, cap, count);
}

int acf_hip_get_raw_detections(acf_hip_ctx* c, int frame, acf_hip_detection* out, int cap, int* count)
{
    return readRecords(c, frame, REC_RAW, out, cap, count);
}

int acf_hip_get_hits(acf_hip_ctx* c, int frame, acf_hip_hit* out, int cap, int* count)
{
    return readRecords(c, frame, REC_HITS, out, cap, count);
}

int acf_hip_export_detections(acf_hip_ctx* c, int32_t* dst_dev, int cap)
{
    const bool parent = c && !c->kids.empty(); // (its children hold the plan's buffers and answer for the plan)
    if (!parent)
    {
        if (int rc = needPlanRead(c, "export_detections")) return rc;
    }
    if (!c->detectValid || !dst_dev || cap <= 0)
    {
        return fail(c, ACF_HIP_E_INVALID, "export_detections: nothing to export");
    }
    if (parent)
    {
        return forEachKid(c, c->lastBatch,
            [&](acf_hip_ctx* k, int first, int) { return acf_hip_export_detections(k, dst_dev + first * (1 + 6 * size_t(cap)), cap); });
    }
    HIPCHK(c, hipSetDevice(c->device));
    hipLaunchKernelGGL(k_export, dim3(cdiv(cap, 256), c->lastBatch), dim3(256), 0, c->stream,
        (const acf_hip_detection*)(nmsActive(c) ? c->d_nmsDets : c->cs.d_dets), (const int32_t*)(nmsActive(c) ? c->d_nmsCounts : c->cs.d_counts), c->maxHits, cap, dst_dev);
    LAUNCHCHK(c, "k_export");
    return ACF_HIP_OK;
}

int acf_hip_read_level(acf_hip_ctx* c, int frame, int level, float* host_out)
{
    return onFrameOwner(c, frame, "read_level: arguments", [&](acf_hip_ctx* c, int frame) -> int {
        if (int rc = needPlanRead(c, "read_level")) return rc;
        if (!c->pyramidValid || frame < 0 || frame >= c->lastBatch || level < 0 || level >= int(c->plan.levels.size()) || !host_out)
        {
            return fail(c, ACF_HIP_E_INVALID, "read_level: arguments");
        }
        if (!c->floatPyramid)
        {
            return fail(c, ACF_HIP_E_INVALID, "read_level: the float pyramid was not kept (option keep_pyramid = 0: the levels left as rank cells only)");
        }
        const acf_hip_level& l = c->plan.levels[level];
        HIPCHK(c, hipStreamSynchronize(c->stream));
        HIPCHK(c, hipMemcpy(host_out, c->d_pyr + size_t(frame) * c->plan.pyr_floats + l.offset, sizeof(float) * c->plan.nChns * l.hP * l.wP, hipMemcpyDeviceToHost));
        return ACF_HIP_OK;
    });
}

int acf_hip_read_rank_level(acf_hip_ctx* c, int frame, int level, uint16_t* host_out)
{
    return onFrameOwner(c, frame, "read_rank_level: arguments, or no detect since the last pyramid", [&](acf_hip_ctx* c, int frame) -> int {
        if (int rc = needPlanRead(c, "read_rank_level")) return rc;
        if (!rankCellsOn(c, c->cs))
        {
            return fail(c, ACF_HIP_E_UNSUPPORTED, "read_rank_level: the plan has no rank cells (model not depth 2 / thresholds too dense / option rank_cells off / LDCF)");
        }
        if (!c->pyramidValid || !c->ranksValid || frame < 0 || frame >= c->lastBatch || level < 0 || level >= int(c->plan.levels.size()) || !host_out)
        {
            return fail(c, ACF_HIP_E_INVALID, "read_rank_level: arguments, or no detect since the last pyramid");
        }
        const acf_hip_level& l = c->plan.levels[level];
        const int pitch = rankPitch(l.hP);
        int64_t off = 0;
        for (int i = 0; i < level; i++)
        {
            off += int64_t(c->plan.nChns) * rankPitch(c->plan.levels[i].hP) * c->plan.levels[i].wP;
        }
        HIPCHK(c, hipStreamSynchronize(c->stream));
        HIPCHK(c, hipMemcpy2D(host_out, size_t(l.hP) * 2, c->cs.d_pyrR + size_t(frame) * c->cs.pyrRCells + off, size_t(pitch) * 2, size_t(l.hP) * 2,
            size_t(c->plan.nChns) * l.wP, hipMemcpyDeviceToHost));
        return ACF_HIP_OK;
    });
}

int acf_hip_rank_cells_host(const acf_hip_params* p, int nChns, int chn, const float* v, int n, uint16_t* cells_out, uint32_t* thr_index_out, int32_t* info)
{
    if (!p || !p->fids || !p->thrs || nChns <= 0 || chn < 0 || chn >= nChns || n < 0 || (n > 0 && !v) || p->treeDepth <= 0 || p->shrink <= 0)
    {
        return ACF_HIP_E_INVALID;
    }
    const int mH = p->modelDsPad_h / p->shrink, mW = p->modelDsPad_w / p->shrink;
    if (mH <= 0 || mW <= 0)
    {
        return ACF_HIP_E_INVALID;
    }
    const size_t nNodes = size_t(p->nTrees) * p->nTreeNodes;
    std::vector<int32_t> chnOfNode(nNodes, -1);
    for (int t = 0; t < p->nTrees; t++)
    {
        for (int k = 0; k < (1 << p->treeDepth) - 1 && k < p->nTreeNodes; k++)
        {
            const size_t q = size_t(t) * p->nTreeNodes + k;
            chnOfNode[q] = int32_t(p->fids[q] / uint32_t(mW * mH));
        }
    }
    RankTables rt;
    buildRankTables(p->thrs, chnOfNode.data(), nNodes, nChns, rt);
    if (info)
    {
        info[0] = rt.ok ? 1 : 0;
        info[1] = rt.ok ? rt.chan[size_t(chn)].shift : 0;
        info[2] = rt.ok ? rt.chan[size_t(chn)].nb : 0;
        info[3] = rt.ok ? rt.chan[size_t(chn)].nThr : 0;
    }
    if (!rt.ok)
    {
        return ACF_HIP_E_UNSUPPORTED;
    }
    for (int i = 0; i < n && cells_out; i++)
    {
        cells_out[i] = uint16_t(rt.rankOfCell(chn, v[i]));
    }
    for (size_t q = 0; q < nNodes && thr_index_out; q++)
    {
        thr_index_out[q] = chnOfNode[q] >= 0 ? rt.rankOfThreshold(chnOfNode[q], p->thrs[q]) : 0u;
    }
    return ACF_HIP_OK;
}

// the plane of a real scale that a one-plane tap reads (M, O, S, Mnorm); null for every other tap
static float* RealScale::*tapPlane(int tap)
{
    switch (tap)
    {
        case ACF_HIP_TAP_M: return &RealScale::M;
        case ACF_HIP_TAP_O: return &RealScale::O;
        case ACF_HIP_TAP_S: return &RealScale::S;
        case ACF_HIP_TAP_MNORM: return &RealScale::Mn;
        default: return nullptr;
    }
}

int acf_hip_read_tap(acf_hip_ctx* c, int frame, int tap, int index, float* host_out, int64_t cap)
{
    return onFrameOwner(c, frame, "read_tap: arguments", [&](acf_hip_ctx* c, int frame) -> int {
        if (int rc = needPlanRead(c, "read_tap")) return rc;
        if (!c->pyramidValid || frame < 0 || frame >= c->lastBatch || !host_out)
        {
            return fail(c, ACF_HIP_E_INVALID, "read_tap: arguments");
        }
        const Plan& pl = c->plan;
        const float* src = nullptr;
        int64_t n = 0;
        if (tap == ACF_HIP_TAP_LDCF)
        {
            if (c->p.ldcfK <= 0 || !c->detectValid || index < 0 || index >= int(c->ldcf.levels.size()))
            {
                return fail(c, ACF_HIP_E_INVALID, "read_tap: LDCF levels exist after acf_hip_detect on a model with ldcfK > 0");
            }
            const acf_hip_level& l = c->ldcf.levels[size_t(index)];
            n = int64_t(pl.nChns) * c->p.ldcfK * l.hP * l.wP;
            src = c->ldcf.d_pyr + size_t(frame) * c->ldcf.floats + l.offset;
        }
        else if (tap == ACF_HIP_TAP_CHNS)
        {
            if (index < 0 || index >= int(pl.levels.size()))
            {
                return fail(c, ACF_HIP_E_INVALID, "read_tap: level");
            }
            const acf_hip_level& l = pl.levels[index];
            n = int64_t(pl.nChns) * l.hC * l.wC;
            src = c->d_chns + size_t(frame) * pl.raw_floats + pl.raw_off[index];
        }
        else
        {
            if (index < 0 || index >= int(c->real.size()))
            {
                return fail(c, ACF_HIP_E_INVALID, "read_tap: real-scale ordinal");
            }
            const RealScale& rs = c->real[index];
            const int64_t np = int64_t(rs.h) * rs.w;
            float* RealScale::*const plane = tapPlane(tap);
            if (pl.d_in == 5 && index == 0 && plane)
            {
                // chnsCompute.cpp:265-269: M and O came with the frame; nothing was computed here, and the reference logs none of them
                return fail(c, ACF_HIP_E_INVALID, "read_tap: M, O, S and Mnorm of the first real scale came with the five-plane frame (none computed)");
            }
            switch (tap)
            {
                case ACF_HIP_TAP_IMAGE:
                    n = np * pl.d;
                    if (rs.resampled)
                    {
                        src = rs.img + size_t(frame) * n;
                    }
                    else if (c->d_color)
                    {
                        src = c->d_color + size_t(frame) * n;
                    }
                    else
                    {
                        src = c->lastFrames + size_t(frame) * pl.d_in * np; // (the caller's frames: d_in planes a frame, M and O behind the image's)
                    }
                    break;
                case ACF_HIP_TAP_SMOOTHED:
                    n = np * pl.d;
                    src = rs.sm + size_t(frame) * n;
                    break;
                default:
                    if (!plane)
                    {
                        return fail(c, ACF_HIP_E_INVALID, "read_tap: unknown tap");
                    }
                    n = np;
                    src = rs.*plane ? rs.*plane + size_t(frame) * n : nullptr;
            }
            if (!src)
            {
                return fail(c, ACF_HIP_E_INVALID, "read_tap: tap not kept (set option \"taps\" before acf_hip_plan)");
            }
        }
        if (cap < n)
        {
            return fail(c, ACF_HIP_E_INVALID, "read_tap: capacity");
        }
        HIPCHK(c, hipStreamSynchronize(c->stream));
        HIPCHK(c, hipMemcpy(host_out, src, sizeof(float) * n, hipMemcpyDeviceToHost));
        return ACF_HIP_OK;
    });
}

// Times and launch counts by kernel name, in the order the names first appear.
struct ProfileTotals
{
    std::vector<const char*> names;
    std::vector<float> ms;
    std::vector<int> launches;
    void add(const char* name, float t, int n)
    {
        size_t j = 0;
        while (j < names.size() && strcmp(names[j], name))
        {
            j++;
        }
        if (j == names.size())
        {
            names.push_back(name);
            ms.push_back(0.f);
            launches.push_back(0);
        }
        ms[j] += t;
        launches[j] += n;
    }
    // acf_hip_profile_get's outputs: *n = the number of names, the first min(*n, cap) entries into the arrays that are not null
    void write(int* n, const char** namesOut, float* msOut, int* launchesOut, int cap) const
    {
        *n = int(names.size());
        for (size_t i = 0; i < names.size() && int(i) < cap; i++)
        {
            if (namesOut) namesOut[i] = names[i];
            if (msOut) msOut[i] = ms[i];
            if (launchesOut) launchesOut[i] = launches[i];
        }
    }
};

int acf_hip_profile_get(acf_hip_ctx* c, int* n, const char** names, float* ms, int* launches, int cap)
{
    if (!c || !n)
    {
        return ACF_HIP_E_INVALID;
    }
    ProfileTotals tot;
    if (!c->kids.empty())
    {
        // sum over the sub-batch contexts (their kernels overlap in time: the sum exceeds the wall clock)
        for (acf_hip_ctx* k : c->kids)
        {
            int kn = 0;
            const char* knames[64];
            float kms[64];
            int kl[64];
            int rc = acf_hip_profile_get(k, &kn, knames, kms, kl, 64);
            if (rc)
            {
                return fail(c, rc, k->err);
            }
            for (int i = 0; i < std::min(kn, 64); i++)
            {
                tot.add(knames[i], kms[i], kl[i]);
            }
        }
        tot.write(n, names, ms, launches, cap);
        return ACF_HIP_OK;
    }
    HIPCHK(c, hipStreamSynchronize(c->stream)); // (the side streams were joined into it)
    for (size_t i = 0; i + 1 < c->evUsed; i++)
    {
        const acf_hip_ctx::ProfMark& m = c->evPool[i];
        if (!strcmp(m.name, "(end)"))
        {
            continue;
        }
        // the kernel ends where the next event of the same stream was recorded (real scales run on their own streams)
        size_t j = i + 1;
        while (j < c->evUsed && c->evPool[j].stream != m.stream)
        {
            j++;
        }
        float dt = 0;
        if (j < c->evUsed && hipEventElapsedTime(&dt, m.ev, c->evPool[j].ev) == hipSuccess)
        {
            tot.add(m.name, dt, 1);
        }
    }
    c->evUsed = 0;
    // the bank's members ran on this context's stream, each under its own markers
    for (acf_hip_ctx* m : c->bankCtx)
    {
        int kn = 0;
        const char* knames[64];
        float kms[64];
        int kl[64];
        if (const int rc = acf_hip_profile_get(m, &kn, knames, kms, kl, 64))
        {
            return fail(c, rc, m->err);
        }
        for (int i = 0; i < std::min(kn, 64); i++)
        {
            tot.add(knames[i], kms[i], kl[i]);
        }
    }
    tot.write(n, names, ms, launches, cap);
    return ACF_HIP_OK;
}
