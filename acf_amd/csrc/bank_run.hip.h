// bank_run.hip.h — part of acf_hip.hip (included there and nowhere else): a bank of classifiers on one pyramid (the header's "a bank of
// classifiers" section; kernel k_join_bank, kernels_bank.hip.h).
//   bankCheck                what a member must share with the primary, and what acf_hip_check_model asks of it (acf_hip_bank_check)
//   acf_hip_set_bank         the members' parameters and arrays into the context (ModelState::bank); drops the plan
//   planBank                 acf_hip_plan's last stage: a context per member (acf_hip_ctx::bankCtx) with the member as its model and,
//                            over the plan's levels, the member's window grid, cascade tables, run buffers and box table; no x86
//                            tables and no pyramid of its own
//   acf_hip_detect_bank      runCascade on every member's state over the owner's float pyramid, on the owner's stream
//   bankModel / the get_bank_* entries   a model index to the context that holds its list, read through readRecords
//   joinChecked / launchJoin / acf_hip_join_bank / acf_hip_op_join_bank   the join, as merge_run.hip.h lays out the merge
// A member's context never builds a pyramid and never swaps a field of its owner: the cascade is handed the member's state and the
// owner's cells.  The join allocates nothing, never waits for the device and changes nothing acf_hip_run left behind.
#pragma once

namespace
{

const size_t kJoinLds = size_t(NMS_CAP) * (8 + 16 + 4 + 1 + 1); // (k_nms's + the model bytes; the offsets are the kernel's own static LDS)

int bankCheck(const acf_hip_params& a, const acf_hip_params& b, std::string& why)
{
    if (a.ldcfK > 0 || b.ldcfK > 0)
    {
        why = "LDCF models (ldcfK > 0) take no bank";
        return ACF_HIP_E_UNSUPPORTED;
    }
    // Options::Pyramid and Options::Pyramid::Chns: one pyramid serves every model
#define ACF_BANK_SAME(field)                                                   \
    if (!(a.field == b.field))                                                 \
    {                                                                          \
        why = "the member's " #field " differs from the primary's (one pyramid serves every model)"; \
        return ACF_HIP_E_INVALID;                                              \
    }
    ACF_BANK_SAME(nPerOct)
    ACF_BANK_SAME(nOctUp)
    ACF_BANK_SAME(nApprox)
    ACF_BANK_SAME(nLambdas)
    for (int i = 0; i < 3 && i < a.nLambdas; i++)
    {
        ACF_BANK_SAME(lambdas[i])
    }
    ACF_BANK_SAME(pad_h)
    ACF_BANK_SAME(pad_w)
    ACF_BANK_SAME(minDs_h)
    ACF_BANK_SAME(minDs_w)
    ACF_BANK_SAME(smooth)
    ACF_BANK_SAME(shrink)
    ACF_BANK_SAME(colorEnabled)
    ACF_BANK_SAME(colorSmooth)
    ACF_BANK_SAME(colorSpace)
    ACF_BANK_SAME(gradMagEnabled)
    ACF_BANK_SAME(colorChn)
    ACF_BANK_SAME(normRad)
    ACF_BANK_SAME(normConst)
    ACF_BANK_SAME(full)
    ACF_BANK_SAME(gradHistEnabled)
    ACF_BANK_SAME(binSize)
    ACF_BANK_SAME(nOrients)
    ACF_BANK_SAME(softBin)
    ACF_BANK_SAME(isLuv)
#undef ACF_BANK_SAME
    if (b.nOrients < 1 || b.nOrients > 12)
    {
        why = "nOrients must be 1..12";
        return ACF_HIP_E_UNSUPPORTED;
    }
    return checkModel(b, numChannels(b), b.shrink, why);
}

} // namespace

int acf_hip_bank_check(const acf_hip_params* primary, const acf_hip_params* member, char* why, int cap)
{
    std::string err;
    int rc = ACF_HIP_E_INVALID;
    if (!primary || !member)
    {
        err = "bank_check: arguments";
    }
    else
    {
        rc = bankCheck(*primary, *member, err);
    }
    if (why && cap > 0)
    {
        std::snprintf(why, size_t(cap), "%s", err.c_str());
    }
    return rc;
}

int acf_hip_set_bank(acf_hip_ctx* c, const acf_hip_params* members, int n)
{
    if (int rc = needModel(c, "set_bank")) return rc;
    if (n < 0 || n > ACF_HIP_BANK_MAX || (n > 0 && !members))
    {
        return fail(c, ACF_HIP_E_INVALID, "set_bank: 0 .. ACF_HIP_BANK_MAX members");
    }
    n = members ? n : 0;
    std::vector<ModelState::BankMember> bank(static_cast<size_t>(n));
    for (int i = 0; i < n; i++)
    {
        std::string why;
        if (const int rc = bankCheck(c->p, members[i], why))
        {
            return fail(c, rc, "set_bank: member " + std::to_string(i) + ": " + why); // (a refused bank leaves the context as it was)
        }
        ModelState::BankMember& m = bank[size_t(i)];
        const acf_hip_params& p = members[i];
        const size_t nodes = size_t(p.nTrees) * p.nTreeNodes;
        m.p = p;
        m.fids.assign(p.fids, p.fids + nodes);
        m.thrs.assign(p.thrs, p.thrs + nodes);
        m.hs.assign(p.hs, p.hs + nodes);
        if (p.child)
        {
            m.child.assign(p.child, p.child + nodes);
        }
        m.p.ldcfK = 0;
        m.p.ldcfFilters = nullptr;
    }
    dropGraph(c); // (behind the checks: a refused bank leaves a captured graph as well)
    c->bank.swap(bank);
    for (auto& m : c->bank) // (after the swap: the vectors' storage does not move with them, the struct's does)
    {
        m.p.fids = m.fids.data();
        m.p.thrs = m.thrs.data();
        m.p.hs = m.hs.data();
        m.p.child = m.child.empty() ? nullptr : m.child.data();
    }
    if (c->hasPlan)
    {
        HIPCHK(c, hipSetDevice(c->device));
        (void)hipStreamSynchronize(c->stream);
        (void)acf_hip_stream_close(c);
        dropPlan(c); // (its members' states were built for the previous bank)
    }
    return ACF_HIP_OK;
}

// acf_hip_plan's last stage on a context that holds the plan's buffers: per member what PlanBuild::cascade builds for the primary
static int planBank(acf_hip_ctx* c, int max_batch, int max_hits)
{
    for (const auto& bm : c->bank)
    {
        acf_hip_ctx* m = nullptr;
        int rc;
        if ((rc = acf_hip_create(c->device, c->stream, &m)))
        {
            return fail(c, rc, "plan: cannot create a bank member's context");
        }
        c->bankCtx.push_back(m); // (from here on dropPlan frees it)
        m->numCus = c->numCus;
        m->ldsPerCu = c->ldsPerCu;
        m->opt = c->opt; // (the x86 tables stay the owner's alone: the cascade evaluates none of the approximate sites)
        if ((rc = acf_hip_set_model(m, &bm.p)))
        {
            return fail(c, rc, "plan: bank member: " + m->err);
        }
        // the plan's geometry with the member's window grid (buildPlan's formula)
        const acf_hip_params& p = m->p;
        m->plan = c->plan;
        for (acf_hip_level& l : m->plan.levels)
        {
            l.nWinR = std::max(0, int(std::ceil(float(l.hP * p.shrink - p.modelDsPad_h + 1) / p.stride)));
            l.nWinC = std::max(0, int(std::ceil(float(l.wP * p.shrink - p.modelDsPad_w + 1) / p.stride)));
        }
        m->maxBatch = max_batch;
        m->maxHits = max_hits;
        const Plan& pl = m->plan;
        if ((rc = buildCascadeTables(m, pl.levels, pl.nChns, p.shrink, max_batch, m->thrs, m->cs, true)) ||
            (rc = allocCascadeRun(m, m->cs, pl.levels, m->thrs, max_hits)))
        {
            return fail(c, rc, "plan: bank member: " + m->err);
        }
        std::vector<BoxLevel> box(pl.levels.size());
        for (size_t i = 0; i < pl.levels.size(); i++)
        {
            box[i].shw_h = pl.levels[i].scalehw_h;
            box[i].shw_w = pl.levels[i].scalehw_w;
            box[i].bh = int(std::lrint(double(p.modelDs_h) / pl.levels[i].scale)); // (as PlanBuild::cascade)
            box[i].bw = int(std::lrint(double(p.modelDs_w) / pl.levels[i].scale));
        }
        if ((rc = devUpload(m, &m->d_boxLevels, box)))
        {
            return fail(c, rc, "plan: bank member: " + m->err);
        }
        m->h_counts.assign(size_t(max_batch), 0);
        m->hasPlan = true;
    }
    return ACF_HIP_OK;
}

int acf_hip_detect_bank(acf_hip_ctx* c)
{
    if (int rc = needCtx(c)) return rc;
    const std::string who = "detect_bank: ";
    if (!c->kids.empty() || c->nStreams > 1)
    {
        return fail(c, ACF_HIP_E_UNSUPPORTED, who + "not available with option \"streams\" > 1");
    }
    if (c->bank.empty())
    {
        return fail(c, ACF_HIP_E_INVALID, who + "no bank (call acf_hip_set_bank)");
    }
    if (!c->hasPlan || c->bankCtx.size() != c->bank.size())
    {
        return fail(c, ACF_HIP_E_INVALID, who + "no plan (call acf_hip_plan after acf_hip_set_bank)");
    }
    if (!c->pyramidValid)
    {
        return fail(c, ACF_HIP_E_INVALID, who + "no pyramid (call acf_hip_pyramid* or acf_hip_run* first)");
    }
    if (!c->floatPyramid)
    {
        return fail(c, ACF_HIP_E_INVALID, who + "the float pyramid of this batch was not written (option \"keep_pyramid\" = 0): the members read it");
    }
    HIPCHK(c, hipSetDevice(c->device));
    const int nF = c->lastBatch;
    const CascInput in = { c->d_pyr, c->plan.pyr_floats, nF, c->plan.nChns };
    c->bankValid = false;
    for (acf_hip_ctx* m : c->bankCtx)
    {
        m->lastBatch = nF;
        m->detectValid = false;
        bool ranksWritten = false; // (the member's rank pyramid: its own k_rank launch writes it from the owner's floats)
        if (const int rc = runCascade(m, m->cs, in, m->d_boxLevels, &ranksWritten))
        {
            return fail(c, rc, who + m->err);
        }
        prof(m, m->stream, "(end)");
        m->countsFetched = false;
        m->pyramidValid = m->detectValid = true;
    }
    c->bankValid = true;
    return ACF_HIP_OK;
}

namespace
{

// model 0: the context itself; m >= 1: member m - 1 under the plan.  Null (with the text left on c): no such model
acf_hip_ctx* bankModel(const acf_hip_ctx* c, int model, const char* who)
{
    if (model == 0)
    {
        return const_cast<acf_hip_ctx*>(c);
    }
    if (model < 0 || size_t(model) > c->bankCtx.size())
    {
        (void)fail(c, ACF_HIP_E_INVALID, std::string(who) + ": model index (0 .. the bank's members under the plan)");
        return nullptr;
    }
    return c->bankCtx[size_t(model) - 1];
}

int bankRecords(acf_hip_ctx* c, const char* who, int model, int frame, RecordList which, void* out, int cap, int* count)
{
    if (int rc = needCtx(c)) return rc;
    acf_hip_ctx* m = bankModel(c, model, who);
    if (!m)
    {
        return ACF_HIP_E_INVALID;
    }
    if (m == c)
    {
        return readRecords(c, frame, which, out, cap, count);
    }
    if (!c->bankValid)
    {
        return fail(c, ACF_HIP_E_INVALID, std::string(who) + ": no lists of the bank (call acf_hip_detect_bank)");
    }
    const int rc = readRecords(m, frame, which, out, cap, count);
    return rc ? fail(c, rc, std::string(who) + ": " + m->err) : rc;
}

} // namespace

int acf_hip_get_bank_levels(const acf_hip_ctx* c, int model, acf_hip_level* out, int cap)
{
    if (int rc = needPlanRead(c, "get_bank_levels")) return rc;
    const acf_hip_ctx* m = bankModel(c, model, "get_bank_levels");
    if (!m)
    {
        return ACF_HIP_E_INVALID;
    }
    if (!out || cap < int(m->plan.levels.size()))
    {
        return fail(c, ACF_HIP_E_INVALID, "get_bank_levels: capacity");
    }
    std::copy(m->plan.levels.begin(), m->plan.levels.end(), out);
    return ACF_HIP_OK;
}

int acf_hip_get_bank_detections(acf_hip_ctx* c, int model, int frame, acf_hip_detection* out, int cap, int* count)
{
    return bankRecords(c, "get_bank_detections", model, frame, REC_RAW, out, cap, count);
}

int acf_hip_get_bank_hits(acf_hip_ctx* c, int model, int frame, acf_hip_hit* out, int cap, int* count)
{
    return bankRecords(c, "get_bank_hits", model, frame, REC_HITS, out, cap, count);
}

int acf_hip_get_bank_forms(const acf_hip_ctx* c, int model, int32_t* out, int cap, int* n)
{
    if (int rc = needCtx(c)) return rc;
    const acf_hip_ctx* m = bankModel(c, model, "get_bank_forms");
    if (!m)
    {
        return ACF_HIP_E_INVALID;
    }
    return acf_hip_get_cascade_forms(m, out, cap, n);
}

namespace
{

const char* joinSpecBad(const acf_hip_bank_spec* s)
{
    if (!s)
    {
        return "null spec";
    }
    const acf_hip_merge_spec ms = { s->nms, s->max_per_frame, s->grow, { s->reserved[0], s->reserved[1] } };
    if (const char* bad = mergeSpecBad(&ms))
    {
        return bad;
    }
    if (s->separate != 0 && s->separate != 1)
    {
        return "separate must be 0 or 1";
    }
    if (!(s->det_scale >= 0) || !std::isfinite(s->det_scale))
    {
        return "det_scale must be 0 (no resize) or a positive finite number";
    }
    return nullptr;
}

// what a call states, checked on the host: the refusal, or the kernel's arguments without its lists and outputs
int joinChecked(acf_hip_ctx* c, const std::string& who, const acf_hip_bank_spec* spec, const void* out, const void* countsOut, JoinArgs& a)
{
    if (!out || !countsOut)
    {
        return fail(c, ACF_HIP_E_INVALID, who + "null records or counts");
    }
    if (const char* bad = joinSpecBad(spec))
    {
        return fail(c, ACF_HIP_E_INVALID, who + bad);
    }
    if (!c->kids.empty())
    {
        return fail(c, ACF_HIP_E_UNSUPPORTED, who + "not available with option \"streams\" > 1");
    }
    a.type = spec->nms.type;
    a.ovrUnion = spec->nms.ovrDnmUnion != 0;
    a.doPrune = spec->nms.prune != 0;
    a.maxCount = spec->nms.maxCount;
    a.separate = spec->separate;
    a.overlap = spec->nms.overlap;
    a.thr = spec->nms.thr;
    a.pruneRatio = spec->nms.pruneRatio;
    a.K = spec->max_per_frame;
    a.inv = spec->det_scale == 0 ? 1.f : 1.f / float(spec->det_scale); // (acf_hip_crop_box's)
    a.grow = spec->grow;
    return ACF_HIP_OK;
}

int launchJoin(acf_hip_ctx* c, const JoinArgs& a)
{
    HIPCHK(c, hipSetDevice(c->device));
    prof(c, c->stream, "k_join_bank");
    hipLaunchKernelGGL(k_join_bank, dim3(unsigned(a.nFrames)), dim3(1024), kJoinLds, c->stream, a);
    LAUNCHCHK(c, "k_join_bank");
    prof(c, c->stream, "(end)");
    return ACF_HIP_OK;
}

} // namespace

int acf_hip_join_bank(acf_hip_ctx* c, const acf_hip_bank_spec* spec, acf_hip_bank_detection* out, int32_t* countsOut, float* boxesOut, int32_t* framesOut)
{
    if (int rc = needCtx(c)) return rc;
    const std::string who = "join_bank: ";
    JoinArgs a{};
    if (int rc = joinChecked(c, who, spec, out, countsOut, a)) return rc;
    if (!c->hasPlan || !c->detectValid || !c->bankValid || c->bankCtx.empty())
    {
        return fail(c, ACF_HIP_E_INVALID, who + "no lists to join (call acf_hip_run* and acf_hip_detect_bank first)");
    }
    a.nModels = 1 + int(c->bankCtx.size());
    a.nFrames = c->lastBatch;
    a.maxHits = c->maxHits;
    a.dets[0] = c->cs.d_dets; // (the raw list, whether or not the device NMS is on)
    a.counts[0] = c->cs.d_counts;
    for (size_t i = 0; i < c->bankCtx.size(); i++)
    {
        a.dets[i + 1] = c->bankCtx[i]->cs.d_dets;
        a.counts[i + 1] = c->bankCtx[i]->cs.d_counts;
    }
    a.out = out;
    a.countsOut = countsOut;
    a.boxesOut = boxesOut;
    a.framesOut = framesOut;
    return launchJoin(c, a);
}

int acf_hip_op_join_bank(acf_hip_ctx* c, const acf_hip_detection* dets, const int32_t* counts, int nModels, int nFrames, int maxHits,
    const acf_hip_bank_spec* spec, acf_hip_bank_detection* out, int32_t* countsOut, float* boxesOut, int32_t* framesOut)
{
    if (int rc = needCtx(c)) return rc;
    const std::string who = "op_join_bank: ";
    JoinArgs a{};
    if (int rc = joinChecked(c, who, spec, out, countsOut, a)) return rc;
    if (!dets || !counts || maxHits < 1 || nModels < 1 || nModels > BANK_MODELS_MAX || nFrames < 1)
    {
        return fail(c, ACF_HIP_E_INVALID, who + "null lists or counts, n_models outside 1 .. ACF_HIP_BANK_MAX + 1, n_frames < 1 or max_hits < 1");
    }
    const size_t slots = size_t(nFrames) * size_t(a.K), perModel = size_t(nFrames) * size_t(maxHits);
    if (slots > 0x7fffffffu / 4 || perModel * size_t(nModels) > 0x7fffffffu)
    {
        return fail(c, ACF_HIP_E_INVALID, who + "more than 2^31 - 1 list entries or output floats");
    }
    HIPCHK(c, hipSetDevice(c->device));
    Scratch s;
    const acf_hip_detection* dDets = s.upload(dets, perModel * size_t(nModels));
    const int32_t* dCounts = s.upload(counts, size_t(nModels) * size_t(nFrames));
    // (the caller's outputs go over first: a slot the kernel does not write keeps what the caller had there)
    a.out = s.upload(out, slots);
    a.countsOut = s.upload(countsOut, size_t(nFrames));
    a.boxesOut = boxesOut ? s.upload(boxesOut, slots * 4) : nullptr;
    a.framesOut = framesOut ? s.upload(framesOut, slots) : nullptr;
    if (!dDets || !dCounts || !a.out || !a.countsOut || (boxesOut && !a.boxesOut) || (framesOut && !a.framesOut))
    {
        (void)hipGetLastError();
        return fail(c, ACF_HIP_E_HIP, who + "device allocation or copy failed");
    }
    a.nModels = nModels;
    a.nFrames = nFrames;
    a.maxHits = maxHits;
    for (int m = 0; m < nModels; m++)
    {
        a.dets[m] = dDets + size_t(m) * perModel;
        a.counts[m] = dCounts + size_t(m) * size_t(nFrames);
    }
    int rc = launchJoin(c, a);
    if (rc || (rc = Scratch::download(c, "op_join_bank", out, a.out, slots)) || (rc = Scratch::download(c, "op_join_bank", countsOut, a.countsOut, size_t(nFrames))) ||
        (boxesOut && (rc = Scratch::download(c, "op_join_bank", boxesOut, a.boxesOut, slots * 4))) ||
        (framesOut && (rc = Scratch::download(c, "op_join_bank", framesOut, a.framesOut, slots))))
    {
        return rc;
    }
    return ACF_HIP_OK;
}
