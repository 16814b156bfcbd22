// pyramid_run.hip.h — part of acf_hip.hip (included there and nowhere else): acf_hip_pyramid's launch logic, one function per stage of
// Detector::chnsPyramid (chnsPyramid.cpp:160-456) in the order the reference runs them.  PyramidRun holds what the stages of ONE call
// share; every stage returns an ACF_HIP_* status.  The real scales' stages enqueue on PyramidRun::st and hand it to the launch helpers they
// call: the context's stream, or the scale's own between realScale and joinScales (option scale_streams).  c->stream itself is never reassigned;
// ingest and colour run on it before any scale has a stream of its own, the levels after joinScales has set st back to it.
//
//   ingest(plan)        the call's frames -> planar f32 as planIngest decided (input_run.hip.h): the preludes, then the ingest kernel
//   colour()            rgbConvert once at full resolution (chnsPyramid.cpp:230-263)
//   prepareScales()     which image every real scale is resampled from (the I = I1 adoption, :313-316), the scales' streams
//   realScale(k)        imageResample(k) -> planScale(k) -> smoothImage(k) -> gradientChannels(k): chnsCompute at a real scale (:297-338,
//                       chnsCompute.cpp:146-338)
//   joinScales()
//   levels(f0, n)       the approximated levels + final smoothing + padding of frames [f0, f0 + n) (:385-435): planLevels decides the forms
//                       (LevelsCall), launchLevels runs them for a frame offset
//   levelsWithImageLambdas()   the same behind the per-image lambda estimate (:341-374)
#pragma once

namespace
{
// How a real scale is computed, decided once after its image is there (PyramidRun::planScale); smoothImage and gradientChannels only read it
struct ScalePlan
{
    bool fuseSm = false;      // k_smooth_vec: smoothing + the level's colour channels from registers (colorDone), in column segments
    bool halfNext = false;    // ... + the next real scale's image, an exact half of this one
    uint32_t fullMask = 0;    // ... the planes whose full-resolution smoothed image is written
    bool wantGrad = false;    // ... the gradient plane's chain also emits gradMag (k_smooth_grad): M and O
    bool triXFused = false;   // ... and convTri's x pass: U (k_smooth_grad_tri)
    bool fuseCells = false;   // convTri's y pass may write the channel cells (k_triy_chns); else S is written and k_chns normalises
    bool blocked = false;     // M, O and U in 64 x 16 blocks (triPlan)
    bool ck = false;          // ... and no U: the x pass leaves checkpoints, k_triy_chns replays it (triPlan)
    bool needU = false;       // convTri runs in a form that reads the plane U
    ChnsArgs a{};             // the level's channel arguments (without the arith tables)
    int nt = 0, warm = 0;     // k_smooth_vec's threads, warm-up columns
    int nSeg = 1, segW = 0;   // column segments of the other planes' launch (and their width)
    int nSegG = 1, segWG = 0; // ... of the gradient plane's launch
    int segStride = 1;        // max(nSeg, nSegG): the hand-over state's segments
    size_t ldsB = 0, ldsG = 0; // LDS bytes of the two launches
};

// The instantiations of the pyramid's kernels.  (Each picker names them in the order the code object lists them.)
using SmoothVecKernel = void (*)(SmoothVecArgs, uint32_t);
using GradMagVecKernel = void (*)(const float*, float*, float*, const float*, int, int, int, int64_t, int64_t, int, int, const uint32_t*);
using LevelAllKernel = void (*)(const float*, float*, float*, const LevelJob*, const ResampleDesc*, const int32_t*, const float*, int, int64_t, int64_t, float,
    float*, int, LevelRankArgs, LevelSegArgs);
using LevelKernel = void (*)(const float*, float*, float*, const LevelJob*, const ResampleDesc*, const int32_t*, const float*, int, int64_t, int64_t, float,
    float*, int);

// How the levels stage runs, decided once per call (PyramidRun::planLevels); launchLevels and its launchers only read it
enum LevelsPath
{
    LV_FUSED,       // k_level_all + k_level groups resample, smooth and place every level
    LV_WAVE_SMOOTH, // the same kernels smooth and place what a separate k_resample approximated
    LV_SMOOTH_JOBS, // launchSmooth over the final jobs
    LV_COPY         // no smoothing: plane copies
};
struct LevelsCall
{
    LevelsPath path = LV_COPY;
    int nLF = 0;               // frames per launch
    bool approxFirst = false;  // the approximated levels come from a k_resample launch of their own
    bool pad = false;          // k_pad_reflect runs
    float pS = 0.f;            // convTri1's p of the final smoothing
    int64_t copyElems = 0;     // LV_COPY: the largest level's elements
    // LV_FUSED / LV_WAVE_SMOOTH
    const LevelJob* jobs = nullptr;                   // the leading nAll go to k_level_all, the rest to k_level in groups
    const std::vector<acf_hip_ctx::LevelGroup>* groups = nullptr;
    int nAll = 0;
    size_t nSide = 0;          // side streams the groups fan out to (0: they follow on the stage's stream)
    bool rawOut = false;       // option taps: the approximated levels' raw channels are written back too
    bool emitRank = false, emitF32 = true; // what the levels leave: the cascade's 16-bit rank cells, floats
    LevelRankArgs ra{};        // (without the frame's output pointer)
    LevelSegArgs lsa{};        // column segments (nSeg, warm-up) of k_level_all's first launch
    size_t ldsL = 0;
    LevelAllKernel allKernel = nullptr;
    bool lvTurns = false;      // option cascade_turns: k_level_all takes turns with the other contexts' (chain lvChain)
    int lvChain = 1;
};

static SmoothVecKernel smoothGradKernel(bool tri, bool half, bool x86, bool ck)
{
    if (tri && ck)
    {
        if (!x86)
        {
            return half ? k_smooth_grad_tri<true, false, true> : k_smooth_grad_tri<false, false, true>;
        }
        return half ? k_smooth_grad_tri<true, true, true> : k_smooth_grad_tri<false, true, true>;
    }
    if (!x86)
    {
        if (!tri)
        {
            return half ? k_smooth_grad<true, false> : k_smooth_grad<false, false>;
        }
        return half ? k_smooth_grad_tri<true, false> : k_smooth_grad_tri<false, false>;
    }
    if (!tri)
    {
        return half ? k_smooth_grad<true, true> : k_smooth_grad<false, true>;
    }
    return half ? k_smooth_grad_tri<true, true> : k_smooth_grad_tri<false, true>;
}

static SmoothVecKernel smoothVecKernel(bool half)
{
    return half ? k_smooth_vec<true> : k_smooth_vec<false>;
}

static GradMagVecKernel gradMagVecKernel(bool blocked, bool x86)
{
    if (blocked)
    {
        return x86 ? k_grad_mag_vec<true, true> : k_grad_mag_vec<true, false>;
    }
    return x86 ? k_grad_mag_vec<false, true> : k_grad_mag_vec<false, false>;
}

// rankNeg: the model holds a zero threshold (RankTables::hasZero): the rank forms that put negative cells below it
static LevelAllKernel levelAllKernel(bool f32, bool rank, bool rankNeg, bool segmented)
{
    if (rank && rankNeg)
    {
        if (f32)
        {
            return segmented ? k_level_all<LO_F32 | LO_RANK | LO_RANK_NEG, 1> : k_level_all<LO_F32 | LO_RANK | LO_RANK_NEG, 0>;
        }
        return segmented ? k_level_all<LO_RANK | LO_RANK_NEG, 1> : k_level_all<LO_RANK | LO_RANK_NEG, 0>;
    }
    if (f32 && rank)
    {
        return segmented ? k_level_all<LO_F32 | LO_RANK, 1> : k_level_all<LO_F32 | LO_RANK, 0>;
    }
    if (rank)
    {
        return segmented ? k_level_all<LO_RANK, 1> : k_level_all<LO_RANK, 0>;
    }
    return segmented ? k_level_all<LO_F32, 1> : k_level_all<LO_F32, 0>;
}

// null: R rows per lane are not instantiated for the mode
static LevelKernel levelKernel(int R, int mode)
{
#define LEVEL_R(RR)                                 \
    switch (mode)                                   \
    {                                               \
        case LM_REAL: return k_level<RR, LM_REAL>;  \
        case LM_DD: return k_level<RR, LM_DD>;      \
        default: return k_level<RR, LM_UU>;         \
    }
    switch (R)
    {
        case 1: LEVEL_R(1)
        case 2: LEVEL_R(2)
        case 3: LEVEL_R(3)
        case 4: LEVEL_R(4)
        case 5: LEVEL_R(5)
        case 6: LEVEL_R(6)
        case 7: LEVEL_R(7)
        case 8: LEVEL_R(8)
        default:
            // nine rows per lane: the full-resolution level of a 4K frame (540 cells); a real level's copy + smoothing only
            return R == LEVEL_MAX_R_REAL && mode == LM_REAL ? k_level<9, LM_REAL> : nullptr;
    }
#undef LEVEL_R
}

// option count_repairs: the n planes a verify kernel judged (its flags at d_flags) into c->repairs[slot], those it flagged into [slot + 1]
static int countRepairs(acf_hip_ctx* c, hipStream_t st, const int32_t* d_flags, size_t n, int slot)
{
    if (!c->opt.countRepairs)
    {
        return ACF_HIP_OK;
    }
    std::vector<int32_t> fl(n);
    HIPCHK(c, hipMemcpyAsync(fl.data(), d_flags, n * 4, hipMemcpyDeviceToHost, st));
    HIPCHK(c, hipStreamSynchronize(st));
    c->repairs[slot] += int64_t(n);
    for (int32_t v : fl)
    {
        c->repairs[slot + 1] += v != 0;
    }
    return ACF_HIP_OK;
}

struct PyramidRun
{
    acf_hip_ctx* const c;
    const acf_hip_params& p;
    const Plan& pl;
    const int nF;
    const int H, W, d, d_in, shrink;
    const int64_t np0;
    const float* frames;                          // planar f32 input planes (null once the 8-bit ingest has converted them itself)
    const float* cur = nullptr;                   // "I" of chnsPyramid: the image the next real scale is resampled from
    int64_t cur_fs = 0;
    int curH = 0, curW = 0;
    float pColor = 0.f;
    std::vector<int> srcIdx;                      // per real scale: the real scale whose smoothed image it is resampled from (-1: the frame)
    std::vector<char> halfDone, pairDone;         // the scale's image was produced already (by the previous scale's smoothing / its strip pair)
    bool scalePar = false;                        // the real scales on their own streams
    hipStream_t st;                               // the stream the current stage enqueues on: the context's, but a real scale's own between realScale and joinScales
    LevelsCall lv;                                // the levels stage of this call (planLevels)

    PyramidRun(acf_hip_ctx* ctx, const float* frames_, int nF_)
        : c(ctx), p(ctx->p), pl(ctx->plan), nF(nF_), H(pl.H), W(pl.W), d(pl.d), d_in(pl.d_in), shrink(ctx->p.shrink), np0(int64_t(pl.H) * pl.W), frames(frames_),
          st(ctx->stream)
    {
    }

    int ingest(const IngestPlan& ip);
    int colour(bool ingestConverted);
    int prepareScales();
    int realScale(size_t k);
    int imageResample(size_t k, const float*& img, int64_t& img_fs);
    ScalePlan planScale(size_t k, const float* img, int64_t img_fs);
    int smoothImage(size_t k, const float* img, int64_t img_fs, const ScalePlan& sp);
    int gradientChannels(size_t k, const ScalePlan& sp);
    int joinScales();
    int planLevels(int nLF);
    void noteLevelForms();
    int levels(int f0, int nLF);
    int launchLevels(const LevelsCall& lc, int f0);
    int launchLevelAll(const LevelsCall& lc, int f0);
    int launchLevelGroups(const LevelsCall& lc, int f0);
    int padLevels(const LevelsCall& lc, int f0);
    int levelsWithImageLambdas();
};

// ---- the ingest planIngest decided: its preludes, then the kernel, to the destination the plan names
int PyramidRun::ingest(const IngestPlan& ip)
{
    int rc;
    if ((ip.toRgb && (rc = launchYuvToRgb(c, ip.toRgbSrc, nF, c->d_yuvRgb))) ||
        (ip.resize && (rc = launchResizeU8(c, c->rz, ip.resizeSrc, ip.resizeCpp, ip.resizeStride, nF, c->rz.d_out))))
    {
        return rc;
    }
    prof(c, c->stream, ip.profName);
    if (!ip.convert && !c->d_stage && (rc = devAlloc(c, &c->d_stage, size_t(c->maxBatch) * d_in * np0)))
    {
        return rc;
    }
    IngestArgs a{};
    ingestShared(c, ip.convert ? c->d_color : c->d_stage, int64_t(ip.convert ? d : d_in) * np0, ip.nOut, a);
    a.in = ip.in;
    a.cpp = ip.g.cpp;
    a.ro = ip.g.ro;
    a.go = ip.g.go;
    a.bo = ip.g.bo;
    a.rowStride = ip.g.stride;
    a.in_fs = ip.g.frameStride;
    void* args[] = { &a, const_cast<IngestPlan::Second*>(&ip.second) };
    (void)hipLaunchKernel(ip.kernel, dim3(cdiv(W, IG_T), cdiv(H, IG_T), nF), dim3(256), args, 0, c->stream);
    LAUNCHCHK(c, ip.launchName);
    frames = ip.convert ? nullptr : c->d_stage; // (converted: the pyramid starts from d_color)
    return ACF_HIP_OK;
}

// ---- colour conversion, once at full resolution (chnsPyramid.cpp:230-263)
int PyramidRun::colour(bool ingestConverted)
{
    cur = frames;
    cur_fs = int64_t(d_in) * np0;
    curH = H;
    curW = W;
    if (ingestConverted)
    {
        cur = c->d_color;
        cur_fs = int64_t(d) * np0;
    }
    else if (c->d_color)
    {
        prof(c, c->stream, "k_colour");
        const int64_t out_fs = int64_t(d) * np0;
        launchColour(c, frames, c->d_color, np0, nF, cur_fs, out_fs, p.colorSpace, d_in); // (hsv: d_in == 3, the plan checked)
        LAUNCHCHK(c, "colour conversion");
        cur = c->d_color;
        cur_fs = out_fs;
    }
    return ACF_HIP_OK;
}

// ---- real scales, in order (chnsPyramid.cpp:297-338 + chnsCompute.cpp:146-338)
int PyramidRun::prepareScales()
{
    pColor = p.colorSmooth > 0 ? float(12.0 / p.colorSmooth / (p.colorSmooth + 2.0) - 2.0) : 0.f;
    // which real scale's smoothed image each real scale is resampled from (-1: the input frame), following the
    // reference's I = I1 adoption (chnsPyramid.cpp:313-316)
    srcIdx.assign(c->real.size(), -1);
    halfDone.assign(c->real.size(), 0);
    pairDone.assign(c->real.size() + 1, 0);
    {
        int curIdx = -1;
        for (size_t k = 0; k < c->real.size(); k++)
        {
            srcIdx[k] = curIdx;
            if (c->real[k].adoptAsI)
            {
                curIdx = int(k);
            }
        }
    }
    // Real scale k + 1 needs scale k's SMOOTHED image only (its exact half, or the adopted image it is resampled from); what
    // follows the smoothing of scale k — gradMag, convTri, the cells: column-sequential chains that leave most of the machine
    // idle — runs beside the smaller scales' own chains: every scale gets a stream, ordered by "scale k has been smoothed"
    // events (option scale_streams).
    if (c->opt.scaleStreams && c->real.size() > 1 && !c->opt.taps)
    {
        ensureSide(c);
    }
    const size_t nSideS = c->side.size();
    scalePar = c->opt.scaleStreams && c->real.size() > 1 && nSideS >= c->real.size() - 1 && c->evJoin.size() >= nSideS && !c->opt.taps;
    while (scalePar && c->evScale.size() < c->real.size())
    {
        hipEvent_t e;
        HIPCHK(c, hipEventCreateWithFlags(&e, hipEventDisableTiming));
        c->evScale.push_back(e);
    }
    return ACF_HIP_OK;
}

int PyramidRun::realScale(size_t k)
{
    int rc;
    RealScale& rs = c->real[k];
    const int64_t np = int64_t(rs.h) * rs.w;
    if (scalePar)
    {
        if (k > 0)
        {
            prof(c, st, "(end)"); // closes the previous scale's last kernel on its stream
        }
        st = k == 0 ? c->stream : c->side[k - 1];
        if (k > 0)
        {
            HIPCHK(c, hipStreamWaitEvent(st, c->evScale[k - 1], 0));
        }
    }
    const float* img = cur;
    int64_t img_fs = cur_fs;
    rs.scaleForm = ACF_HIP_SF_ROUTE_NONE;
    if (rs.resampled && (rc = imageResample(k, img, img_fs)))
    {
        return rc;
    }
    ScalePlan sp = planScale(k, img, img_fs);
    if (sp.needU && !rs.U)
    {
        // the first call that takes a form which reads U where the plan expected checkpoints (a form switch set after the plan)
        if ((rc = allocU(c, rs, c->maxBatch)))
        {
            return rc;
        }
        sp = planScale(k, img, img_fs);
    }
    rs.triForm = (sp.ck ? 1 : 0) | (rs.U ? 2 : 0);
    if ((rc = smoothImage(k, img, img_fs, sp)))
    {
        return rc;
    }
    if (scalePar)
    {
        HIPCHK(c, hipEventRecord(c->evScale[k], st));
    }
    if (rs.adoptAsI)
    {
        cur = rs.sm;
        cur_fs = int64_t(d) * np;
        curH = rs.h;
        curW = rs.w;
    }
    return gradientChannels(k, sp);
}

// the real scale's image from the adopted image (chnsPyramid.cpp:305-311)
int PyramidRun::imageResample(size_t k, const float*& img, int64_t& img_fs)
{
    RealScale& rs = c->real[k];
    const int64_t np = int64_t(rs.h) * rs.w;
    if (rs.src_h != curH || rs.src_w != curW)
    {
        return fail(c, ACF_HIP_E_INVALID, "pyramid: internal plan mismatch");
    }
    if (c->h_descs[rs.descIndex].src_frame_stride != cur_fs)
    {
        return fail(c, ACF_HIP_E_INVALID, "pyramid: internal frame-stride mismatch");
    }
    prof(c, st, "k_resample(image)");
    const ResampleDesc& hd = c->h_descs[rs.descIndex];
    const bool exactHalf = hd.xmode == RS_EXACT && hd.ymode == RS_EXACT && hd.xk == 2 && hd.yk == 2 && hd.ha % 4 == 0 && hd.hb % 2 == 0 &&
        hd.src_frame_stride % 4 == 0 && hd.dst_frame_stride % 2 == 0 && hd.src_off % 4 == 0 && hd.dst_off % 2 == 0 &&
        (uintptr_t(cur) & 15) == 0 && (uintptr_t(rs.img) & 7) == 0; // (k_resample_half's case: one thread per output pair)
    // (rs.scaleForm: every branch writes down the route it is, for acf_hip_get_scale_forms)
    if (halfDone[k] || pairDone[k])
    {
        // already produced by the previous scale's k_smooth_vec, or together with the previous scale's image (k_resample_strip)
        rs.scaleForm = halfDone[k] ? ACF_HIP_SF_ROUTE_HALF_FUSED : ACF_HIP_SF_ROUTE_PAIR_B;
    }
    else if (rs.strip.ok && !exactHalf && !resampleGenericOnly() && (uintptr_t(cur) & 15) == 0)
    {
        // (with the scales on their own streams the next scale's chain would need one more event: the pair is for the one-stream order)
        const bool pair = rs.stripPair.ok && k + 1 < c->real.size() && srcIdx[k + 1] == srcIdx[k] && !c->opt.taps && !scalePar;
        if (pair)
        {
            pairDone[k + 1] = 1;
        }
        const StripPlan& sp = pair ? rs.stripPair : rs.strip;
        const int nSplit = launchStrip(c, st, sp, c->d_descs, rs.descIndex, pair ? c->real[k + 1].descIndex : -1, hd.nplanes, cur, rs.img,
            pair ? c->real[k + 1].img : nullptr, c->d_it, c->d_ft, nF);
        rs.scaleForm = (pair ? ACF_HIP_SF_ROUTE_STRIP_PAIR_A : ACF_HIP_SF_ROUTE_STRIP) | (sp.slowRows > 0 ? ACF_HIP_SF_SLOW : 0) | std::min(sp.nty, 255) << 8 |
            std::min(nSplit, 255) << 16;
    }
    else if (exactHalf)
    {
        const int64_t items = int64_t(hd.hb / 2) * hd.wb * hd.nplanes;
        hipLaunchKernelGGL(k_resample_half, dim3(cdiv(items, 256), 1, nF), dim3(256), 0, st, cur, rs.img,
            (const ResampleDesc*)(c->d_descs + rs.descIndex));
        rs.scaleForm = ACF_HIP_SF_ROUTE_HALF;
    }
    else if (resampleUpOk(hd) && !resampleGenericOnly() && (uintptr_t(rs.img) & 15) == 0)
    {
        // nOctUp > 0: the frame up-sampled (cfg 4)
        const int nw = hd.nplanes * cdiv(hd.hb, 256) * cdiv(hd.wb, RSU_XC);
        hipLaunchKernelGGL(k_resample_up, dim3(cdiv(nw, 4), 1, nF), dim3(256), 0, st, cur, rs.img,
            (const ResampleDesc*)(c->d_descs + rs.descIndex), (const int32_t*)c->d_it, (const float*)c->d_ft);
        rs.scaleForm = ACF_HIP_SF_ROUTE_UP;
    }
    else
    {
        // small planes: fewer columns per wave, more waves
        const int xt = int64_t(resampleBlocks(hd)) * nF < 4096 ? 2 : RS_XT;
        hipLaunchKernelGGL(k_resample, dim3(resampleBlocks(hd, xt), 1, nF), dim3(64, 4), 0, st, cur, rs.img,
            (const ResampleDesc*)(c->d_descs + rs.descIndex), (const int32_t*)c->d_it, (const float*)c->d_ft, xt);
        rs.scaleForm = ACF_HIP_SF_ROUTE_GENERIC | (xt == 2 ? ACF_HIP_SF_XT2 : 0);
    }
    LAUNCHCHK(c, "k_resample(image)");
    img = rs.img;
    img_fs = int64_t(d) * np;
    return ACF_HIP_OK;
}

// the scale's plan: which forms smoothImage and gradientChannels take (the one triPlan of the scale gives the M / O / U layout)
ScalePlan PyramidRun::planScale(size_t k, const float* img, int64_t img_fs)
{
    const RealScale& rs = c->real[k];
    const int64_t np = int64_t(rs.h) * rs.w;
    const bool grad = p.gradMagEnabled || p.gradHistEnabled;
    const bool moWithImage = d_in == 5 && k == 0; // (five planes: M, O came with the image)
    ScalePlan sp;
    sp.fuseSm = p.colorSmooth > 0 && p.colorEnabled && !c->opt.taps && c->opt.fusedSmooth && shrink == 4 && rs.h % 4 == 0 && rs.w % 4 == 0 && rs.w >= 16 &&
        rs.h / 4 <= SV_MAXW * SV_OWN && img_fs % 4 == 0 && np % 4 == 0 && (uintptr_t(img) & 15) == 0;
    ChnsArgs& a = sp.a;
    a.sm = rs.sm;
    a.M = rs.M;
    a.S = rs.S;
    a.O = rs.O;
    a.Mn = c->opt.taps ? rs.Mn : nullptr;
    a.chns = c->d_chns + pl.raw_off[rs.level];
    a.sm_fs = int64_t(d) * np;
    a.m_fs = np;
    a.chns_fs = pl.raw_floats;
    a.h = rs.h;
    a.w = rs.w;
    a.d = d;
    a.colorEnabled = p.colorEnabled;
    a.colorDone = sp.fuseSm ? 1 : 0;
    a.magEnabled = p.gradMagEnabled;
    a.histEnabled = p.gradHistEnabled;
    a.nOrients = p.nOrients;
    a.doNorm = p.normRad != 0;
    a.full = p.full;
    a.hardBin = p.softBin < 0;
    a.normConst = float(p.normConst);
    a.rq_y = shrinkGainY(shrink);
    // M, O and U of this scale in 64 x 16 blocks when every kernel that touches them is the vector form
    const bool gradVec = rs.h % 4 == 0 && np % 4 == 0;
    sp.fuseCells = shrink == 4 && !c->opt.taps;
    if (grad && p.normRad && !moWithImage)
    {
        const TriPlan tp = triPlan(rs.M, rs.U, rs.h, rs.w, p.normRad, np, sp.fuseCells ? &a : nullptr, rs.uFloats, rs.moFloats, gradVec, rs.Ck, rs.ckFloats);
        sp.blocked = tp.blocked;
        sp.ck = tp.ck;
        sp.needU = !tp.ck;
    }
    if (!sp.fuseSm)
    {
        return sp;
    }
    // k_smooth_vec: smoothing + the level's colour channels (+ the next real scale's image when it is an exact half of this one) from
    // registers; full-resolution smoothed planes are written only where something still reads them
    sp.halfNext = k + 1 < c->real.size() && srcIdx[k + 1] == int(k) && c->real[k + 1].resampled && [&] {
        const ResampleDesc& nd = c->h_descs[c->real[k + 1].descIndex];
        return nd.xmode == RS_EXACT && nd.ymode == RS_EXACT && nd.xk == 2 && nd.yk == 2 && nd.ha == rs.h && nd.wa == rs.w;
    }();
    bool needFullAll = false;
    for (size_t m = k + 1; m < c->real.size(); m++)
    {
        if (srcIdx[m] == int(k) && !(m == k + 1 && sp.halfNext))
        {
            needFullAll = true;
        }
    }
    sp.nt = cdiv(rs.h / 4, SV_OWN) * 64; // a wave owns SV_OWN row quads and shadows SV_K of each neighbour
    // the gradient plane's chain also emits gradMag (k_smooth_grad): its smoothed plane is then written only where a later scale is
    // resampled from it, and k_grad_mag_vec does not run for this scale.  Where it pays (measured at 1080p, 3 x 96 frames: +4 % frames/s
    // with scale 0 fused, +2 % with every scale; one frame alone 1.21 -> 1.61 / 2.40 ms): the gradient work rides on a chain of column
    // steps, so it needs many chains (frames x segments) and a plane big enough for the saved round trip to matter.  A/B: the variables.
    const int64_t gradMinPx = int64_t(1) << 20;
    const int gradMinF = 16;
    sp.wantGrad = grad && gradVec && !moWithImage && (c->opt.fusedGrad >= 2 || (c->opt.fusedGrad == 1 && np >= gradMinPx && nF >= gradMinF));
    // convTri's x pass on the same chain: running sums have no warm-up, so the gradient plane is then one segment
    // (96 workgroups for 96 frames: slower alone, faster beside other contexts' kernels — DESIGN.md 3.0)
    const int triMinF = 64;
    sp.triXFused = sp.wantGrad && sp.blocked && p.normRad == 5 && rs.w >= 48 && sp.nt <= 512 &&
        (c->opt.fusedTri >= 2 || (c->opt.fusedTri == 1 && c->opt.sharedDevice && nF >= triMinF));
    for (int z = 0; z < d; z++)
    {
        if (needFullAll || (grad && z == p.colorChn && !sp.wantGrad))
        {
            sp.fullMask |= 1u << z;
        }
    }
    // column segments: as many as give a launch ~6 waves per SIMD (a plane is a chain of column steps with nt / 64 waves), each at least
    // 4 warm-ups long; one segment = the plain recursion.  `planesOf`: planes in the launch
    sp.warm = std::max(16, c->opt.smoothWarm);
    auto segmentsFor = [&](int planesOf, int& segW_) {
        int n = c->opt.smoothSegments;
        if (n == 0 && c->opt.sharedDevice && nF >= 64)
        {
            n = 1; // (beside other contexts: the plain chain — no warm-up columns, nothing to verify or repair)
        }
        if (n == 0)
        {
            const int64_t waves = int64_t(std::max(planesOf, 1)) * nF * (sp.nt / 64);
            n = int(std::min<int64_t>((6 * 1024 + waves - 1) / waves, rs.w / (4 * sp.warm)));
        }
        n = std::max(1, std::min(n, std::min(c->segCap, rs.w / 16)));
        segW_ = cdiv(cdiv(rs.w, n), 16) * 16;
        return cdiv(rs.w, segW_);
    };
    // the two launches cut their planes on their own: the gradient plane's launch has a third of the chains (more segments), the
    // other planes' launch two thirds
    if (!sp.wantGrad)
    {
        sp.nSeg = sp.nSegG = segmentsFor(d, sp.segW);
        sp.segWG = sp.segW;
    }
    else
    {
        if (sp.triXFused)
        {
            sp.nSegG = 1;
            sp.segWG = cdiv(rs.w, 16) * 16;
        }
        else
        {
            sp.nSegG = segmentsFor(1, sp.segWG);
        }
        sp.nSeg = sp.nSegG;
        sp.segW = sp.segWG;
        if (d > 1)
        {
            sp.nSeg = segmentsFor(d - 1, sp.segW);
        }
    }
    sp.segStride = std::max(sp.nSeg, sp.nSegG);
    sp.ldsB = size_t(2) * SV_MAXW * 2 * SV_K * 4 * sizeof(float);
    sp.ldsG = sp.ldsB + size_t(GM_ACOS_N) * sizeof(float) + (c->opt.arith ? size_t(X86_GM_N) * sizeof(uint2) : 0); // (+ gradMag's table pairs, option "arith")
    return sp;
}

int PyramidRun::smoothImage(size_t k, const float* img, int64_t img_fs, const ScalePlan& sp)
{
    int rc;
    RealScale& rs = c->real[k];
    const int64_t np = int64_t(rs.h) * rs.w;
    // convTri(I, I, pColor.smooth, 1) in place (chnsCompute.cpp:239)
    if (!sp.fuseSm)
    {
        if (p.colorSmooth > 0)
        {
            return launchSmooth(c, st, img, rs.sm, c->d_realJobs + k, 1, d, rs.h, img_fs, int64_t(d) * np, nF, pColor, true);
        }
        hipLaunchKernelGGL(k_copy_planes, dim3(cdiv(np * d, 256), 1, nF), dim3(256), 0, st, img, rs.sm, (const SmoothJob*)(c->d_realJobs + k), img_fs,
            int64_t(d) * np);
        LAUNCHCHK(c, "k_copy_planes");
        return ACF_HIP_OK;
    }
    SmoothVecArgs sa{};
    sa.in = img;
    sa.in_fs = img_fs;
    sa.in_ps = np;
    sa.sm = rs.sm;
    sa.sm_fs = int64_t(d) * np;
    sa.sm_ps = np;
    sa.chns = c->d_chns + pl.raw_off[rs.level];
    sa.chns_fs = pl.raw_floats;
    sa.cells = int64_t(rs.h / 4) * (rs.w / 4);
    sa.h = rs.h;
    sa.w = rs.w;
    sa.p = pColor;
    sa.rq_y = shrinkGainY(shrink);
    sa.dump = c->d_dump;
    if (sp.halfNext)
    {
        const RealScale& nx = c->real[k + 1];
        sa.half = nx.img;
        sa.half_ps = int64_t(nx.h) * nx.w;
        sa.half_fs = int64_t(d) * sa.half_ps;
        sa.rkHalf = c->h_descs[nx.descIndex].rk[0];
        halfDone[k + 1] = true;
    }
    sa.plane0 = 0;
    sa.nPlanes = d;
    sa.segW = sp.segW;
    sa.warm = sp.warm;
    sa.nSeg = sp.nSeg;
    sa.segStride = sp.segStride;
    sa.specState = c->d_specState;
    sa.trueState = c->d_trueState;
    sa.redo = nullptr;
    sa.skipZ = -1;
    if (sp.wantGrad)
    {
        sa.skipZ = p.colorChn;
        sa.gM = rs.M;
        sa.gO = rs.O;
        sa.acos = c->d_acos;
        sa.mo_fs = sp.blocked ? moBlockedFloats(rs.h, rs.w) : np;
        sa.nybM = sp.blocked ? (rs.h + 15) / 16 : 0;
        sa.full = p.full;
        if (sp.triXFused)
        {
            sa.tU = sp.ck ? rs.Ck : rs.U;
            sa.u_fs = sp.ck ? triCkFloats(rs.h, rs.w) : uBlockedFloats(rs.h, rs.w);
            sa.nybU = triCkBlockRows(rs.h);
        }
    }
    // the gradient plane's launch (with convTri's x pass on the chain or without, the next scale's half image or not, exact reciprocals
    // or — option "arith" — one x86 CPU's): first, its chains are the long ones; then the other planes' launch "k_smooth_vec"
    auto gradArgs = [&](int segW, int nSeg) {
        SmoothVecArgs g = sa;
        g.plane0 = p.colorChn;
        g.skipZ = -1;
        g.segW = segW;
        g.nSeg = nSeg;
        g.x86 = x86T(c);
        return g;
    };
    const SmoothVecKernel gradKernel = smoothGradKernel(sp.triXFused, sp.halfNext, x86T(c) != nullptr, sp.ck), vecKernel = smoothVecKernel(sp.halfNext);
    const char* gradName = sp.triXFused ? "k_smooth_grad_tri" : "k_smooth_grad";
    const int nVec = sp.wantGrad ? d - 1 : d;
    // (the repair flags are zero here: set by k_smooth_verify, taken down by the repair launch that reads them)
    if (sp.wantGrad)
    {
        if ((rc = allowLds(c, reinterpret_cast<const void*>(gradKernel), sp.ldsG)))
        {
            return rc;
        }
        prof(c, st, gradName);
        hipLaunchKernelGGL(gradKernel, dim3(1, sp.nSegG, nF), dim3(sp.nt), sp.ldsG, st, gradArgs(sp.segWG, sp.nSegG), sp.fullMask);
    }
    if (nVec > 0)
    {
        prof(c, st, "k_smooth_vec");
        hipLaunchKernelGGL(vecKernel, dim3(nVec, sp.nSeg, nF), dim3(sp.nt), sp.ldsB, st, sa, sp.fullMask);
    }
    LAUNCHCHK(c, "k_smooth_vec");
    if (sp.segStride == 1)
    {
        return ACF_HIP_OK;
    }
    // the segments' hand-overs, bit for bit; planes with a difference are recomputed as one chain
    hipLaunchKernelGGL(k_smooth_verify, dim3(sp.segStride - 1, d, nF), dim3(256), 0, st, (const float*)c->d_specState, (const float*)c->d_trueState,
        rs.h, sp.segStride, d, c->d_redo, c->opt.smoothForceRedo, sp.nSeg, sp.wantGrad ? p.colorChn : -1, sp.nSegG);
    LAUNCHCHK(c, "k_smooth_verify");
    if ((rc = countRepairs(c, st, c->d_redo, size_t(nF) * d, 0)))
    {
        return rc;
    }
    sa.segW = rs.w;
    sa.warm = 0;
    sa.nSeg = 1;
    sa.redo = c->d_redo;
    if (sp.wantGrad)
    {
        prof(c, st, gradName);
        if (sp.nSegG > 1) // (else nothing to repair: the plane was one chain)
        {
            hipLaunchKernelGGL(gradKernel, dim3(1, 1, nF), dim3(sp.nt), sp.ldsG, st, gradArgs(rs.w, 1), sp.fullMask);
        }
    }
    if (nVec > 0)
    {
        prof(c, st, "k_smooth_vec");
        hipLaunchKernelGGL(vecKernel, dim3(nVec, 1, nF), dim3(sp.nt), sp.ldsB, st, sa, sp.fullMask);
    }
    LAUNCHCHK(c, "k_smooth_vec(repair)");
    return ACF_HIP_OK;
}

// gradMag, convTri(M), gradMagNorm, gradHist and the shrunk channels of a real scale (chnsCompute.cpp:263-331, addChn :340-370)
int PyramidRun::gradientChannels(size_t k, const ScalePlan& sp)
{
    int rc;
    RealScale& rs = c->real[k];
    const int64_t np = int64_t(rs.h) * rs.w;
    ChnsArgs a = sp.a;
    if (d_in == 5 && k == 0)
    {
        // chnsCompute.cpp:219-226,265-269 (chnsPyramid.cpp:318-322): the first real scale takes the M, O planes that came with the image —
        // no gradientMag, no normalisation; magnitude channel and histogram from them (k_chns)
        a.M = frames + 3 * np0;
        a.O = frames + 4 * np0;
        a.S = nullptr;
        a.Mn = nullptr;
        a.m_fs = int64_t(d_in) * np0;
        a.doNorm = 0;
        return launchChns(c, st, a, shrink, nF);
    }
    a.x86 = x86T(c);
    if ((p.gradMagEnabled || p.gradHistEnabled) && !sp.wantGrad) // (with it, M and O are there already)
    {
        prof(c, st, "k_grad_mag");
        if (rs.h % 4 == 0 && np % 4 == 0)
        {
            // 16 bytes per lane, persistent grid (one 16-wave workgroup per CU around the 80 KB LDS table), grid-stride over (frame, strip, row quad)
            const int64_t items = int64_t(cdiv(rs.w, GMV_XT)) * (rs.h / 4) * nF;
            const int gmvMax = 256;
            const int blocks = int(std::min<int64_t>(gmvMax, (items + GMV_BLOCK - 1) / GMV_BLOCK));
            hipLaunchKernelGGL(gradMagVecKernel(sp.blocked, a.x86 != nullptr), dim3(blocks), dim3(GMV_BLOCK), 0, st,
                (const float*)(rs.sm + int64_t(p.colorChn) * np), rs.M, rs.O, (const float*)c->d_acos, rs.h, rs.w, p.full, int64_t(d) * np,
                sp.blocked ? moBlockedFloats(rs.h, rs.w) : np, nF, sp.blocked ? (rs.h + 15) / 16 : 0, a.x86);
        }
        else
        {
            // enough workgroups to fill the chip twice over, each long enough to amortise its 80 KB table copy
            const int rowBlocks = cdiv(rs.h, GM_ROWS), nStrips = cdiv(rs.w, GM_XT);
            const int want = std::max(1, cdiv(1024, rowBlocks * nF));
            const int spb = std::max(8, cdiv(nStrips, want));
            hipLaunchKernelGGL(k_grad_mag_strip, dim3(rowBlocks, cdiv(nStrips, spb), nF), dim3(GM_ROWS), 0, st,
                (const float*)(rs.sm + int64_t(p.colorChn) * np), rs.M, rs.O, (const float*)c->d_acos, rs.h, rs.w, p.full, int64_t(d) * np, np, spb, x86T(c));
        }
        LAUNCHCHK(c, "k_grad_mag");
    }
    bool cellsDone = false;
    if ((p.gradMagEnabled || p.gradHistEnabled) && p.normRad)
    {
        // convTri(M, normRad): x running sums, then the y pass — fused with the channel cells when the level allows it
        // (S then never reaches HBM), else S is written for k_chns
        if ((rc = launchTri(c, st, rs.M, rs.U, rs.S, rs.h, rs.w, p.normRad, np, nF, sp.fuseCells ? &a : nullptr, &cellsDone, rs.uFloats, rs.moFloats,
                 sp.blocked, sp.triXFused, rs.Ck, rs.ckFloats, sp.ck)))
        {
            return rc;
        }
    }
    return cellsDone ? ACF_HIP_OK : launchChns(c, st, a, shrink, nF);
}

int PyramidRun::joinScales()
{
    if (scalePar)
    {
        prof(c, st, "(end)");
        st = c->stream;
        return joinStreams(c, c->real.size() - 1, [this](size_t i) { return c->side[i]; }, st);
    }
    return ACF_HIP_OK;
}

// ---- approximated levels, smoothing and padding of frames [f0, f0 + nLF) of the batch (chnsPyramid.cpp:385-435)
// The stage's forms, decided once per call; what depends on the frame offset (the channels, the pyramid, the rank cells' frame) is the launchers'
int PyramidRun::planLevels(int nLF)
{
    LevelsCall& lc = lv;
    lc = LevelsCall{};
    lc.nLF = nLF;
    const bool waveSmooth = p.smooth > 0 && c->finalMaxH <= 64 * LEVEL_MAX_R_REAL && c->opt.fusedLevels != 0;
    const bool fused = waveSmooth && c->fusedOk && c->opt.fusedLevels == 1;
    lc.path = fused ? LV_FUSED : waveSmooth ? LV_WAVE_SMOOTH : p.smooth > 0 ? LV_SMOOTH_JOBS : LV_COPY;
    lc.approxFirst = !fused && c->nApproxDescs > 0;
    lc.pad = p.pad_h / shrink > 0 || p.pad_w / shrink > 0;
    lc.pS = p.smooth > 0 ? float(12.0 / p.smooth / (p.smooth + 2.0) - 2.0) : 0.f;
    if (!waveSmooth)
    {
        for (const auto& l : pl.levels)
        {
            lc.copyElems = std::max<int64_t>(lc.copyElems, int64_t(pl.nChns) * l.hC * l.wC); // (LV_COPY's grid)
        }
        return ACF_HIP_OK;
    }
    lc.rawOut = fused && c->opt.taps;
    lc.jobs = fused ? c->d_levelJobs : c->d_levelJobsRaw;
    lc.groups = fused ? &c->levelGroups : &c->levelGroupsRaw;
    lc.nAll = fused ? c->nAllJobs : c->nAllJobsRaw;
    lc.lvChain = (c->opt.cascadeTurns & 4) ? 0 : 1;
    lc.lvTurns = (c->opt.cascadeTurns & 6) && fused && c->nAllJobs > 0;
    // every group is an independent launch (disjoint outputs): on the side streams, forked from st
    if (!lc.groups->empty())
    {
        ensureSide(c);
        lc.nSide = c->evFork ? c->side.size() : 0;
    }
    for (const auto& g : *lc.groups)
    {
        if (!levelKernel(g.R, g.mode))
        {
            return fail(c, ACF_HIP_E_UNSUPPORTED, "pyramid: level taller than the level kernels' rows per lane");
        }
    }
    // what the levels leave as: floats (always, unless the caller has declared the float pyramid unneeded), and the
    // cascade's 16-bit rank cells when every level goes through this one launch
    // (the rank cells have one reader, the tile kernel: a plan or option that routes the cascade elsewhere keeps floats)
    lc.emitRank = fused && c->levelsEmitRank && rankCellsOn(c, c->cs) && !c->opt.taps && c->opt.cascadeTiles;
    // (depths other than 2 keep the floats: their queue's overflow path reads them)
    lc.emitF32 = !(lc.emitRank && !c->opt.keepPyramid && !c->autoLambdas) || (c->cs.tilesR.ok && c->p.treeDepth != 2);
    if (lc.nAll == 0)
    {
        return ACF_HIP_OK;
    }
    lc.ldsL = size_t(LEVEL_WAVES) * (lc.emitRank ? LEVEL_ALL_WF_RANK : LEVEL_ALL_WF) * sizeof(float);
    if (lc.emitRank)
    {
        lc.ra.fs = c->cs.pyrRCells;
        lc.ra.chan = c->cs.d_rankChan;
        lc.ra.rec = c->cs.d_rankRec;
        lc.ldsL += size_t(c->cs.rankMaxRec) * sizeof(RankRec);
    }
    // column segments for small batches (a level's chain of up to wC column steps is then the launch's duration):
    // as many as give the launch ~4 waves per SIMD, at most levelSegCap; every hand-over verified on the device
    int nSegL = 1;
    if (fused && !c->opt.taps && nLF <= c->levelSegFrames && c->opt.levelSegments != 1 && !c->autoLambdas)
    {
        const int64_t wavesL = int64_t(lc.nAll) * pl.nChns * nLF;
        nSegL = c->opt.levelSegments > 1 ? c->opt.levelSegments : int((4 * 1024 + wavesL - 1) / wavesL); // 0: ~4 waves per SIMD
        nSegL = std::max(1, std::min(nSegL, c->levelSegCap));
    }
    lc.lsa.nSeg = nSegL;
    lc.lsa.warm = std::max(4, c->opt.levelWarm / 4 * 4);
    lc.lsa.hMax = c->levelHMax;
    lc.lsa.nJobs = lc.nAll;
    lc.lsa.spec = c->d_lvSpec;
    lc.lsa.tru = c->d_lvTrue;
    lc.lsa.redo = nullptr;
    lc.allKernel = levelAllKernel(lc.emitF32, lc.emitRank, c->cs.rankHasZero, nSegL > 1);
    return allowLds(c, reinterpret_cast<const void*>(lc.allKernel), lc.ldsL);
}

int PyramidRun::levels(int f0, int nLF)
{
    if (int rc = planLevels(nLF))
    {
        return rc;
    }
    noteLevelForms();
    return launchLevels(lv, f0);
}

// acf_hip_get_level_forms' call-wide words: what planLevels decided, as launchLevels reads it
void PyramidRun::noteLevelForms()
{
    static_assert(LV_FUSED == ACF_HIP_LV_FUSED && LV_WAVE_SMOOTH == ACF_HIP_LV_WAVE_SMOOTH && LV_SMOOTH_JOBS == ACF_HIP_LV_SMOOTH_JOBS && LV_COPY == ACF_HIP_LV_COPY, "");
    const bool wave = lv.path == LV_FUSED || lv.path == LV_WAVE_SMOOTH;
    const int32_t w[ACF_HIP_LF_HEAD] = { int32_t(lv.path), wave && lv.emitRank, !wave || lv.emitF32, wave && lv.nAll > 0 ? lv.lsa.nSeg : 0, lv.approxFirst,
        int32_t(pl.levels.size()) };
    std::copy(w, w + ACF_HIP_LF_HEAD, c->levelCallForm);
}

int PyramidRun::launchLevels(const LevelsCall& lc, int f0)
{
    int rc;
    float* const chnsF = c->d_chns + int64_t(f0) * pl.raw_floats;
    float* const pyrF = c->d_pyr + int64_t(f0) * pl.pyr_floats;
    const int nL = int(pl.levels.size());
    if (lc.approxFirst)
    {
        // ---- approximated levels: one launch, blockIdx.y = level (chnsPyramid.cpp:385-397)
        prof(c, st, "k_resample(approx)");
        hipLaunchKernelGGL(k_resample, dim3(c->approxMaxBlocks, c->nApproxDescs, lc.nLF), dim3(64, 4), 0, st,
            (const float*)chnsF, chnsF, (const ResampleDesc*)(c->d_descs + c->nImgDescs), (const int32_t*)c->d_it, (const float*)c->d_ft, RS_XT);
        LAUNCHCHK(c, "k_resample(approx)");
    }
    if (lc.path == LV_FUSED || lc.path == LV_WAVE_SMOOTH)
    {
        // ---- (approximated-scale resample +) smoothing + placement in the padded pyramid: one wave per plane (k_level)
        if (lc.lvTurns && (rc = turnBegin(c, 1, lc.lvChain)))
        {
            return rc;
        }
        prof(c, st, lc.path == LV_FUSED ? "k_level(fused)" : "k_level(smooth)");
        // the groups' streams fork here: their launches run beside k_level_all; biggest planes first
        if (lc.nSide && (rc = forkStreams(c, st, c->evFork, lc.nSide, [this](size_t i) { return c->side[i]; })))
        {
            return rc;
        }
        if ((rc = launchLevelAll(lc, f0)) || (rc = launchLevelGroups(lc, f0)))
        {
            return rc;
        }
    }
    else if (lc.path == LV_SMOOTH_JOBS)
    {
        // ---- smooth every plane of every level into the fused, padded pyramid (chnsPyramid.cpp:399-435)
        if ((rc = launchSmooth(c, st, chnsF, pyrF, c->d_finalJobs, nL, pl.nChns, c->finalMaxH, pl.raw_floats, pl.pyr_floats, lc.nLF, lc.pS, true)))
        {
            return rc;
        }
    }
    else
    {
        hipLaunchKernelGGL(k_copy_planes, dim3(cdiv(lc.copyElems, 256), nL, lc.nLF), dim3(256), 0, st, (const float*)chnsF, pyrF,
            (const SmoothJob*)c->d_finalJobs, pl.raw_floats, pl.pyr_floats);
        LAUNCHCHK(c, "k_copy_planes(final)");
    }
    return lc.pad ? padLevels(lc, f0) : ACF_HIP_OK;
}

// the leading nAll jobs in one launch (k_level_all); in column segments: launch, verify, repair
int PyramidRun::launchLevelAll(const LevelsCall& lc, int f0)
{
    int rc;
    if (lc.nAll == 0)
    {
        return ACF_HIP_OK;
    }
    float* const chnsF = c->d_chns + int64_t(f0) * pl.raw_floats;
    LevelRankArgs ra = lc.ra;
    if (lc.emitRank)
    {
        ra.out = c->cs.d_pyrR + int64_t(f0) * c->cs.pyrRCells;
    }
    LevelSegArgs lsa = lc.lsa;
    auto launchAll = [&](int nz) {
        hipLaunchKernelGGL(lc.allKernel, dim3(pl.nChns, cdiv(lc.nLF, LEVEL_WAVES), nz), dim3(64 * LEVEL_WAVES), lc.ldsL, st, (const float*)chnsF,
            c->d_pyr + int64_t(f0) * pl.pyr_floats, lc.rawOut ? chnsF : nullptr, lc.jobs, (const ResampleDesc*)(c->d_descs + c->nImgDescs),
            (const int32_t*)c->d_it, (const float*)c->d_ft, pl.nChns, pl.raw_floats, pl.pyr_floats, lc.pS, c->d_dump, lc.nLF, ra, lsa);
    };
    launchAll(lc.nAll * lsa.nSeg);
    if (lsa.nSeg > 1)
    {
        // the segments' hand-overs, bit for bit; level planes with a difference are recomputed as one chain
        hipLaunchKernelGGL(k_level_verify, dim3(lc.nAll * lsa.nSeg, pl.nChns, lc.nLF), dim3(64), 0, st, (const float*)c->d_lvSpec,
            (const float*)c->d_lvTrue, lc.jobs, lsa, pl.nChns, c->d_lvRedo, c->opt.smoothForceRedo);
        if ((rc = countRepairs(c, st, c->d_lvRedo, size_t(lc.nLF) * lc.nAll * pl.nChns, 2)))
        {
            return rc;
        }
        lsa.nSeg = 1;
        lsa.redo = c->d_lvRedo;
        launchAll(lc.nAll);
    }
    LAUNCHCHK(c, "k_level_all");
    return lc.lvTurns ? turnEnd(c, 1, lc.lvChain) : ACF_HIP_OK;
}

// the other jobs in groups of equal (rows per lane, mode), one launch each (k_level): round-robin over the forked streams, then joined
int PyramidRun::launchLevelGroups(const LevelsCall& lc, int f0)
{
    float* const chnsF = c->d_chns + int64_t(f0) * pl.raw_floats;
    size_t gi = 0;
    for (auto git = lc.groups->rbegin(); git != lc.groups->rend(); ++git, ++gi)
    {
        const auto& g = *git;
        hipStream_t lst = lc.nSide ? c->side[gi % lc.nSide] : st;
        dim3 grid(pl.nChns, g.count, cdiv(lc.nLF, LEVEL_WAVES)), block(64 * LEVEL_WAVES);
        hipLaunchKernelGGL(levelKernel(g.R, g.mode), grid, block, 0, lst, (const float*)chnsF, c->d_pyr + int64_t(f0) * pl.pyr_floats,
            lc.rawOut ? chnsF : nullptr, lc.jobs + g.first, (const ResampleDesc*)(c->d_descs + c->nImgDescs), (const int32_t*)c->d_it, (const float*)c->d_ft,
            pl.nChns, pl.raw_floats, pl.pyr_floats, lc.pS, c->d_dump, lc.nLF);
        LAUNCHCHK(c, "k_level");
    }
    return joinStreams(c, std::min(lc.nSide, lc.groups->size()), [this](size_t i) { return c->side[i]; }, st);
}

int PyramidRun::padLevels(const LevelsCall& lc, int f0)
{
    const dim3 grid(cdiv(c->padMaxElems, 256), int(pl.levels.size()), lc.nLF);
    prof(c, st, "k_pad_reflect");
    if (lc.emitF32)
    {
        hipLaunchKernelGGL(k_pad_reflect<float>, grid, dim3(256), 0, st, c->d_pyr + int64_t(f0) * pl.pyr_floats, (const PadJob*)c->d_padJobs, pl.pyr_floats);
    }
    if (lc.emitRank)
    {
        hipLaunchKernelGGL(k_pad_reflect<uint16_t>, grid, dim3(256), 0, st, c->cs.d_pyrR + int64_t(f0) * c->cs.pyrRCells, (const PadJob*)c->d_padJobsR,
            c->cs.pyrRCells);
    }
    LAUNCHCHK(c, "k_pad_reflect");
    return ACF_HIP_OK;
}

// Image-specific lambdas (chnsPyramid.cpp:341-374), then the levels frame by frame with that frame's gains
int PyramidRun::levelsWithImageLambdas()
{
    int rc;
    // Image-specific lambdas (chnsPyramid.cpp:341-374): per-type means of the raw channels at two real levels (f64 plane
    // sums on the device, k_plane_sums), lambda = -log2(f0/f1) / log2(s0/s1) on the host with the C library the
    // oracle uses, then the approximated levels frame by frame with that frame's gains written into the descriptors
    // (stream-ordered copies).  A fallback path for models that ship without lambdas: correctness first — it
    // synchronises once per batch and launches per frame.
    if ((rc = planLevels(1))) // (one plan serves every frame's launches)
    {
        return rc;
    }
    noteLevelForms();
    prof(c, st, "k_plane_sums");
    const int lv0 = pl.lambdaLevel[0], lv1 = pl.lambdaLevel[1];
    SumJob j0{ pl.raw_off[size_t(lv0)], pl.levels[size_t(lv0)].hC * pl.levels[size_t(lv0)].wC, 0 };
    SumJob j1{ pl.raw_off[size_t(lv1)], pl.levels[size_t(lv1)].hC * pl.levels[size_t(lv1)].wC, 0 };
    hipLaunchKernelGGL(k_plane_sums, dim3(pl.nChns, 2, nF), dim3(256), 0, st, (const float*)c->d_chns, pl.raw_floats, j0, j1, pl.nChns, c->d_planeSums);
    LAUNCHCHK(c, "k_plane_sums");
    std::vector<double> sums(size_t(nF) * 2 * pl.nChns);
    HIPCHK(c, hipMemcpyAsync(sums.data(), c->d_planeSums, sums.size() * sizeof(double), hipMemcpyDeviceToHost, st));
    HIPCHK(c, hipStreamSynchronize(st));
    const int nColorL = p.colorEnabled ? d : 0, nMagL = p.gradMagEnabled ? 1 : 0, nHistL = p.gradHistEnabled ? p.nOrients : 0;
    const int nTypeCh[3] = { nColorL, nMagL, nHistL };
    // one copy of the approximated levels' descriptors per frame: each stays untouched until its stream-ordered upload is done
    std::vector<std::vector<ResampleDesc>> descsAll(size_t(nF),
        std::vector<ResampleDesc>(c->h_descs.begin() + c->nImgDescs, c->h_descs.begin() + c->nImgDescs + c->nApproxDescs));
    for (int f = 0; f < nF; f++)
    {
        std::vector<ResampleDesc>& descs = descsAll[size_t(f)];
        double lam[3] = { 0, 0, 0 };
        int z0 = 0;
        for (int j = 0; j < 3; j++)
        {
            if (!nTypeCh[j])
            {
                continue;
            }
            double s0 = 0, s1 = 0; // sum(MatP): the per-plane sums added in plane order (MatP.cpp:97-106)
            for (int k = 0; k < nTypeCh[j]; k++)
            {
                s0 += sums[(size_t(f) * 2 + 0) * pl.nChns + z0 + k];
                s1 += sums[(size_t(f) * 2 + 1) * pl.nChns + z0 + k];
            }
            const double f0 = s0 / (double(nTypeCh[j]) * j0.cells), f1 = s1 / (double(nTypeCh[j]) * j1.cells);
            lam[j] = -(std::log(f0 / f1) / std::log(2.0)) / (std::log(pl.levels[size_t(lv0)].scale / pl.levels[size_t(lv1)].scale) / std::log(2.0));
            z0 += nTypeCh[j];
        }
        for (int j = 0; j < 3; j++)
        {
            c->h_lambdas[size_t(f) * 3 + j] = lam[j];
        }
        size_t ai = 0;
        for (size_t i = 0; i < pl.levels.size(); i++)
        {
            const acf_hip_level& l = pl.levels[i];
            if (l.isReal)
            {
                continue;
            }
            const acf_hip_level& lr = pl.levels[size_t(l.realIndex)];
            double ratio[3];
            for (int j = 0; j < 3; j++)
            {
                ratio[j] = std::pow(l.scale / lr.scale, -lam[j]); // :393
            }
            setResampleGain(descs[ai], ratio, nColorL, nColorL + nMagL);
            ai++;
        }
        if (!descs.empty())
        {
            HIPCHK(c, hipMemcpyAsync(c->d_descs + c->nImgDescs, descs.data(), descs.size() * sizeof(ResampleDesc), hipMemcpyHostToDevice, st));
        }
        if ((rc = launchLevels(lv, f)))
        {
            return rc;
        }
    }
    HIPCHK(c, hipStreamSynchronize(st)); // descsAll is read by the uploads above
    return ACF_HIP_OK;
}

int pyramidBody(acf_hip_ctx* c, const FrameSource& src, int nF)
{
    const float* const frames = src.kind == SRC_F32 ? static_cast<const float*>(src.base) : nullptr;
    if (c && !c->kids.empty())
    {
        if (src.kind != SRC_F32)
        {
            return fail(c, ACF_HIP_E_UNSUPPORTED, std::string(src.who) + ": not available with option \"streams\" > 1");
        }
        if (!frames || nF <= 0 || nF > c->maxBatch)
        {
            return fail(c, ACF_HIP_E_INVALID, "pyramid: n_frames out of range");
        }
        const size_t per = size_t(c->plan.d_in) * c->plan.H * c->plan.W;
        const int rc = forEachKid(c, nF, [&](acf_hip_ctx* k, int first, int n) { return acf_hip_pyramid(k, frames + first * per, n); });
        if (!rc)
        {
            c->lastBatch = nF;
            c->pyramidValid = true;
            c->detectValid = false;
            c->viewRun = false;
        }
        return rc;
    }
    if (int rc = needPlan(c, "pyramid")) return rc;
    if (!src.base || nF <= 0 || nF > c->maxBatch)
    {
        return fail(c, ACF_HIP_E_INVALID, "pyramid: n_frames out of range");
    }
    HIPCHK(c, hipSetDevice(c->device));
    c->pyramidValid = c->detectValid = c->bankValid = false;
    c->viewRun = src.kind == SRC_VIEW; // (every other run clears it)
    int rc;
    PyramidRun run(c, frames, nF);
    IngestPlan ip; // (planar float frames: none; convert stays false)
    if (src.kind != SRC_F32 && ((rc = planIngest(c, src, ip)) || (rc = run.ingest(ip))))
    {
        return rc;
    }
    c->lastFrames = run.frames;
    if ((rc = run.colour(ip.convert)) || (rc = run.prepareScales()))
    {
        return rc;
    }
    for (size_t k = 0; k < c->real.size(); k++)
    {
        if ((rc = run.realScale(k)))
        {
            return rc;
        }
    }
    if ((rc = run.joinScales()))
    {
        return rc;
    }
    if (!c->autoLambdas)
    {
        for (int f = 0; f < nF; f++)
        {
            c->h_lambdas[size_t(f) * 3 + 0] = c->p.lambdas[0];
            c->h_lambdas[size_t(f) * 3 + 1] = c->p.lambdas[1];
            c->h_lambdas[size_t(f) * 3 + 2] = c->p.lambdas[2];
        }
        if ((rc = run.levels(0, nF)))
        {
            return rc;
        }
    }
    else if ((rc = run.levelsWithImageLambdas()))
    {
        return rc;
    }
    prof(c, c->stream, "(end)");
    c->lastBatch = nF;
    c->pyramidValid = true;
    c->ranksValid = run.lv.emitRank;   // else the cascade converts the float pyramid first (k_rank)
    c->floatPyramid = run.lv.emitF32;
    return ACF_HIP_OK;
}
} // namespace
