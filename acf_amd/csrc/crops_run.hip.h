// crops_run.hip.h — part of acf_hip.hip (included there and nowhere else): Detector::evaluate(const cv::Mat&) for a batch of crops
// (ACF.cpp:123-133), acf_hip_evaluate_crops / acf_hip_evaluate_crops_u8.  Device pointers in, device scores out, a model but no plan.
//   planCropCall     every check of the call and its sizes, once (CropCall)
//   cropFusedFits    THE decision between the two forms: by crop size alone
//   cropFused        k_crop_score: one launch, asynchronous, no allocation after the first call with a model
//   cropStaged       the batch as frames through the kernels acf_hip_chns_compute launches, then k_evaluate_windows
// Both forms return the bits of acf_hip_chns_compute + acf_hip_op_evaluate per crop (kernels_crops.hip.h says how).
#pragma once

namespace
{

// what one call computes, decided before anything is launched
struct CropCall
{
    acf_hip_params p; // the channel options in force (the caller's, or the model's)
    int n, h, w, d;
    int hc, wc, dcol, nC, hs, ws; // cropped planes, colour planes, channels, cell planes
    int mH, mW;                   // the window in cells
    int conv;                     // CR_*
    bool fused;
    int nt;     // k_crop_score's workgroup
    size_t lds; // ... and its dynamic LDS, bytes
};

// Does k_crop_score take crops of h x w x d with channel options p (and the context's window)?  Its whole working set lives in one
// workgroup's LDS (kernels_crops.hip.h: four planes of (hc | 1) * wc floats, the window's cells, two columns of row sums) and its
// smoothing step gives every (colour plane, row) a thread.  Every option acf_hip_chns_compute takes is carried, so size decides alone.
// An 80 x 80 x 3 crop with 10 channels takes 123 KB; 128 x 64 x 3 (INRIA) 157 KB; 160 x 160 does not fit.
bool cropFusedFits(const acf_hip_ctx* c, int h, int w, int d, const acf_hip_params& p, int* ntOut = nullptr, size_t* ldsOut = nullptr)
{
    const int hc = h - h % p.shrink, wc = w - w % p.shrink;
    const int dcol = d == 1 ? 1 : colorPlanes(p), nC = numChannels(p, dcol);
    const int mH = c->p.modelDsPad_h / c->p.shrink, mW = c->p.modelDsPad_w / c->p.shrink;
    const int rows = dcol * hc;
#ifdef ACF_CROPS_FORCE_STAGED // (profiles/crop_scores.py's A/B build of the staged form on crops the fused kernel takes; never the product)
    return false;
#endif
    if (rows > 1024)
    {
        return false;
    }
    const int nt = std::max(256, (rows + 63) / 64 * 64);
    const size_t lds = size_t(cropLdsFloats(hc, wc, dcol, nC, mH, mW, nt)) * sizeof(float);
    if (ntOut) *ntOut = nt;
    if (ldsOut) *ldsOut = lds;
    return lds <= std::min(c->ldsPerCu, size_t(160) * 1024);
}

// The classifier on the device for the calls that have no plan: uploaded at the first call after acf_hip_set_model, kept until the
// next one (dropCropModel).
int ensureCropModel(acf_hip_ctx* c)
{
    auto& m = c->crop;
    if (m.valid)
    {
        return ACF_HIP_OK;
    }
    auto up = [&](auto*& dst, const auto& v) {
        using T = typename std::remove_reference<decltype(v)>::type::value_type;
        void* p = nullptr;
        if (hipMalloc(&p, std::max<size_t>(v.size(), 1) * sizeof(T)) != hipSuccess)
        {
            return false;
        }
        dst = static_cast<T*>(p);
        return v.empty() || hipMemcpy(p, v.data(), v.size() * sizeof(T), hipMemcpyHostToDevice) == hipSuccess;
    };
    if (!up(m.fids, c->fids) || !up(m.thrs, c->thrs) || !up(m.hs, c->hs) || !up(m.child, c->child))
    {
        (void)hipGetLastError();
        dropCropModel(c);
        return fail(c, ACF_HIP_E_HIP, "evaluate_crops: uploading the classifier failed");
    }
    // the largest feature id a walk can read (checkModel's rule, kept as one number so that a call compares once): the first
    // 2^depth - 1 nodes of a fixed-depth tree, the nodes with a child of the child-pointer walk; child[] itself passed at acf_hip_set_model
    m.fidMax = 0;
    const size_t nInternal = c->p.treeDepth > 0 ? (size_t(1) << c->p.treeDepth) - 1 : 0;
    for (size_t i = 0; i < c->fids.size(); i++)
    {
        if (c->p.treeDepth > 0 ? i % size_t(c->p.nTreeNodes) < nInternal : c->child[i] != 0)
        {
            m.fidMax = std::max(m.fidMax, c->fids[i]);
        }
    }
    m.valid = true;
    return ACF_HIP_OK;
}

int planCropCall(acf_hip_ctx* c, const acf_hip_params* pIn, const void* crops, const float* scores, int n, int h, int w, int d, CropCall& k)
{
    if (int rc = opBegin(c)) return rc;
    if (int rc = needModel(c, "evaluate_crops")) return rc;
    if (!crops || !scores || n < 1 || h <= 0 || w <= 0 || (d != 1 && d != 3))
    {
        return fail(c, ACF_HIP_E_INVALID, "evaluate_crops: arguments (device pointers, n >= 1, d = 1 or 3)");
    }
    if (c->p.ldcfK > 0)
    {
        return fail(c, ACF_HIP_E_UNSUPPORTED, "evaluate_crops: LDCF models are not scored on crops");
    }
    k.p = pIn ? *pIn : c->p;
    const acf_hip_params& p = k.p;
    {
        std::string err;
        if (const int rcc = checkChnsParams(p, d, err)) // (acf_hip_chns_compute's checks, its codes)
        {
            return fail(c, rcc, "evaluate_crops: " + err);
        }
    }
    if (p.nOrients < 1 || p.nOrients > 12)
    {
        return fail(c, ACF_HIP_E_UNSUPPORTED, "evaluate_crops: nOrients must be 1..12");
    }
    if (d == 1 && p.colorChn != 0)
    {
        return fail(c, ACF_HIP_E_INVALID, "evaluate_crops: colorChn of a 1-plane image must be 0");
    }
    if (p.colorSmooth > 1)
    {
        return fail(c, ACF_HIP_E_UNSUPPORTED, "evaluate_crops: pColor.smooth > 1 (convTri with a radius) is not built for the colour planes");
    }
    k.n = n, k.h = h, k.w = w, k.d = d;
    k.hc = h - h % p.shrink, k.wc = w - w % p.shrink; // chnsCompute.cpp:203-217
    k.dcol = d == 1 ? 1 : colorPlanes(p);
    k.nC = numChannels(p, k.dcol);
    k.hs = k.hc / p.shrink, k.ws = k.wc / p.shrink;
    k.mH = c->p.modelDsPad_h / c->p.shrink, k.mW = c->p.modelDsPad_w / c->p.shrink;
    if (k.hc < c->p.modelDsPad_h || k.wc < c->p.modelDsPad_w || k.hs < k.mH || k.ws < k.mW || k.hc < 2 || k.wc < 2)
    {
        return fail(c, ACF_HIP_E_INVALID, "evaluate_crops: the cropped image is smaller than the model's window (modelDsPad)");
    }
    const int m = std::min(k.hc, k.wc);
    if ((p.gradMagEnabled || p.gradHistEnabled) && p.normRad && (m < 4 || 2 * p.normRad + 1 >= m || p.normRad < 2 || p.normRad > 15))
    {
        return fail(c, ACF_HIP_E_UNSUPPORTED, "evaluate_crops: normRad against the image size");
    }
    if (int rc = ensureCropModel(c)) return rc;
    if (int64_t(c->crop.fidMax) >= int64_t(k.nC) * k.mH * k.mW)
    {
        return fail(c, ACF_HIP_E_INVALID, "evaluate_crops: the model reads a feature beyond these channels' window cells (its fids against nChns * window)");
    }
    k.conv = CR_PASS;
    if (d == 3 && !colourPassthrough(p, d))
    {
        k.conv = p.colorSpace == ACF_HIP_CS_LUV ? ((int64_t(k.hc) * k.wc) % 4 == 0 ? CR_LUV_VEC : CR_LUV) // rgbConvertMex.cpp:92,343
            : p.colorSpace == ACF_HIP_CS_GRAY ? CR_GRAY : CR_HSV;
    }
    k.fused = cropFusedFits(c, h, w, d, p, &k.nt, &k.lds);
    return ACF_HIP_OK;
}

// where a call's crops lie: exactly one of f32 / u8 is set
struct CropSrc
{
    const float* f32;
    const uint8_t* u8;
    U8Geom g; // (u8)
};

using CropKernel = void (*)(CropArgs);

CropKernel cropKernel(int shrink, bool maxO6)
{
    if (shrink == 4)
    {
        return maxO6 ? k_crop_score<4, 6> : k_crop_score<4, 12>;
    }
    return maxO6 ? k_crop_score<2, 6> : k_crop_score<2, 12>;
}

int cropFused(acf_hip_ctx* c, const CropCall& k, const CropSrc& s, double cascThr, float* scores)
{
    const acf_hip_params& p = k.p;
    CropArgs a{};
    a.inF = s.f32;
    a.inU8 = s.u8;
    a.scores = scores;
    a.n = k.n, a.h = k.h, a.w = k.w, a.d = k.d;
    a.hc = k.hc, a.wc = k.wc, a.dcol = k.dcol;
    a.cpp = s.g.cpp, a.ro = s.g.ro, a.go = s.g.go, a.bo = s.g.bo, a.rowStride = s.g.stride;
    a.in_fs = s.u8 ? s.g.frameStride : int64_t(k.d) * k.h * k.w;
    a.conv = k.conv;
    a.lTable = c->d_lTable;
    a.k = makeLuvConsts();
    a.mr = kGray.r, a.mg = kGray.g, a.mb = kGray.b;
    a.acos = c->d_acos;
    a.x86 = x86T(c);
    a.smooth = p.colorSmooth > 0;
    a.smoothP = a.smooth ? float(12.0 / p.colorSmooth / (p.colorSmooth + 2.0) - 2.0) : 0.f;
    a.colorChn = p.colorChn, a.colorEnabled = p.colorEnabled, a.magEnabled = p.gradMagEnabled, a.histEnabled = p.gradHistEnabled;
    a.nOrients = p.nOrients, a.full = p.full, a.hardBin = p.softBin < 0, a.normRad = p.normRad;
    a.normConst = float(p.normConst);
    a.rq_y = shrinkGainY(p.shrink);
    a.pitch = k.hc | 1;
    a.mH = k.mH, a.mW = k.mW, a.nC = k.nC;
    a.fids = c->crop.fids, a.thrs = c->crop.thrs, a.hs = c->crop.hs, a.child = c->crop.child;
    a.nTrees = c->p.nTrees, a.nTreeNodes = c->p.nTreeNodes, a.depth = c->p.treeDepth;
    a.cascThr = float(cascThr);
    const CropKernel kern = cropKernel(p.shrink, p.nOrients <= 6);
    if (int rc = allowLds(c, reinterpret_cast<const void*>(kern), k.lds)) return rc;
    // one workgroup a CU at most (an 80 x 80 crop's LDS admits no second); it takes crops blockIdx.x, + gridDim.x, ...
    prof(c, c->stream, "k_crop_score");
    hipLaunchKernelGGL(kern, dim3(std::min(k.n, c->numCus)), dim3(k.nt), k.lds, c->stream, a);
    LAUNCHCHK(c, "k_crop_score");
    prof(c, c->stream, "(end)");
    return ACF_HIP_OK;
}

// The staged form.  Its planes are a Scratch of this call, sized for a chunk of the batch (at most ~256 MB) and reused by the chunks in
// stream order; the stream is synchronised before the Scratch is released, so this form is NOT asynchronous.
int cropStaged(acf_hip_ctx* c, const CropCall& k, const CropSrc& s, double cascThr, float* scores)
{
    const acf_hip_params& p = k.p;
    const int64_t np = int64_t(k.hc) * k.wc, cellsPer = int64_t(k.nC) * k.hs * k.ws;
    const bool convert = k.conv != CR_PASS, grad = p.gradMagEnabled || p.gradHistEnabled;
    const int64_t perCrop = (int64_t(k.d) + (convert ? k.dcol : 0) + 4) * np + cellsPer;
    const int chunk = int(std::max<int64_t>(1, std::min<int64_t>(k.n, (int64_t(64) << 20) / perCrop)));
    Scratch sc;
    float* dI = sc.alloc<float>(size_t(chunk) * k.d * np);
    float* dCol = convert ? sc.alloc<float>(size_t(chunk) * k.dcol * np) : dI; // (a pass-through's planes are smoothed where they are)
    float *dM = sc.alloc<float>(size_t(chunk) * np), *dO = sc.alloc<float>(size_t(chunk) * np), *dU = sc.alloc<float>(size_t(chunk) * np),
          *dS = sc.alloc<float>(size_t(chunk) * np);
    float* dOut = sc.alloc<float>(size_t(chunk) * cellsPer);
    SmoothJob j{};
    j.h = k.hc, j.w = k.wc, j.nplanes = k.dcol, j.out_cs = k.hc;
    j.in_ps = j.out_ps = np;
    SmoothJob* dj = sc.upload(&j, 1);
    if (!dI || !dCol || !dM || !dO || !dU || !dS || !dOut || !dj)
    {
        (void)hipGetLastError();
        return fail(c, ACF_HIP_E_HIP, "evaluate_crops: allocation");
    }
    int rc = ACF_HIP_OK;
    for (int f0 = 0; f0 < k.n && !rc; f0 += chunk)
    {
        const int nF = std::min(chunk, k.n - f0);
        prof(c, c->stream, "k_crop_gather");
        if (s.u8)
        {
            hipLaunchKernelGGL(k_crop_gather_u8, dim3(cdiv(np, 256), 1, nF), dim3(256), 0, c->stream, s.u8 + int64_t(f0) * s.g.frameStride, dI, k.d, k.hc, k.wc,
                s.g.cpp, s.g.ro, s.g.go, s.g.bo, s.g.stride, s.g.frameStride, int64_t(k.d) * np);
        }
        else
        {
            hipLaunchKernelGGL(k_crop_gather, dim3(cdiv(int64_t(k.d) * np, 256), 1, nF), dim3(256), 0, c->stream, s.f32 + int64_t(f0) * k.d * k.h * k.w, dI, k.h,
                k.w, k.d, k.hc, k.wc, int64_t(k.d) * np);
        }
        LAUNCHCHK(c, "k_crop_gather");
        if (convert)
        {
            prof(c, c->stream, "k_rgb_convert");
            launchColour(c, dI, dCol, np, nF, int64_t(k.d) * np, int64_t(k.dcol) * np, p.colorSpace, k.d);
            LAUNCHCHK(c, "evaluate_crops: colour conversion");
        }
        if (p.colorSmooth > 0)
        {
            const float pColor = float(12.0 / p.colorSmooth / (p.colorSmooth + 2.0) - 2.0);
            if ((rc = launchSmooth(c, c->stream, dCol, dCol, dj, 1, k.dcol, k.hc, int64_t(k.dcol) * np, int64_t(k.dcol) * np, nF, pColor, true)))
            {
                break;
            }
        }
        ChnsArgs a{};
        a.sm = dCol, a.M = dM, a.S = dS, a.O = dO, a.chns = dOut;
        a.sm_fs = int64_t(k.dcol) * np, a.m_fs = np, a.chns_fs = cellsPer;
        a.h = k.hc, a.w = k.wc, a.d = k.dcol;
        a.colorEnabled = p.colorEnabled, a.magEnabled = p.gradMagEnabled, a.histEnabled = p.gradHistEnabled;
        a.nOrients = p.nOrients, a.doNorm = p.normRad != 0, a.full = p.full, a.hardBin = p.softBin < 0;
        a.normConst = float(p.normConst);
        a.rq_y = shrinkGainY(p.shrink);
        a.x86 = x86T(c);
        if (grad)
        {
            prof(c, c->stream, "k_grad_mag");
            hipLaunchKernelGGL(k_grad_mag_strip, dim3(cdiv(k.hc, GM_ROWS), 1, nF), dim3(GM_ROWS), 0, c->stream, (const float*)(dCol + int64_t(p.colorChn) * np), dM,
                dO, (const float*)c->d_acos, k.hc, k.wc, p.full, int64_t(k.dcol) * np, np, cdiv(k.wc, GM_XT), x86T(c));
            LAUNCHCHK(c, "evaluate_crops: k_grad_mag");
            if (p.normRad && (rc = launchTri(c, c->stream, dM, dU, dS, k.hc, k.wc, p.normRad, np, nF)))
            {
                break;
            }
        }
        if ((rc = launchChns(c, c->stream, a, p.shrink, nF)))
        {
            break;
        }
        prof(c, c->stream, "k_evaluate_windows");
        hipLaunchKernelGGL(k_evaluate_windows, dim3(nF), dim3(64), 0, c->stream, (const float*)dOut, cellsPer, k.hs, k.ws, k.mH, k.mW,
            (const uint32_t*)c->crop.fids, (const float*)c->crop.thrs, (const float*)c->crop.hs, (const uint32_t*)c->crop.child, c->p.nTrees, c->p.nTreeNodes,
            c->p.treeDepth, float(cascThr), scores + f0);
        LAUNCHCHK(c, "k_evaluate_windows");
    }
    prof(c, c->stream, "(end)");
    const hipError_t e = hipStreamSynchronize(c->stream); // (the Scratch goes when this returns)
    if (!rc && e != hipSuccess)
    {
        rc = fail(c, ACF_HIP_E_HIP, std::string("evaluate_crops: ") + hipGetErrorString(e));
    }
    return rc;
}

int evaluateCrops(acf_hip_ctx* c, const acf_hip_params* chns, const CropSrc& s, int n, int h, int w, int d, double cascThr, float* scores)
{
    CropCall k{};
    if (int rc = planCropCall(c, chns, s.u8 ? static_cast<const void*>(s.u8) : s.f32, scores, n, h, w, d, k)) return rc;
    return k.fused ? cropFused(c, k, s, cascThr, scores) : cropStaged(c, k, s, cascThr, scores);
}

} // namespace

int acf_hip_evaluate_crops(acf_hip_ctx* c, const acf_hip_params* chns, const float* crops_dev, int n, int h, int w, int d, double cascThr, float* scores_dev)
{
    if (int rc = needCtx(c)) return rc;
    CropSrc s{};
    s.f32 = crops_dev;
    return evaluateCrops(c, chns, s, n, h, w, d, cascThr, scores_dev);
}

int acf_hip_evaluate_crops_u8(acf_hip_ctx* c, const acf_hip_params* chns, const uint8_t* crops_dev, int n, int h, int w, int pix, int row_stride_bytes,
    double cascThr, float* scores_dev)
{
    if (int rc = needCtx(c)) return rc;
    if (int rc = needModel(c, "evaluate_crops_u8")) return rc;
    CropSrc s{};
    s.u8 = crops_dev;
    if (pixIsYuv(pix))
    {
        return fail(c, ACF_HIP_E_INVALID, "evaluate_crops_u8: NV12 / NV21 crops are not taken (RGB, BGR, RGBA, BGRA or GRAY)");
    }
    if (const char* bad = u8Geom(pix, h, w, row_stride_bytes, 0, 0, s.g))
    {
        return fail(c, ACF_HIP_E_INVALID, std::string("evaluate_crops_u8: ") + bad);
    }
    return evaluateCrops(c, chns, s, n, h, w, s.g.cpp == 1 ? 1 : 3, cascThr, scores_dev);
}
