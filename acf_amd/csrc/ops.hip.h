// ops.hip.h — part of acf_hip.hip (included there and nowhere else): the entries that run ONE operator on a caller's host planes,
// outside any plan.  Each begins with opBegin (or a guard), keeps its one-off device buffers in a Scratch, launches on the context's
// stream and ends with Scratch::download.
//   acf_hip_op_yuv420_to_rgb, _op_resize_u8      the 8-bit front end's kernels on one frame
//   acf_hip_op_nms                               bbNms of one list (k_nms)
//   acf_hip_op_rgb_convert, _op_conv_tri, _op_gradient_mag, _op_gradient_hist, _op_im_resample, _op_im_resample_pair   the channel operators (smoothOne, gradMagOne)
//   acf_hip_chns_compute                         chnsCompute of one image at its own scale
//   acf_hip_set_x86_tables, _selftest_x86, _selftest_gradmag   the reference-arithmetic tables and their checks on the device
//   acf_hip_thrs_u8, opAcfDetect1 (acf_hip_op_acf_detect1, _u8, _rank), acf_hip_op_evaluate   the cascade on a caller's channel buffer
#pragma once

int acf_hip_op_yuv420_to_rgb(acf_hip_ctx* c, const uint8_t* src, int rows, int cols, int pix, int rowStride, int64_t chromaOff, uint8_t* dst)
{
    if (int rc = needCtx(c)) return rc;
    if (!src || !dst || !pixIsYuv(pix) || chromaOff < 0)
    {
        return fail(c, ACF_HIP_E_INVALID, "op_yuv420_to_rgb: arguments (pix: ACF_HIP_PIX_NV12 or _NV21)");
    }
    U8Geom g;
    if (const char* bad = u8Geom(pix, rows, cols, rowStride, chromaOff, 0, g))
    {
        return fail(c, ACF_HIP_E_INVALID, std::string("op_yuv420_to_rgb: ") + bad);
    }
    HIPCHK(c, hipSetDevice(c->device));
    const size_t nD = size_t(rows) * cols * 3;
    Scratch s;
    uint8_t *dS = s.upload(src, size_t(g.frameStride)), *dD = s.alloc<uint8_t>(nD);
    if (!dS || !dD)
    {
        (void)hipGetLastError();
        return fail(c, ACF_HIP_E_HIP, "op_yuv420_to_rgb: device allocation or copy failed");
    }
    if (int rc = launchYuvToRgb(c, yuvSrc(dS, pix, rows, cols, g), 1, dD))
    {
        return rc;
    }
    return Scratch::download(c, "op_yuv420_to_rgb", dst, dD, nD);
}

int acf_hip_op_resize_u8(acf_hip_ctx* c, const uint8_t* src, int rows, int cols, int cpp, int rowStride, double scale, uint8_t* dst, int dstRows, int dstCols)
{
    if (int rc = needCtx(c)) return rc;
    if (!src || !dst || cpp < 1 || cpp > 4)
    {
        return fail(c, ACF_HIP_E_INVALID, "op_resize_u8: arguments");
    }
    if (cpp == 2)
    {
        // OpenCV's 2 x 2 area path rounds two-channel pixels with saturate_cast(sum * 0.25f) (half to even), not (sum + 2) >> 2 as for
        // 1, 3 and 4 channels; no pixel format of the path has two channels (ACF_HIP_PIX_*), so the form is not restated
        return fail(c, ACF_HIP_E_UNSUPPORTED, "op_resize_u8: two-channel images are not supported (1, 3 or 4 bytes per pixel)");
    }
    acf_hip_ctx::InputResize rz;
    if (buildResizeTables(rows, cols, scale, rz.t) || rz.t.drows != dstRows || rz.t.dcols != dstCols)
    {
        return fail(c, ACF_HIP_E_INVALID, "op_resize_u8: dst size must be acf_hip_resize_dims(rows, cols, scale)");
    }
    const int stride = rowStride > 0 ? rowStride : cols * cpp;
    if (stride < cols * cpp)
    {
        return fail(c, ACF_HIP_E_INVALID, "op_resize_u8: row stride smaller than a row");
    }
    HIPCHK(c, hipSetDevice(c->device));
    const size_t nD = size_t(dstRows) * dstCols * cpp;
    Scratch s;
    auto up = [&](const std::vector<int32_t>& v) { return s.upload(v.data(), v.size()); };
    uint8_t *dS = s.upload(src, size_t(stride) * rows), *dD = s.alloc<uint8_t>(nD);
    rz.d_xlin = up(rz.t.xlin), rz.d_ylin = up(rz.t.ylin), rz.d_xrun = up(rz.t.xrun), rz.d_yrun = up(rz.t.yrun), rz.d_xtap = up(rz.t.xtap), rz.d_ytap = up(rz.t.ytap);
    if (!dS || !dD || !rz.d_xlin || !rz.d_ylin || !rz.d_xrun || !rz.d_yrun || !rz.d_xtap || !rz.d_ytap)
    {
        (void)hipGetLastError();
        return fail(c, ACF_HIP_E_HIP, "op_resize_u8: device allocation or copy failed");
    }
    if (int rc = launchResizeU8(c, rz, dS, cpp, stride, 1, dD))
    {
        return rc;
    }
    return Scratch::download(c, "op_resize_u8", dst, dD, nD);
}

int acf_hip_op_nms(acf_hip_ctx* c, const int32_t* boxes, const double* scores, int n, const acf_hip_nms_params* q, int32_t* keep_idx, int* count)
{
    if (int rc = needCtx(c)) return rc;
    if (!q || !count || n < 0 || (n > 0 && (!boxes || !scores || !keep_idx)))
    {
        return fail(c, ACF_HIP_E_INVALID, "op_nms: arguments");
    }
    int rc = checkNmsParams(c, q);
    if (rc)
    {
        return rc;
    }
    if (n == 0 || q->type == 0)
    {
        // bbNms returns its input for an empty list and for type "none" (bbNms.cpp:262-273); prune still applies to the caller
        for (int i = 0; i < n; i++)
        {
            keep_idx[i] = i;
        }
        *count = n;
        return ACF_HIP_OK;
    }
    if (n > NMS_CAP)
    {
        return fail(c, ACF_HIP_E_CAPACITY, "op_nms: more than ACF_HIP_NMS_CAP boxes");
    }
    HIPCHK(c, hipSetDevice(c->device));
    Scratch s;
    NmsArgs a{};
    a.boxes = s.upload(boxes, size_t(n) * 4);
    a.scores = s.upload(scores, size_t(n));
    a.nOp = n;
    fillNmsArgs(a, *q);
    a.keep = s.alloc<int32_t>(NMS_CAP);
    a.nKeep = s.alloc<int32_t>(1);
    if (!a.boxes || !a.scores || !a.keep || !a.nKeep)
    {
        (void)hipGetLastError();
        return fail(c, ACF_HIP_E_HIP, "op_nms: device allocation or copy failed");
    }
    if ((rc = allowLds(c, reinterpret_cast<const void*>(&k_nms), kNmsLds)))
    {
        return rc;
    }
    hipLaunchKernelGGL(k_nms, dim3(1), dim3(1024), kNmsLds, c->stream, a);
    if (const hipError_t e = hipGetLastError())
    {
        return fail(c, ACF_HIP_E_HIP, std::string("op_nms: ") + hipGetErrorString(e));
    }
    int32_t m = 0;
    if ((rc = Scratch::download(c, "op_nms", &m, a.nKeep, 1)) || (m > 0 && (rc = Scratch::download(c, "op_nms", keep_idx, a.keep, size_t(m)))))
    {
        return rc;
    }
    *count = m;
    return ACF_HIP_OK;
}

int acf_hip_op_rgb_convert(acf_hip_ctx* c, const float* in, float* out, int h, int w, int flag)
{
    if (int rc = opBegin(c)) return rc;
    if (!in || !out || h <= 0 || w <= 0)
    {
        return fail(c, ACF_HIP_E_INVALID, "op_rgb_convert: arguments");
    }
    const int n = h * w;
    Scratch s;
    float* di = s.upload(in, size_t(3) * n);
    const int dOut = flag == ACF_HIP_CS_GRAY ? 1 : 3;
    float* dout = s.alloc<float>(size_t(dOut) * n);
    if (!di || !dout)
    {
        return fail(c, ACF_HIP_E_HIP, "op_rgb_convert: allocation");
    }
    if (flag != ACF_HIP_CS_LUV && flag != ACF_HIP_CS_GRAY && flag != ACF_HIP_CS_HSV)
    {
        return fail(c, ACF_HIP_E_UNSUPPORTED, "op_rgb_convert: flag");
    }
    launchColour(c, di, dout, n, 1, 0, 0, flag, 3);
    LAUNCHCHK(c, "op_rgb_convert");
    return Scratch::download(c, "op_rgb_convert", out, dout, size_t(dOut) * n);
}

namespace
{
// convTri with a radius <= 1 (k_smooth_tri1) of the d planes of ONE h x w frame, tight, through a one-job SmoothJob; `who` prefixes the
// error texts
int smoothOne(acf_hip_ctx* c, Scratch& s, const char* who, const float* in, float* out, int h, int w, int d, int64_t fs, float p, bool aliased)
{
    SmoothJob j{};
    j.h = h;
    j.w = w;
    j.nplanes = d;
    j.out_cs = h;
    j.in_ps = int64_t(h) * w;
    j.out_ps = int64_t(h) * w;
    SmoothJob* dj = s.upload(&j, 1);
    if (!dj)
    {
        return fail(c, ACF_HIP_E_HIP, std::string(who) + ": allocation");
    }
    return launchSmooth(c, c->stream, in, out, dj, 1, d, h, fs, fs, 1, p, aliased);
}

// gradMag of ONE h x w plane I into M and O (k_grad_mag_strip), then convTri(M, normRad) into S through U when normRad > 0; `who`
// prefixes the launch's error text, normRadErr is the text for a normRad the plane is too small for
int gradMagOne(acf_hip_ctx* c, const char* who, const char* normRadErr, const float* I, float* M, float* O, float* U, float* S, int h, int w, int full,
    int normRad)
{
    hipLaunchKernelGGL(k_grad_mag_strip, dim3(cdiv(h, GM_ROWS), 1, 1), dim3(GM_ROWS), 0, c->stream, I, M, O, (const float*)c->d_acos, h, w, full, int64_t(0),
        int64_t(0), cdiv(w, GM_XT), x86T(c));
    LAUNCHCHK(c, std::string(who) + ": k_grad_mag");
    if (!normRad)
    {
        return ACF_HIP_OK;
    }
    if (std::min(h, w) < 4 || 2 * normRad + 1 >= std::min(h, w) || normRad < 2)
    {
        return fail(c, ACF_HIP_E_UNSUPPORTED, normRadErr);
    }
    return launchTri(c, c->stream, M, U, S, h, w, normRad, int64_t(h) * w, 1);
}
} // namespace

int acf_hip_op_conv_tri(acf_hip_ctx* c, const float* in, float* out, int h, int w, int d, double r, int aliased)
{
    if (int rc = opBegin(c)) return rc;
    if (!in || !out || h <= 0 || w <= 0 || d <= 0)
    {
        return fail(c, ACF_HIP_E_INVALID, "op_conv_tri: arguments");
    }
    const int m = std::min(h, w);
    if (m < 4 || (2 * r + 1) >= m)
    {
        return fail(c, ACF_HIP_E_UNSUPPORTED, "op_conv_tri: plane too small (sepFilter2D fallback, convTri.cpp:224-251)");
    }
    const int64_t np = int64_t(h) * w;
    Scratch s;
    float* di = s.upload(in, size_t(np) * d);
    float* dout = s.alloc<float>(size_t(np) * d);
    if (!di || !dout)
    {
        return fail(c, ACF_HIP_E_HIP, "op_conv_tri: allocation");
    }
    int rc;
    if (r > 0 && r <= 1.0)
    {
        if ((rc = smoothOne(c, s, "op_conv_tri", di, dout, h, w, d, 0, float(12.0 / r / (r + 2.0) - 2.0), aliased != 0)))
        {
            return rc;
        }
    }
    else if (r > 1)
    {
        const int ri = int(std::round(float(r)));
        if (ri >= m / 2)
        {
            return fail(c, ACF_HIP_E_INVALID, "op_conv_tri: mask larger than image (convTri.cpp:166-169)");
        }
        float* dU = s.alloc<float>(size_t(np) * d);
        if (!dU)
        {
            return fail(c, ACF_HIP_E_HIP, "op_conv_tri: allocation");
        }
        if ((rc = launchTri(c, c->stream, di, dU, dout, h, w, ri, np, d)))
        {
            return rc;
        }
    }
    else
    {
        return fail(c, ACF_HIP_E_UNSUPPORTED, "op_conv_tri: radius");
    }
    return Scratch::download(c, "op_conv_tri", out, dout, size_t(np) * d);
}

// the device's table functions on the host (kernels.hip.h: x86_rcp_bits), for the composed table of gm_inv_x86g
static uint32_t hostX86RcpBits(uint32_t u, const uint32_t* rcp4096)
{
    const uint32_t s = u & 0x80000000u, e = (u >> 23) & 0xffu, m = u & 0x7fffffu;
    if (e == 0xffu)
    {
        return m ? (u | 0x400000u) : s;
    }
    if (e == 0)
    {
        return s | 0x7f800000u;
    }
    const uint32_t t = rcp4096[m >> 11];
    const int re = int((t >> 23) & 0xffu) + 127 - int(e);
    return re <= 0 ? s : (s | (uint32_t(re) << 23) | (t & 0x7fffffu));
}

int acf_hip_set_x86_tables(acf_hip_ctx* c, const uint32_t* rcp4096, const uint32_t* rsqrt8192)
{
    if (int rc = opBegin(c)) return rc;
    if (!rcp4096 || !rsqrt8192)
    {
        return fail(c, ACF_HIP_E_INVALID, "set_x86_tables: null table");
    }
    dropGraph(c);
    if (!c->d_x86)
    {
        // (not one of the plan's buffers: it outlives a re-plan; freed by acf_hip_destroy)
        HIPCHK(c, hipMalloc(reinterpret_cast<void**>(&c->d_x86), X86_BUF_N * sizeof(uint32_t)));
        c->x86Owned = true;
    }
    HIPCHK(c, hipStreamSynchronize(c->stream)); // (a run in flight may be reading the previous tables)
    // [rcp 4096][rsqrt 8192][gradMag's pairs {RSQ[i], rcp(RSQ[i])} x 8192][rcp(1e10)] (kernels_channels.hip.h: gm_inv_x86g)
    std::vector<uint32_t> buf(X86_BUF_N, 0u);
    memcpy(buf.data(), rcp4096, 4096 * sizeof(uint32_t));
    memcpy(buf.data() + 4096, rsqrt8192, 8192 * sizeof(uint32_t));
    for (int i = 0; i < X86_GM_N; i++)
    {
        buf[size_t(X86_TABLE_N) + 2 * size_t(i)] = rsqrt8192[i];
        buf[size_t(X86_TABLE_N) + 2 * size_t(i) + 1] = hostX86RcpBits(rsqrt8192[i], rcp4096);
    }
    {
        const float big = 1e10f;
        uint32_t bb;
        memcpy(&bb, &big, 4);
        buf[size_t(X86_TABLE_N) + 2 * size_t(X86_GM_N)] = hostX86RcpBits(bb, rcp4096);
    }
    HIPCHK(c, hipMemcpy(c->d_x86, buf.data(), buf.size() * sizeof(uint32_t), hipMemcpyHostToDevice));
    for (acf_hip_ctx* k : c->kids)
    {
        k->d_x86 = c->d_x86;
    }
    return ACF_HIP_OK;
}

int acf_hip_selftest_x86(acf_hip_ctx* c, uint32_t first_bits, uint64_t count, uint32_t stride, uint64_t digest[3])
{
    if (int rc = opBegin(c)) return rc;
    if (!digest || !c->d_x86)
    {
        return fail(c, ACF_HIP_E_INVALID, "selftest_x86: install tables first (acf_hip_set_x86_tables)");
    }
    Scratch s;
    unsigned long long* d = s.alloc<unsigned long long>(3);
    if (!d)
    {
        return fail(c, ACF_HIP_E_HIP, "selftest_x86: allocation");
    }
    HIPCHK(c, hipMemset(d, 0, 3 * sizeof(unsigned long long)));
    hipLaunchKernelGGL(k_x86_digest, dim3(4096), dim3(256), 0, c->stream, (const uint32_t*)c->d_x86, first_bits, (unsigned long long)count, stride, d);
    LAUNCHCHK(c, "k_x86_digest");
    // ... and gradMag's one-read form against the two table functions over the same patterns (negative non-NaN ones skipped)
    hipLaunchKernelGGL(k_gm_x86_selftest, dim3(4096), dim3(256), 0, c->stream, (const uint32_t*)c->d_x86, first_bits, (unsigned long long)count, stride, d + 2);
    LAUNCHCHK(c, "k_gm_x86_selftest");
    unsigned long long out[3];
    if (int rc = Scratch::download(c, "selftest_x86", out, d, 3))
    {
        return rc;
    }
    digest[0] = out[0];
    digest[1] = out[1];
    digest[2] = out[2];
    return ACF_HIP_OK;
}

int acf_hip_selftest_gradmag(acf_hip_ctx* c, uint32_t first_bits, uint32_t last_bits, uint64_t* mismatches, uint32_t* first_bad_bits)
{
    if (int rc = opBegin(c)) return rc;
    if (!mismatches || last_bits < first_bits)
    {
        return fail(c, ACF_HIP_E_INVALID, "selftest_gradmag: arguments");
    }
    Scratch s;
    unsigned long long* d = s.alloc<unsigned long long>(2);
    if (!d)
    {
        return fail(c, ACF_HIP_E_HIP, "selftest_gradmag: allocation");
    }
    const unsigned long long init[2] = { 0ull, ~0ull };
    HIPCHK(c, hipMemcpy(d, init, sizeof(init), hipMemcpyHostToDevice));
    const unsigned long long count = (unsigned long long)(last_bits - first_bits) + 1ull;
    hipLaunchKernelGGL(k_gm_inv_selftest, dim3(4096), dim3(256), 0, c->stream, first_bits, count, d);
    LAUNCHCHK(c, "k_gm_inv_selftest");
    unsigned long long out[2];
    if (int rc = Scratch::download(c, "selftest_gradmag", out, d, 2))
    {
        return rc;
    }
    *mismatches = out[0];
    if (first_bad_bits)
    {
        *first_bad_bits = uint32_t(out[1]);
    }
    return ACF_HIP_OK;
}

int acf_hip_op_gradient_mag(acf_hip_ctx* c, const float* in, float* M, float* O, float* S_out, int h, int w, int normRad, double normConst, int full)
{
    if (int rc = opBegin(c)) return rc;
    if (!in || !M || !O || h < 2 || w < 2)
    {
        return fail(c, ACF_HIP_E_INVALID, "op_gradient_mag: arguments");
    }
    const int64_t np = int64_t(h) * w;
    Scratch s;
    float* di = s.upload(in, size_t(np));
    float *dM = s.alloc<float>(np), *dO = s.alloc<float>(np), *dU = s.alloc<float>(np), *dS = s.alloc<float>(np);
    if (!di || !dM || !dO || !dU || !dS)
    {
        return fail(c, ACF_HIP_E_HIP, "op_gradient_mag: allocation");
    }
    if (int rc = gradMagOne(c, "op_gradient_mag", "op_gradient_mag: normRad", di, dM, dO, dU, dS, h, w, full, normRad))
    {
        return rc;
    }
    if (normRad)
    {
        hipLaunchKernelGGL(k_norm, dim3(cdiv(np, 256)), dim3(256), 0, c->stream, dM, (const float*)dS, int(np), float(normConst), x86T(c));
        LAUNCHCHK(c, "k_norm");
    }
    int rc;
    if ((rc = Scratch::download(c, "op_gradient_mag", M, dM, size_t(np))) || (rc = Scratch::download(c, "op_gradient_mag", O, dO, size_t(np))))
    {
        return rc;
    }
    return S_out && normRad ? Scratch::download(c, "op_gradient_mag", S_out, dS, size_t(np)) : ACF_HIP_OK;
}

// Detector::chnsCompute (ACF.h:342-349, chnsCompute.cpp:146-338): the channels of ONE image at its own scale, no pyramid plan.
int acf_hip_chns_compute(acf_hip_ctx* c, const acf_hip_params* pIn, const float* in, int h, int w, int d, float* out, int64_t cap, int* nChnsOut, int* hCOut,
    int* wCOut)
{
    if (int rc = opBegin(c)) return rc;
    const acf_hip_params* pp = pIn ? pIn : (c->hasModel ? &c->p : nullptr);
    if (!pp)
    {
        return fail(c, ACF_HIP_E_INVALID, "chns_compute: no parameters (pass them, or set a model first)");
    }
    acf_hip_params p = *pp;
    if (!in || h <= 0 || w <= 0 || (d != 1 && d != 3 && d != 5)) // (5: the image's own M, O planes behind three image planes, chnsCompute.cpp:219-226)
    {
        return fail(c, ACF_HIP_E_INVALID, "chns_compute: arguments");
    }
    {
        std::string err;
        const int rcc = checkChnsParams(p, d, err); // (the checks acf_hip_plan makes on the same fields)
        if (rcc)
        {
            return fail(c, rcc, "chns_compute: " + err);
        }
    }
    if (p.nOrients < 1 || p.nOrients > 12)
    {
        return fail(c, ACF_HIP_E_UNSUPPORTED, "chns_compute: nOrients must be 1..12");
    }
    if (d == 1 && p.colorChn != 0)
    {
        return fail(c, ACF_HIP_E_INVALID, "chns_compute: colorChn of a 1-plane image must be 0 (gradientMag reads I[colorChn], chnsCompute.cpp:278-282)");
    }
    const int shrink = p.shrink;
    const int hc = h - h % shrink, wc = w - w % shrink; // crop so divisible by shrink (chnsCompute.cpp:203-217)
    // a 1-plane image is its own colour plane for gray and orig alike (rgbConvert.cpp:129-148); replicating it is chnsPyramid's rule only
    // (chnsPyramid.cpp:234-244)
    const int dcol = d == 1 ? 1 : colorPlanes(p), nC = numChannels(p, dcol);
    const int hs = hc / shrink, ws = wc / shrink;
    if (nChnsOut)
    {
        *nChnsOut = nC;
    }
    if (hCOut)
    {
        *hCOut = hs;
    }
    if (wCOut)
    {
        *wCOut = ws;
    }
    if (!out)
    {
        return ACF_HIP_OK; // (a size query)
    }
    if (hc < 2 || wc < 2 || hs < 1 || ws < 1)
    {
        return fail(c, ACF_HIP_E_INVALID, "chns_compute: image smaller than a cell");
    }
    if (cap < int64_t(nC) * hs * ws)
    {
        return fail(c, ACF_HIP_E_CAPACITY, "chns_compute: output buffer too small");
    }
    const int64_t np = int64_t(hc) * wc;
    Scratch s;
    // the cropped planes, tight: [d][wc][hc]
    std::vector<float> crop;
    const float* src = in;
    if (hc != h || wc != w)
    {
        crop.resize(size_t(d) * np);
        for (int z = 0; z < d; z++)
        {
            for (int x = 0; x < wc; x++)
            {
                memcpy(&crop[(size_t(z) * wc + x) * hc], in + (size_t(z) * w + x) * h, sizeof(float) * hc);
            }
        }
        src = crop.data();
    }
    float* dI = s.upload(src, size_t(d) * np);
    float* dCol = s.alloc<float>(size_t(dcol) * np);
    float *dM = s.alloc<float>(np), *dO = s.alloc<float>(np), *dU = s.alloc<float>(np), *dS = s.alloc<float>(np);
    float* dOut = s.alloc<float>(size_t(nC) * hs * ws);
    if (!dI || !dCol || !dM || !dO || !dU || !dS || !dOut)
    {
        return fail(c, ACF_HIP_E_HIP, "chns_compute: allocation");
    }
    // rgbConvert(I, I, colorSpace, true, isLuv) (chnsCompute.cpp:235; rgbConvert.cpp:101-170)
    if (d == 1 || colourPassthrough(p, d))
    {
        HIPCHK(c, hipMemcpyAsync(dCol, dI, sizeof(float) * dcol * np, hipMemcpyDeviceToDevice, c->stream));
    }
    else
    {
        launchColour(c, dI, dCol, np, 1, 0, 0, p.colorSpace, d);
        LAUNCHCHK(c, "chns_compute: colour conversion");
    }
    // convTri(I, I, pColor.smooth, 1) in place (chnsCompute.cpp:239)
    if (p.colorSmooth > 0)
    {
        if (p.colorSmooth > 1)
        {
            return fail(c, ACF_HIP_E_UNSUPPORTED, "chns_compute: pColor.smooth > 1 (convTri with a radius) is not built for the colour planes");
        }
        const float pColor = float(12.0 / p.colorSmooth / (p.colorSmooth + 2.0) - 2.0);
        if (int rc = smoothOne(c, s, "chns_compute", dCol, dCol, hc, wc, dcol, int64_t(dcol) * np, pColor, true))
        {
            return rc;
        }
    }
    ChnsArgs a{};
    a.sm = dCol;
    a.M = dM;
    a.S = dS;
    a.O = dO;
    a.chns = dOut;
    a.sm_fs = int64_t(dcol) * np;
    a.m_fs = np;
    a.chns_fs = int64_t(nC) * hs * ws;
    a.h = hc;
    a.w = wc;
    a.d = dcol;
    a.colorEnabled = p.colorEnabled;
    a.magEnabled = p.gradMagEnabled;
    a.histEnabled = p.gradHistEnabled;
    a.nOrients = p.nOrients;
    a.doNorm = p.normRad != 0;
    a.full = p.full;
    a.hardBin = p.softBin < 0;
    a.normConst = float(p.normConst);
    a.rq_y = shrinkGainY(shrink);
    a.x86 = x86T(c);
    if (d == 5)
    {
        // M = MO[0], O = MO[1] (chnsCompute.cpp:265-269): no gradientMag, no normalisation
        a.M = dI + 3 * np;
        a.O = dI + 4 * np;
        a.doNorm = 0;
    }
    else if (p.gradMagEnabled || p.gradHistEnabled)
    {
        if (int rc = gradMagOne(c, "chns_compute", "chns_compute: normRad against the image size", dCol + int64_t(p.colorChn) * np, dM, dO, dU, dS, hc, wc,
                p.full, p.normRad))
        {
            return rc;
        }
    }
    int rc = launchChns(c, c->stream, a, shrink, 1);
    if (rc)
    {
        return rc;
    }
    return Scratch::download(c, "chns_compute", out, dOut, size_t(nC) * hs * ws);
}

int acf_hip_op_gradient_hist(acf_hip_ctx* c, const float* M, const float* O, float* H, int h, int w, int bin, int nOrients, int softBin, int full)
{
    if (int rc = opBegin(c)) return rc;
    if (!M || !O || !H || h <= 0 || w <= 0 || nOrients < 1 || nOrients > 12)
    {
        return fail(c, ACF_HIP_E_INVALID, "op_gradient_hist: arguments");
    }
    if (softBin % 2 != 0)
    {
        return fail(c, ACF_HIP_E_UNSUPPORTED, "op_gradient_hist: odd softBin (trilinear spatial binning) is not built");
    }
    if ((bin != 2 && bin != 4) || h % bin || w % bin)
    {
        return fail(c, ACF_HIP_E_UNSUPPORTED, "op_gradient_hist: bin must be 2 or 4 and divide h, w");
    }
    const int64_t np = int64_t(h) * w, nc = np / (bin * bin);
    Scratch s;
    float *dM = s.upload(M, np), *dO = s.upload(O, np), *dH = s.alloc<float>(nc * nOrients);
    if (!dM || !dO || !dH)
    {
        return fail(c, ACF_HIP_E_HIP, "op_gradient_hist: allocation");
    }
    ChnsArgs a{};
    a.M = dM;
    a.S = dM;
    a.O = dO;
    a.chns = dH;
    a.h = h;
    a.w = w;
    a.d = 0;
    a.histEnabled = 1;
    a.nOrients = nOrients;
    a.full = full;
    a.hardBin = softBin < 0;
    a.rq_y = shrinkGainY(bin);
    int rc = launchChns(c, c->stream, a, bin, 1);
    if (rc)
    {
        return rc;
    }
    return Scratch::download(c, "op_gradient_hist", H, dH, size_t(nc) * nOrients);
}

// one output of the resample operators: the strip march where its plan holds, else k_resample_up, else the generic kernel
static int resampleOpLaunch(acf_hip_ctx* c, const ResampleDesc& dd, const StripPlan& sp, const ResampleDesc* ddescs, int desc, const float* di, float* dout,
    const int32_t* dit, const float* dft)
{
    if (sp.ok && !resampleGenericOnly())
    {
        // the strip march the pyramid uses for its down-sampled real scales
        if (int rc = ensureConstTables(c))
        {
            return rc;
        }
        launchStrip(c, c->stream, sp, ddescs, desc, -1, dd.nplanes, di, dout, nullptr, dit, dft, 1);
    }
    else if (resampleUpOk(dd) && !resampleGenericOnly())
    {
        hipLaunchKernelGGL(k_resample_up, dim3(cdiv(dd.nplanes * cdiv(dd.hb, 256) * cdiv(dd.wb, RSU_XC), 4), 1, 1), dim3(256), 0, c->stream, di, dout, ddescs + desc,
            dit, dft);
    }
    else
    {
        hipLaunchKernelGGL(k_resample, dim3(resampleBlocks(dd), 1, 1), dim3(64, 4), 0, c->stream, di, dout, ddescs + desc, dit, dft, RS_XT);
    }
    LAUNCHCHK(c, "k_resample");
    return ACF_HIP_OK;
}

int acf_hip_op_im_resample(acf_hip_ctx* c, const float* in, float* out, int ha, int wa, int hb, int wb, int d, double nrm)
{
    if (int rc = opBegin(c)) return rc;
    if (!in || !out || ha <= 0 || wa <= 0 || hb <= 0 || wb <= 0 || d <= 0)
    {
        return fail(c, ACF_HIP_E_INVALID, "op_im_resample: arguments");
    }
    TableArena arena;
    ResampleDesc dd;
    int rc = buildResample(ha, wa, hb, wb, dd, arena);
    if (rc)
    {
        return fail(c, rc, "op_im_resample: degenerate geometry");
    }
    const double ratio[3] = { nrm, nrm, nrm };
    setResampleGain(dd, ratio, d, d);
    dd.nplanes = d;
    Scratch s;
    float* di = s.upload(in, size_t(d) * ha * wa);
    float* dout = s.alloc<float>(size_t(d) * hb * wb);
    dd.src_frame_stride = int64_t(d) * ha * wa;
    dd.dst_frame_stride = int64_t(d) * hb * wb;
    const StripPlan sp = stripPlan(dd, nullptr, arena); // appends its tile ranges to the int arena
    ResampleDesc* ddesc = s.upload(&dd, 1);
    int32_t* dit = s.upload(arena.ints.data(), arena.ints.size());
    float* dft = s.upload(arena.floats.data(), arena.floats.size());
    if (!di || !dout || !ddesc || !dit || !dft)
    {
        return fail(c, ACF_HIP_E_HIP, "op_im_resample: allocation");
    }
    if ((rc = resampleOpLaunch(c, dd, sp, ddesc, 0, di, dout, dit, dft)))
    {
        return rc;
    }
    return Scratch::download(c, "op_im_resample", out, dout, size_t(d) * hb * wb);
}

// Tests only: the two-output form of k_resample_strip, planned as PlanBuild::imageStrips plans two real scales of one source
int acf_hip_op_im_resample_pair(acf_hip_ctx* c, const float* in, float* outA, float* outB, int ha, int wa, int hbA, int wbA, int hbB, int wbB, int d, double nrm,
    uint64_t* word)
{
    if (int rc = opBegin(c)) return rc;
    if (!in || !outA || !outB || !word || ha <= 0 || wa <= 0 || hbA <= 0 || wbA <= 0 || hbB <= 0 || wbB <= 0 || d <= 0 || hbB > hbA || wbB > wbA)
    {
        return fail(c, ACF_HIP_E_INVALID, "op_im_resample_pair: arguments");
    }
    TableArena arena;
    ResampleDesc dd[2];
    const int hb[2] = { hbA, hbB }, wb[2] = { wbA, wbB };
    const double ratio[3] = { nrm, nrm, nrm };
    for (int i = 0; i < 2; i++)
    {
        if (int rc = buildResample(ha, wa, hb[i], wb[i], dd[i], arena))
        {
            return fail(c, rc, "op_im_resample_pair: degenerate geometry");
        }
        setResampleGain(dd[i], ratio, d, d);
        dd[i].nplanes = d;
        dd[i].src_frame_stride = int64_t(d) * ha * wa;
        dd[i].dst_frame_stride = int64_t(d) * hb[i] * wb[i];
    }
    // (every plan appends its tile ranges to the int arena: all of them before the upload)
    const StripPlan pair = resampleGenericOnly() ? StripPlan{} : stripPlan(dd[0], &dd[1], arena);
    StripPlan one[2];
    for (int i = 0; i < 2 && !pair.ok; i++)
    {
        one[i] = stripPlan(dd[i], nullptr, arena);
    }
    Scratch s;
    float* di = s.upload(in, size_t(d) * ha * wa);
    float* dout[2] = { s.alloc<float>(size_t(d) * hbA * wbA), s.alloc<float>(size_t(d) * hbB * wbB) };
    ResampleDesc* ddesc = s.upload(dd, 2);
    int32_t* dit = s.upload(arena.ints.data(), arena.ints.size());
    float* dft = s.upload(arena.floats.data(), arena.floats.size());
    if (!di || !dout[0] || !dout[1] || !ddesc || !dit || !dft)
    {
        return fail(c, ACF_HIP_E_HIP, "op_im_resample_pair: allocation");
    }
    int rc;
    if (pair.ok)
    {
        if ((rc = ensureConstTables(c)))
        {
            return rc;
        }
        const int nSplit = launchStrip(c, c->stream, pair, ddesc, 0, 1, d, di, dout[0], dout[1], dit, dft, 1);
        LAUNCHCHK(c, "k_resample_strip(pair)");
        auto f = [](int v, int bits) { return uint64_t(std::min(v, (1 << bits) - 1)); };
        *word = (pair.slowRows > 0 ? uint64_t(ACF_HIP_SF_SLOW) : 0) | f(pair.nty, 8) << 8 | f(pair.ntyB, 8) << 16 | f(nSplit, 8) << 24 | f(pair.nSteps, 16) << 32 |
            f(pair.nStepsB, 16) << 48;
    }
    else
    {
        *word = uint64_t(pair.why);
        for (int i = 0; i < 2; i++)
        {
            if ((rc = resampleOpLaunch(c, dd[i], one[i], ddesc, i, di, dout[i], dit, dft)))
            {
                return rc;
            }
        }
    }
    if ((rc = Scratch::download(c, "op_im_resample_pair", outA, dout[0], size_t(d) * hbA * wbA)))
    {
        return rc;
    }
    return Scratch::download(c, "op_im_resample_pair", outB, dout[1], size_t(d) * hbB * wbB);
}

// thrs.convertTo(thrsU8, CV_8UC1, 255.0f) (ACFIOArchive.h:96-99): OpenCV's 32f->8u cvtScale works in f32 and rounds
// with cvRound (to nearest even), then saturates.
int acf_hip_thrs_u8(const float* thrs, int n, uint8_t* out)
{
    if (!thrs || !out || n < 0)
    {
        return ACF_HIP_E_INVALID;
    }
    for (int i = 0; i < n; i++)
    {
        const float v = thrs[i] * 255.0f;
        // cvRound is cvtss2si: half to even; NaN and |v| >= 2^31 convert to INT_MIN, which saturate_cast<uchar> maps to 0
        const bool inRange = v > -2147483648.0f && v < 2147483648.0f;
        const float r = inRange ? std::nearbyint(v) : -1.0f;
        out[i] = uint8_t(r < 0.f ? 0 : (r > 255.f ? 255 : int(r)));
    }
    return ACF_HIP_OK;
}

// acfDetect1 on one caller's channel buffer: a cascade state of its own (one level, one frame, cap hits), built, run and freed
// here.  The plan's state, its batch and its resident results are not touched.  thrs == nullptr: the model's thresholds.
// rank: the call as acf_hip_detect makes it on a plan's pyramid with rank cells (acf_hip_op_acf_detect1_rank) — the rank set built
// with the tables, the rank cells made from the caller's floats by runCascade's ensureRankCells; refused where the call would
// not read them.
static int opAcfDetect1(acf_hip_ctx* c, const void* chns, bool u8, const std::vector<float>* thrs, int hP, int wP, int nChns, acf_hip_hit* out, int cap, int* count,
    bool rank = false)
{
    if (int rc = opBegin(c)) return rc;
    if (int rc = needModel(c, "op_acf_detect1")) return rc;
    if (!chns || hP <= 0 || wP <= 0 || nChns <= 0 || cap <= 0 || !count)
    {
        return fail(c, ACF_HIP_E_INVALID, "op_acf_detect1: arguments");
    }
    const acf_hip_params& p = c->p;
    std::vector<acf_hip_level> lv(1);
    lv[0] = acf_hip_level{};
    lv[0].scale = 1.0;
    lv[0].scalehw_h = lv[0].scalehw_w = 1.0;
    lv[0].hP = lv[0].hC = hP;
    lv[0].wP = lv[0].wC = wP;
    lv[0].nWinR = std::max(0, int(std::ceil(float(hP * p.shrink - p.modelDsPad_h + 1) / p.stride)));
    lv[0].nWinC = std::max(0, int(std::ceil(float(wP * p.shrink - p.modelDsPad_w + 1) / p.stride)));
    lv[0].offset = 0;
    std::vector<BoxLevel> box(1);
    box[0].shw_h = box[0].shw_w = 1.0;
    box[0].bw = p.modelDs_w;
    box[0].bh = p.modelDs_h;
    const AllocMark temporaries{ c, c->allocs.size() }; // (what the cascade builders allocate into the context, for this call only)
    const std::vector<float>& th = thrs ? *thrs : c->thrs;
    const size_t n = size_t(nChns) * hP * wP;
    CascState cs;
    BoxLevel* dBox = nullptr;
    float* dChn = nullptr;
    uint8_t* dBytes = nullptr;
    int rc;
    if ((rc = buildCascadeTables(c, lv, nChns, p.shrink, 1, th, cs, rank)) || (rc = allocCascadeRun(c, cs, lv, th, cap)) || (rc = devUpload(c, &dBox, box)) ||
        (rc = devAlloc(c, &dChn, n + 64)) || (u8 && (rc = devAlloc(c, &dBytes, n))))
    {
        return rc;
    }
    if (hipMemcpy(u8 ? static_cast<void*>(dBytes) : dChn, chns, n * (u8 ? 1 : sizeof(float)), hipMemcpyHostToDevice) != hipSuccess)
    {
        return fail(c, ACF_HIP_E_HIP, u8 ? "op_acf_detect1_u8: upload" : "op_acf_detect1: upload");
    }
    if (u8)
    {
        hipLaunchKernelGGL(k_widen_u8, dim3(cdiv(int64_t(n), 256)), dim3(256), 0, c->stream, (const uint8_t*)dBytes, dChn, int64_t(n));
        if (hipGetLastError() != hipSuccess)
        {
            return fail(c, ACF_HIP_E_HIP, "launch k_widen_u8");
        }
    }
    const CascInput in = { dChn, 0, 1, nChns };
    if (rank && !planCascadeCall(c, cs, in, true).rank)
    {
        return fail(c, ACF_HIP_E_UNSUPPORTED, "op_acf_detect1_rank: this model, buffer and these options give no cascade on rank cells");
    }
    bool ranksWritten = false; // (the caller's buffer has floats only: k_rank runs)
    if ((rc = runCascade(c, cs, in, dBox, rank ? &ranksWritten : nullptr)))
    {
        return rc;
    }
    prof(c, c->stream, "(end)");
    int nHits = 0;
    if (hipStreamSynchronize(c->stream) != hipSuccess || hipMemcpy(&nHits, cs.d_counts, sizeof(int), hipMemcpyDeviceToHost) != hipSuccess)
    {
        return fail(c, ACF_HIP_E_HIP, "op_acf_detect1: sync");
    }
    *count = nHits;
    const int m = std::min(nHits, cap);
    if (m > 0 && out && hipMemcpy(out, cs.d_sorted, sizeof(acf_hip_hit) * m, hipMemcpyDeviceToHost) != hipSuccess)
    {
        return fail(c, ACF_HIP_E_HIP, "op_acf_detect1: download");
    }
    return nHits > cap ? fail(c, ACF_HIP_E_CAPACITY, "op_acf_detect1: more hits than cap") : ACF_HIP_OK;
}

int acf_hip_op_acf_detect1(acf_hip_ctx* c, const float* chns, int hP, int wP, int nChns, acf_hip_hit* out, int cap, int* count)
{
    return opAcfDetect1(c, chns, false, nullptr, hP, wP, nChns, out, cap, count);
}

// Tests only: the same call with rank cells standing for the floats
int acf_hip_op_acf_detect1_rank(acf_hip_ctx* c, const float* chns, int hP, int wP, int nChns, acf_hip_hit* out, int cap, int* count)
{
    return opAcfDetect1(c, chns, false, nullptr, hP, wP, nChns, out, cap, count, true);
}

// The uint8_t body of acfDetect1 (acfDetect1.cpp:157-166,187-192): features and thresholds are bytes, compared after
// promotion to float (`float ftr = chns1[...]; ftr < thrs[k]`).  Bytes widen to f32 exactly, so the planes are widened
// on the device and the f32 cascade runs on them with the widened thresholds: same comparisons, same sums.
int acf_hip_op_acf_detect1_u8(acf_hip_ctx* c, const uint8_t* chns, int hP, int wP, int nChns, const uint8_t* thrsU8, acf_hip_hit* out, int cap, int* count)
{
    if (int rc = needModel(c, "op_acf_detect1_u8")) return rc;
    std::vector<uint8_t> derived;
    if (!thrsU8)
    {
        derived.resize(c->thrs.size());
        acf_hip_thrs_u8(c->thrs.data(), int(c->thrs.size()), derived.data());
        thrsU8 = derived.data();
    }
    std::vector<float> wide(c->thrs.size());
    for (size_t i = 0; i < wide.size(); i++)
    {
        wide[i] = float(thrsU8[i]);
    }
    return opAcfDetect1(c, chns, true, &wide, hP, wP, nChns, out, cap, count);
}

int acf_hip_op_evaluate(acf_hip_ctx* c, const float* chns, int hP, int wP, int nChns, double cascThr, float* score)
{
    if (int rc = opBegin(c)) return rc;
    if (int rc = needModel(c, "op_evaluate")) return rc;
    const acf_hip_params& p = c->p;
    const int mH = p.modelDsPad_h / p.shrink, mW = p.modelDsPad_w / p.shrink;
    if (!chns || !score || nChns <= 0 || hP < mH || wP < mW)
    {
        return fail(c, ACF_HIP_E_INVALID, "op_evaluate: the buffer must hold at least one window");
    }
    {
        // before anything is allocated or launched: every test's feature id lies inside the nChns planes of the window
        std::string why;
        if (const int rc = checkModel(p, nChns, p.shrink, why))
        {
            return fail(c, rc, "op_evaluate: " + why);
        }
    }
    Scratch s;
    const size_t n = size_t(nChns) * hP * wP;
    float* dC = s.upload(chns, n);
    uint32_t* dF = s.upload(c->fids.data(), c->fids.size());
    float* dT = s.upload(c->thrs.data(), c->thrs.size());
    float* dH = s.upload(c->hs.data(), c->hs.size());
    uint32_t* dCh = c->child.empty() ? nullptr : s.upload(c->child.data(), c->child.size());
    float* dS = s.alloc<float>(1);
    if (!dC || !dF || !dT || !dH || !dS || (p.treeDepth == 0 && !dCh))
    {
        return fail(c, ACF_HIP_E_HIP, "op_evaluate: allocation");
    }
    hipLaunchKernelGGL(k_evaluate_window, dim3(1), dim3(64), 0, c->stream, (const float*)dC, hP, wP, mH, mW, (const uint32_t*)dF, (const float*)dT,
        (const float*)dH, (const uint32_t*)dCh, p.nTrees, p.nTreeNodes, p.treeDepth, float(cascThr), dS);
    LAUNCHCHK(c, "k_evaluate_window");
    return Scratch::download(c, "op_evaluate", score, dS, 1);
}
