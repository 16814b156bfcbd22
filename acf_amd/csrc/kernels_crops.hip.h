// kernels_crops.hip.h — part of kernels.hip.h (included from there, after the parts whose __device__ arithmetic it calls).
// Detector::evaluate(const cv::Mat&) for a batch of window-sized crops (ACF.cpp:123-133 = computeChannels + evaluate(MatP),
// acfDetect1.cpp:337-342): acf_hip_evaluate_crops / _u8 (crops_run.hip.h).
//
//   k_crop_score          the fused form: a workgroup takes crops in turn (grid-stride over the batch); a crop enters LDS once, straight
//                         from its floats or bytes, every stage of chnsCompute runs there and only the 4-byte score leaves.
//   k_crop_gather(_u8)    the staged form's first step: the cropped planes of every crop, tight, as a batch of frames for the kernels
//                         acf_hip_chns_compute launches
//   k_evaluate_windows    the staged form's last step: k_evaluate_window for a batch, one wave per crop
//
// Both forms give the bits of acf_hip_chns_compute + acf_hip_op_evaluate per crop.  k_crop_score calls the arithmetic the staged
// kernels hold (luv_px, hsv_px, gm_inv_fast / gm_inv_x86, x86_rcp, hist_add2, tree_leaf) and restates, in their association order,
// the loops that exist only as whole kernels: k_smooth_tri1<., true>'s aliased column recursion, k_grad_mag_strip's pixel,
// k_tri_x / k_tri_y's running sums and k_chns's cell sums (citations at each).  It carries every channel option
// acf_hip_chns_compute takes, option "arith" included, for 1- and 3-plane crops; which crops it takes is cropFusedFits's decision
// (LDS and workgroup size), nothing else.
//
// LDS of k_crop_score, in floats (pitch = hc | 1: odd, so lanes along y (stride 1) and lanes along x (stride pitch) both fall on
// distinct banks of the 64):
//   plane[4][wc * pitch]   slots 0 .. dcol-1 the colour planes; after the colour cells are taken gradMag writes M and O over the
//                          two colour planes it does not read (dcol = 1: slots 1, 2), convTri's x pass then writes U over the
//                          plane gradMag read, its y pass S into slot 3
//   T[2][dcol * hc]        convTri1's column of row sums, double-buffered by column parity (one barrier per column)
//   cells[nC][mW][mH]      the channels of the window at (0, 0) only: a feature id indexes it directly
//   leaf[blockDim]         the leaves' values of one chunk of trees; then one int: the chunk ended the cascade
// The acos table (80 KB), rgb2luv's table and the "arith" tables stay in global memory: every workgroup reads the same ones (L2).
#pragma once

namespace acfhip
{

enum
{
    CR_PASS = 0,    // the planes are the colour planes as they are
    CR_LUV_VEC = 1, // rgb2luv_sse body (pixels % 4 == 0)
    CR_LUV = 2,     // scalar rgb2luv
    CR_GRAY = 3,
    CR_HSV = 4
};

struct CropArgs
{
    const float* inF;   // float entry: n x [d][w][h]
    const uint8_t* inU8; // 8-bit entry (inF null): n upright packed images, rowStride bytes a row, in_fs bytes apart
    float* scores;
    int32_t n, h, w, d; // as given (d: planes of the image)
    int32_t hc, wc;     // cropped to multiples of shrink
    int32_t dcol;       // colour planes after the conversion
    int32_t cpp, ro, go, bo, rowStride;
    int64_t in_fs;      // floats (float entry) or bytes between crops
    int32_t conv;       // CR_*
    const float* lTable;
    LuvConsts k;
    float mr, mg, mb;
    const float* acos; // the table's first entry (its centre is + 10010)
    const uint32_t* x86; // option "arith", or null
    int32_t smooth;    // pColor.smooth > 0
    float smoothP;
    int32_t colorChn, colorEnabled, magEnabled, histEnabled, nOrients, full, hardBin, normRad;
    float normConst, rq_y;
    int32_t pitch;
    int32_t mH, mW, nC; // window cells, channels
    const uint32_t* fids;
    const float* thrs;
    const float* hs;
    const uint32_t* child;
    int32_t nTrees, nTreeNodes, depth;
    float cascThr;
};

// floats of dynamic LDS k_crop_score<..> takes with nt threads (the layout above)
__host__ __device__ inline int64_t cropLdsFloats(int hc, int wc, int dcol, int nC, int mH, int mW, int nt)
{
    return 4 * int64_t(hc | 1) * wc + 2 * int64_t(dcol) * hc + int64_t(nC) * mH * mW + nt + 4;
}

// one pixel of gradMag (gradientMex.cpp:17-87,168-251) as k_grad_mag_strip / k_grad_mag_vec compute it: l, r the x neighbours, u, d the
// y neighbours (clamped at the borders), rx, ry 1 at a border and .5 inside; acosT the table's centre
__device__ __forceinline__ void crop_grad_px(float l, float r, float u, float d, float rx, float ry, const float* __restrict__ acosT, int full,
    const uint32_t* __restrict__ x86, float& Mo, float& Oo)
{
    const float gx = (r - l) * rx;
    const float gy = (d - u) * ry;
    const float m2 = gx * gx + gy * gy;
    float m;
    if (x86)
    {
        gm_inv_x86(m2, m, Mo, x86);
    }
    else
    {
        gm_inv_fast(m2, m, Mo);
    }
    float g = (gx * m) * 10000.0f;
    g = __int_as_float(__float_as_int(g) ^ (__float_as_int(gy) & 0x80000000));
    g = g < 10009.0f ? g : 10009.0f;
    g = g > -10009.0f ? g : -10009.0f;
    float ov = acosT[(int)g];
    if (full)
    {
        ov += (gy < 0) * 3.14159265f;
    }
    Oo = ov;
}

// addChn's shrink of one S x S cell of a plane (k_chns: x inner per row, then the rows; imResampleMex.cpp:210-215, 312-317)
template <int S>
__device__ __forceinline__ float crop_cell_sum(const float* __restrict__ P, int pitch, float rq_y)
{
    float C[S];
#pragma unroll
    for (int yy = 0; yy < S; yy++)
    {
        float s = P[yy];
#pragma unroll
        for (int xx = 1; xx < S; xx++)
        {
            s = s + P[xx * pitch + yy];
        }
        C[yy] = s;
    }
    float s = C[0];
#pragma unroll
    for (int yy = 1; yy < S; yy++)
    {
        s = s + C[yy];
    }
    return s * rq_y;
}

// The trees of one window in chunks of nt: every thread walks one tree of the chunk (the leaves do not depend on each other), thread 0
// adds their values in tree order and stops where k_evaluate_window stops.  leaf: nt floats and one int behind them.  Ends with a
// barrier; every thread returns, thread 0 with the score.
__device__ __forceinline__ float crop_cascade(const float* chns, int area, int hP, int mH, int mW, const uint32_t* __restrict__ fids,
    const float* __restrict__ thrs, const float* __restrict__ hs, const uint32_t* __restrict__ child, int nTrees, int nTreeNodes, int depth, float cascThr,
    float* leaf, int tid, int nt)
{
    int* stop = reinterpret_cast<int*>(leaf + nt);
    float h = 0.f;
    for (int t0 = 0; t0 < nTrees; t0 += nt)
    {
        if (t0 + tid < nTrees)
        {
            leaf[tid] = hs[tree_leaf(chns, area, hP, mH, mW, fids, thrs, child, nTreeNodes, depth, t0 + tid)];
        }
        __syncthreads();
        if (tid == 0)
        {
            // (sixteen leaves into registers at a time: the additions stay in tree order, only the LDS reads' latencies overlap)
            const int m = min(nt, nTrees - t0);
            int st = 0;
            for (int q0 = 0; q0 < m && !st; q0 += 16)
            {
                float v[16];
#pragma unroll
                for (int j = 0; j < 16; j++)
                {
                    v[j] = leaf[min(q0 + j, m - 1)];
                }
#pragma unroll
                for (int j = 0; j < 16; j++)
                {
                    if (!st && q0 + j < m)
                    {
                        h += v[j];
                        st = h <= cascThr;
                    }
                }
            }
            *stop = st;
        }
        __syncthreads();
        if (*stop)
        {
            break;
        }
    }
    __syncthreads();
    return h;
}

template <int S, int MAXO>
__global__ void __launch_bounds__(1024) k_crop_score(CropArgs a)
{
    extern __shared__ float cr_lds[];
    const int tid = threadIdx.x, nt = blockDim.x;
    const int hc = a.hc, wc = a.wc, pitch = a.pitch, dcol = a.dcol;
    const int ps = pitch * wc, np = hc * wc;
    float* const P = cr_lds;
    float* const Tb = P + 4 * ps;
    float* const cells = Tb + 2 * dcol * hc;
    const int wcells = a.mW * a.mH;
    float* const leaf = cells + a.nC * wcells;
    const float* acosT = a.acos + 10010;
    const int sI = a.colorChn, sM = dcol == 3 ? (a.colorChn + 1) % 3 : 1, sO = dcol == 3 ? (a.colorChn + 2) % 3 : 2, sU = sI, sS = 3;
    const bool grad = a.magEnabled || a.histEnabled;
    for (int crop = blockIdx.x; crop < a.n; crop += gridDim.x)
    {
        // ---- the crop's pixels, through rgbConvert (chnsCompute.cpp:203-235), into the colour planes
        for (int i = tid; i < np; i += nt)
        {
            float r, g = 0.f, b = 0.f;
            int x, y;
            if (a.inF)
            {
                x = i / hc, y = i - x * hc; // lanes along image-y: the planes' contiguous direction
                const float* I = a.inF + int64_t(crop) * a.in_fs + int64_t(x) * a.h + y;
                r = I[0];
                if (a.d == 3)
                {
                    g = I[int64_t(a.h) * a.w];
                    b = I[2 * int64_t(a.h) * a.w];
                }
            }
            else
            {
                y = i / wc, x = i - y * wc; // lanes along image-x: the bytes' contiguous direction
                const uint8_t* px = a.inU8 + int64_t(crop) * a.in_fs + int64_t(y) * a.rowStride + x * a.cpp;
                const float sc = float(1.0 / 255.0); // cvt8UC3To32FC3, as k_ingest_u8
                r = float(px[a.ro]) * sc;
                if (a.d == 3)
                {
                    g = float(px[a.go]) * sc;
                    b = float(px[a.bo]) * sc;
                }
            }
            float o0 = r, o1 = g, o2 = b;
            if (a.conv == CR_LUV_VEC)
            {
                luv_px<true>(r, g, b, a.lTable, a.k, o0, o1, o2, a.x86);
            }
            else if (a.conv == CR_LUV)
            {
                luv_px<false>(r, g, b, a.lTable, a.k, o0, o1, o2, a.x86);
            }
            else if (a.conv == CR_GRAY)
            {
                o0 = r * a.mr + g * a.mg + b * a.mb; // rgbConvertMex.cpp:241-252
            }
            else if (a.conv == CR_HSV)
            {
                hsv_px(r, g, b, o0, o1, o2);
            }
            float* d = P + x * pitch + y;
            d[0] = o0;
            if (dcol == 3)
            {
                d[ps] = o1;
                d[2 * ps] = o2;
            }
        }
        __syncthreads();
        // ---- convTri(I, I, pColor.smooth, 1) in place (chnsCompute.cpp:239; convConst.cpp:445-525): k_smooth_tri1<., true>'s column
        // recursion, a thread per (plane, row); the left neighbour of column i is column i - 1's OUTPUT (the reference's aliasing)
        if (a.smooth)
        {
            const int items = dcol * hc; // <= nt (cropFusedFits)
            const bool act = tid < items;
            const int z = act ? tid / hc : 0, y = act ? tid - z * hc : 0;
            float* Pz = P + z * ps + y;
            const float p = a.smoothP, nrm = 1.0f / ((p + 2) * (p + 2)), p1 = 1 + p;
            const int ym = max(y - 1, 0), yp = min(y + 1, hc - 1);
            float prev = 0.f;
            for (int i = 0; i < wc; i++)
            {
                float* Tz = Tb + (i & 1) * items + z * hc;
                float T = 0.f;
                if (act)
                {
                    const float Im = Pz[i * pitch];
                    const float Ir = Pz[min(i + 1, wc - 1) * pitch];
                    const float Il = i == 0 ? Im : prev;
                    T = nrm * (Il + p * Im + Ir);
                    Tz[y] = T;
                }
                __syncthreads();
                if (act)
                {
                    const float tm = Tz[ym], tp = Tz[yp];
                    const float mid = tm + p * T + tp;
                    const float top = p1 * T + tp;
                    const float bot = tm + p1 * T;
                    const float o = y == 0 ? top : (y == hc - 1 ? bot : mid);
                    prev = o;
                    Pz[i * pitch] = o;
                }
            }
            __syncthreads();
        }
        // ---- the colour channels' cells (addChn's shrink), before M and O take the planes' room
        int ch = 0;
        if (a.colorEnabled)
        {
            for (int i = tid; i < dcol * wcells; i += nt)
            {
                const int z = i / wcells, cell = i - z * wcells;
                const int xc = cell / a.mH, yc = cell - xc * a.mH;
                cells[i] = crop_cell_sum<S>(P + z * ps + xc * S * pitch + yc * S, pitch, a.rq_y);
            }
            ch = dcol;
            __syncthreads();
        }
        if (grad)
        {
            // ---- gradientMag of plane colorChn (chnsCompute.cpp:263-283)
            const float* I = P + sI * ps;
            for (int i = tid; i < np; i += nt)
            {
                const int x = i / hc, y = i - x * hc;
                const int xl = max(x - 1, 0), xr = min(x + 1, wc - 1), yu = max(y - 1, 0), yd = min(y + 1, hc - 1);
                const float rx = (x == 0 || x == wc - 1) ? 1.f : .5f, ry = (y == 0 || y == hc - 1) ? 1.f : .5f;
                float M, O;
                crop_grad_px(I[xl * pitch + y], I[xr * pitch + y], I[x * pitch + yu], I[x * pitch + yd], rx, ry, acosT, a.full, a.x86, M, O);
                P[sM * ps + x * pitch + y] = M;
                P[sO * ps + x * pitch + y] = O;
            }
            __syncthreads();
            if (a.normRad > 0)
            {
                // ---- S = convTri(M, normRad): k_tri_x's running sums along x (a thread per row), k_tri_y's down the columns (a thread
                // per column) — convConst.cpp:347-442, 269-297
                const int r = a.normRad + 1;
                for (int y = tid; y < hc; y += nt)
                {
                    const float* Ir = P + sM * ps + y;
                    float* Uc = P + sU * ps + y;
                    const float nrm = 1.0f / (r * r * r * r);
                    float T, U;
                    U = T = Ir[0];
                    for (int i = 1; i < r; i++)
                    {
                        T += Ir[i * pitch];
                        U += T;
                    }
                    U = nrm * (2 * U - T);
                    T = 0;
                    Uc[0] = U;
                    for (int i = 1; i < wc; i++)
                    {
                        const float Il = (i <= r) ? Ir[(r - i) * pitch] : Ir[(i - 1 - r) * pitch];
                        const float Im = Ir[(i - 1) * pitch];
                        const float Iq = (i > wc - r) ? Ir[(2 * wc - r - i) * pitch] : Ir[(i - 1 + r) * pitch];
                        T += Il + Iq - 2 * Im;
                        U += nrm * T;
                        Uc[i * pitch] = U;
                    }
                }
                __syncthreads();
                const int r0 = r - 1, r1 = r + 1, r2 = 2 * hc - r, h0 = r + 1, h1 = hc - r + 1;
                for (int x = tid; x < wc; x += nt)
                {
                    const float* col = P + sU * ps + x * pitch;
                    float* oc = P + sS * ps + x * pitch;
                    float t, u;
                    u = t = col[0];
                    for (int q = 1; q < r; q++)
                    {
                        t += col[q];
                        u += t;
                    }
                    u = 2 * u - t;
                    t = 0;
                    oc[0] = u;
                    for (int j = 1; j < hc; j++)
                    {
                        const float aa = (j < h0) ? col[r - j] : col[j - r1];
                        const float bb = (j < h1) ? col[r0 + j] : col[r2 - j];
                        t += aa + bb - 2 * col[j - 1];
                        u += t;
                        oc[j] = u;
                    }
                }
                __syncthreads();
            }
            // ---- gradMagNorm, the magnitude channel and gradHist per cell (k_chns: gradientMex.cpp:254-275, 278-372), addChn's shrink
            for (int cell = tid; cell < wcells; cell += nt)
            {
                const int xc = cell / a.mH, yc = cell - xc * a.mH;
                const int pb = xc * S * pitch + yc * S;
                const float *Mp = P + sM * ps + pb, *Op = P + sO * ps + pb, *Sp = P + sS * ps + pb;
                float mn[S][S], ov[S][S];
#pragma unroll
                for (int xx = 0; xx < S; xx++)
                {
#pragma unroll
                    for (int yy = 0; yy < S; yy++)
                    {
                        float m = Mp[xx * pitch + yy];
                        ov[xx][yy] = Op[xx * pitch + yy];
                        if (a.normRad > 0)
                        {
                            const float s = Sp[xx * pitch + yy];
                            m = a.x86 ? m * x86_rcp(s + a.normConst, a.x86) : m * (1.0f / (s + a.normConst));
                        }
                        mn[xx][yy] = m;
                    }
                }
                int c2 = ch;
                if (a.magEnabled)
                {
                    float C[S];
#pragma unroll
                    for (int yy = 0; yy < S; yy++)
                    {
                        float s = mn[0][yy];
#pragma unroll
                        for (int xx = 1; xx < S; xx++)
                        {
                            s = s + mn[xx][yy];
                        }
                        C[yy] = s;
                    }
                    float s = C[0];
#pragma unroll
                    for (int yy = 1; yy < S; yy++)
                    {
                        s = s + C[yy];
                    }
                    cells[c2 * wcells + cell] = s * a.rq_y;
                    c2++;
                }
                if (a.histEnabled)
                {
                    float H[MAXO];
#pragma unroll
                    for (int bI = 0; bI < MAXO; bI++)
                    {
                        H[bI] = 0.f;
                    }
                    const float oMult = (float)a.nOrients / (a.full ? 2 * 3.14159265f : 3.14159265f);
                    const float sInv2 = 1 / (float)S / (float)S;
                    const int nO = a.nOrients;
#pragma unroll
                    for (int xx = 0; xx < S; xx++)
                    {
#pragma unroll
                        for (int yy = 0; yy < S; yy++)
                        {
                            const float o = ov[xx][yy] * oMult;
                            int o0 = a.hardBin ? (int)(o + .5f) : (int)o;
                            const float od = a.hardBin ? 0.f : o - (float)o0;
                            if (o0 >= nO)
                            {
                                o0 = 0;
                            }
                            const float m = mn[xx][yy] * sInv2;
                            const float m1 = od * m;
                            const float m0 = m - m1;
                            hist_add2<MAXO>(H, o0, nO, m0, m1);
                        }
                    }
#pragma unroll
                    for (int bI = 0; bI < MAXO; bI++)
                    {
                        if (bI < nO)
                        {
                            cells[(c2 + bI) * wcells + cell] = H[bI];
                        }
                    }
                }
            }
        }
        __syncthreads();
        // ---- Detector::evaluate on the window's cells: [nC][mW][mH], so a feature id is the cell's index
        const float h = crop_cascade(cells, wcells, a.mH, a.mH, a.mW, a.fids, a.thrs, a.hs, a.child, a.nTrees, a.nTreeNodes, a.depth, a.cascThr, leaf, tid, nt);
        if (tid == 0)
        {
            a.scores[crop] = h;
        }
    }
}

// The staged form's first step: crop i's planes cut to hc x wc, tight, at out + i * out_fs ([d][wc][hc]).
__global__ void __launch_bounds__(256) k_crop_gather(const float* __restrict__ in, float* __restrict__ out, int h, int w, int d, int hc, int wc, int64_t out_fs)
{
    const int64_t per = int64_t(d) * wc * hc;
    const int64_t e = int64_t(blockIdx.x) * 256 + threadIdx.x;
    if (e >= per)
    {
        return;
    }
    const int z = int(e / (int64_t(wc) * hc));
    const int rem = int(e - int64_t(z) * wc * hc);
    const int x = rem / hc, y = rem - x * hc;
    out[int64_t(blockIdx.z) * out_fs + e] = in[int64_t(blockIdx.z) * d * h * w + (int64_t(z) * w + x) * h + y];
}

// ... from upright packed bytes: k_ingest_u8's arithmetic (float(v) * float(1 / 255.0)), the planes r, g, b (or the one gray plane)
__global__ void __launch_bounds__(256) k_crop_gather_u8(const uint8_t* __restrict__ in, float* __restrict__ out, int d, int hc, int wc, int cpp, int ro, int go,
    int bo, int rowStride, int64_t in_fs, int64_t out_fs)
{
    const int64_t e = int64_t(blockIdx.x) * 256 + threadIdx.x;
    if (e >= int64_t(wc) * hc)
    {
        return;
    }
    const int y = int(e / wc), x = int(e - int64_t(y) * wc);
    const uint8_t* px = in + int64_t(blockIdx.z) * in_fs + int64_t(y) * rowStride + x * cpp;
    float* o = out + int64_t(blockIdx.z) * out_fs + int64_t(x) * hc + y;
    const float sc = float(1.0 / 255.0);
    o[0] = float(px[ro]) * sc;
    if (d == 3)
    {
        o[int64_t(wc) * hc] = float(px[go]) * sc;
        o[2 * int64_t(wc) * hc] = float(px[bo]) * sc;
    }
}

// The staged form's last step: Detector::evaluate(const MatP&, ...) for a batch — k_evaluate_window per channel buffer, one wave per
// crop (blockIdx.x), the buffers chns_fs floats apart.
__global__ void __launch_bounds__(64) k_evaluate_windows(const float* __restrict__ chns, int64_t chns_fs, int hP, int wP, int mH, int mW,
    const uint32_t* __restrict__ fids, const float* __restrict__ thrs, const float* __restrict__ hs, const uint32_t* __restrict__ child, int nTrees,
    int nTreeNodes, int depth, float cascThr, float* __restrict__ scores)
{
    __shared__ float leaf[64 + 4];
    const float h = crop_cascade(chns + int64_t(blockIdx.x) * chns_fs, hP * wP, hP, mH, mW, fids, thrs, hs, child, nTrees, nTreeNodes, depth, cascThr, leaf,
        threadIdx.x, 64);
    if (threadIdx.x == 0)
    {
        scores[blockIdx.x] = h;
    }
}

} // namespace acfhip
