// kernels_cut.hip.h — crops of the stored frame (acf_hip_cut_crops / acf_hip_cut_detections; the header's "crops of the stored frame"
// section is the definition): one kernel, k_cut_crops, reads only the pixels under the boxes from the frame as the descriptor, the
// format and the orientation code describe it, and writes upright crops of one fixed size, in the order of the boxes.  No reference
// counterpart: the sampling rule is this library's own, every operation an f32 operation rounded once (the build has
// -ffp-contract=off), so that a numpy restatement gives the same bits (tests/cut_crops_ref.py).
//
// One workgroup of 256 per crop slot; lanes run along output columns.  Everything a workgroup decides (the box, the frame, the form,
// the bands) depends on blockIdx alone: uniform.  Two forms, chosen per crop by cut_form (= acf_hip_crop_form), same bits:
//   staged   the crop is walked in bands of output rows.  The coordinates are monotone in the sample index (cut_coord: every step of
//            it is monotone under round-to-nearest), so a band's samples read rows floor(v(first)) .. min(floor(v(last)) + 1, Hu - 1) of U
//            and the crop's columns floor(v(0)) .. min(floor(v(last)) + 1, Wu - 1): that clamped rectangle of U is the rectangle
//            orient_tile gives of the stored frame; it is loaded once, lanes along the STORED rows whatever the turn, through the
//            source's accessor (YUV converted once per stored pixel) into LDS as code values (u8, u16 or the f32 bits), one plane a
//            channel, and sampled from there.  A band takes as many output rows as fit the stage (greedy); a single output row whose
//            footprint does not fit (cut_form's bound excludes it; rounding on boxes far larger than the frame might not) is gathered.
//   gather   every sample fetches its four neighbours through the accessor: right for strong reductions, where a footprint holds far
//            more pixels than are sampled.
// The accessors are those of the resized entries (RzYuvSrcT<CF>: Y at (r, c), U and V at (r >> sub_y, c >> sub_x) in SOURCE
// coordinates, through yuv_chroma / yuv_rgb), the same shape over Yuv16Src's words for wide samples, and over an image's element
// strides for every dtype; OrientSrc is the turn.  Only pixels inside [0, Hs) x [0, Ws) are addressed: the coordinate is clamped
// before it becomes an index (and the index once more), so nothing in a box makes a load leave the description's extent.
//
// LDS: CUT_LDS_BYTES = 32 KiB of the CU's 160 KiB a workgroup: five workgroups (20 waves) a CU by LDS — the kernel waits on memory
// in both forms (the load phase, the gathers), so resident waves are what hides it, and 32 KiB already holds the whole footprint of a
// 112 x 112 crop of an RGB byte source at up to ~1.4 stored pixels a sample in one or two bands; more per workgroup would buy fewer
// bands (two barriers each) at the price of occupancy.  Layout [C][capRows][pitch] code values, pitch = the footprint's width made
// odd: the samplers of a wave read near-consecutive columns of one or two rows (conflict-free up to the 2 .. 4 lanes that share a
// dword of narrow codes); the loaders of a quarter turn write down a column, pitch elements apart — odd, so consecutive lanes fall
// on different banks for f32 codes and share a dword at most pairwise for narrow ones.  (Derived from the address maps with the
// bank rule; SQ_LDS_BANK_CONFLICT was not read.)
#pragma once

namespace acfhip
{

constexpr int CUT_LDS_BYTES = 32 * 1024;

__host__ __device__ inline bool cut_finite(float v)
{
    return __builtin_isfinite(v);
}
// a box the kernel samples; any other gives a crop of zeros
__host__ __device__ inline bool cut_box_ok(float bx, float by, float bw, float bh)
{
    return cut_finite(bx) && cut_finite(by) && cut_finite(bw) && cut_finite(bh) && bw > 0.f && bh > 0.f;
}
// The coordinate of sample m along an axis of n pixels, clamped into the frame (border replication).  For a finite origin and a finite
// step >= 0 no step of it yields NaN (an overflowing product is +inf, and stays so); each is monotone in m.
__host__ __device__ inline float cut_coord(float b0, float step, int m, int n)
{
    float v = (b0 + (float(m) + 0.5f) * step) - 0.5f;
    const float hi = float(n - 1);
    v = v > 0.f ? v : 0.f;
    return v < hi ? v : hi;
}
__host__ __device__ inline int cut_floor(float v, int n)
{
    const int i = int(floorf(v));
    return i < 0 ? 0 : (i > n - 1 ? n - 1 : i);
}
// acf_hip_crop_box: a detection of the reduced frame as a box in U
__host__ __device__ inline void cut_box(int x, int y, int w, int h, float inv, float grow, float (&o)[4])
{
    const float fx = float(x) * inv, fy = float(y) * inv, fw = float(w) * inv, fh = float(h) * inv;
    const float cx = fx + fw * 0.5f, cy = fy + fh * 0.5f;
    const float w2 = fw * grow, h2 = fh * grow;
    o[0] = cx - w2 * 0.5f;
    o[1] = cy - h2 * 0.5f;
    o[2] = w2;
    o[3] = h2;
}
__host__ __device__ inline int cut_pitch(int fw)
{
    return fw | 1;
}
// acf_hip_crop_form: 0 staged, 1 gather.  Gather when the crop's clamped footprint holds more than four pixels a sample (a sample
// fetches four: beyond that the stage would load more than the gathers do), or when the footprint of one output row — at most
// ceil(s * stepy) + 3 rows of the footprint's width — does not fit the stage.  (A bad box samples nothing: 1.)
__host__ __device__ inline int cut_form(int oh, int ow, int s, float bx, float by, float bw, float bh, int Hu, int Wu, int C, int sampleBytes)
{
    if (!cut_box_ok(bx, by, bw, bh))
    {
        return 1;
    }
    const float stepx = bw / float(ow * s), stepy = bh / float(oh * s);
    const int c0 = cut_floor(cut_coord(bx, stepx, 0, Wu), Wu), c1 = cut_floor(cut_coord(bx, stepx, ow * s - 1, Wu), Wu);
    const int r0 = cut_floor(cut_coord(by, stepy, 0, Hu), Hu), r1 = cut_floor(cut_coord(by, stepy, oh * s - 1, Hu), Hu);
    const int fw = (c1 + 1 < Wu ? c1 + 1 : Wu - 1) - c0 + 1, fh = (r1 + 1 < Hu ? r1 + 1 : Hu - 1) - r0 + 1;
    if (int64_t(fw) * fh > 4 * int64_t(ow * s) * (oh * s))
    {
        return 1;
    }
    const float span = ceilf(float(s) * stepy);
    int rows1 = span >= float(Hu) ? Hu : int(span) + 3;
    rows1 = rows1 < fh ? rows1 : fh;
    return int64_t(cut_pitch(fw)) * C * sampleBytes * rows1 > CUT_LDS_BYTES ? 1 : 0;
}

// What a launch reads besides the source: the crop list of acf_hip_cut_crops (boxes, frames), or the detection records and counts of
// the context's last batch (dets != null: acf_hip_cut_detections), the upright geometry, the spec and the destination
struct CutArgs
{
    const float* boxes;     // [n][4]
    const int32_t* frames;  // [n]
    const acf_hip_detection* dets; // [nFrames][maxHits]
    const int32_t* counts;         // [nFrames]; -1: over the device NMS's capacity
    int maxHits, K;
    float inv, grow;        // acf_hip_crop_box's
    float* boxesOut;        // [nFrames][K][4] or null
    int32_t* countsOut;     // [nFrames]
    int nFrames;
    OrientSrc o;
    int Hu, Wu, C;
    int oh, ow, s, dtype, layout;
    float unit;
    uint8_t* dst;
    int64_t cropBytes;
};
// the source as either family describes it (im: element strides; yuv: byte strides, yuv.yuv.k the format's constants)
struct CutSource
{
    ImageArgs im;
    Yuv16Src yuv;
};
enum
{
    CUT_IMG_U8 = 0, // = IM_*
    CUT_IMG_F16 = 1,
    CUT_IMG_BF16 = 2,
    CUT_IMG_F32 = 3,
    CUT_YUV8 = 4,    // the default format: cvtColor's constants inline
    CUT_YUV8_CF = 5, // another 8-bit format
    CUT_YUV16 = 6
};

// px(y, x, v) over an image's element strides: the raw elements of stored pixel (y, x), every dtype
template <int DT>
struct CutImageSrc
{
    using raw = typename ImgElem<DT>::raw;
    const raw* in; // frame n's element (0, 0, 0)
    int64_t sc, sy, sx;
    int nIn;
    __device__ __forceinline__ void px(int y, int x, raw (&v)[4]) const
    {
        const raw* p = in + int64_t(y) * sy + int64_t(x) * sx;
        v[0] = p[0];
        v[1] = nIn == 3 ? p[sc] : raw(0);
        v[2] = nIn == 3 ? p[2 * sc] : raw(0);
        v[3] = 0;
    }
};
// ... and over 16-bit words: RzYuvSrcT's shape with Yuv16Src's sample rule and the 64-bit sums
struct CutYuv16Src
{
    const uint8_t *py, *pu, *pv;
    int64_t ysr, ysp, usr, usp, vsr, vsp;
    int subX, subY, shift, mask;
    YuvCoef k;
    __device__ __forceinline__ int word(const uint8_t* p) const
    {
        return (int(*reinterpret_cast<const uint16_t*>(p)) >> shift) & mask;
    }
    __device__ __forceinline__ void px(int y, int x, int (&v)[4]) const
    {
        const int cr = y >> subY, cc = x >> subX;
        const int Y = word(py + int64_t(y) * ysr + int64_t(x) * ysp);
        const int U = word(pu + int64_t(cr) * usr + int64_t(cc) * usp);
        const int V = word(pv + int64_t(cr) * vsr + int64_t(cc) * vsp);
        yuv_rgb<true>(Y, yuv_chroma<true, int64_t>(U, V, k), k, v[0], v[1], v[2]);
        v[3] = 0;
    }
};

// A source kind: its accessor of frame n, the code value the stage holds, and that code as the exact float the definition samples
template <int KIND>
struct CutKind
{
    static constexpr int DT = KIND;
    using code_t = typename ImgElem<DT>::raw;
    using elem_t = code_t;
    static __device__ __forceinline__ CutImageSrc<DT> at(const CutSource& S, int64_t n)
    {
        return CutImageSrc<DT>{ static_cast<const code_t*>(S.im.in) + n * S.im.sn, S.im.sc, S.im.sy, S.im.sx, S.im.nIn };
    }
    static __device__ __forceinline__ float val(code_t v)
    {
        if constexpr (DT == IM_U8)
        {
            return float(v);
        }
        else
        {
            return ImgElem<DT>::cvt(v);
        }
    }
};
template <bool CF>
struct CutKindYuv8
{
    using code_t = uint8_t;
    using elem_t = int;
    static __device__ __forceinline__ RzYuvSrcT<CF> at(const CutSource& S, int64_t n)
    {
        const YuvDescSrc& d = S.yuv.yuv;
        return RzYuvSrcT<CF>{ d.base + d.y.off + n * d.y.sn, d.base + d.u.off + n * d.u.sn, d.base + d.v.off + n * d.v.sn, d.y.sr, d.y.sp, d.u.sr, d.u.sp, d.v.sr,
            d.v.sp, d.subX, d.subY, d.k };
    }
    static __device__ __forceinline__ float val(code_t v)
    {
        return float(v);
    }
};
template <>
struct CutKind<CUT_YUV8> : CutKindYuv8<false>
{
};
template <>
struct CutKind<CUT_YUV8_CF> : CutKindYuv8<true>
{
};
template <>
struct CutKind<CUT_YUV16>
{
    using code_t = uint16_t;
    using elem_t = int;
    static __device__ __forceinline__ CutYuv16Src at(const CutSource& S, int64_t n)
    {
        const YuvDescSrc& d = S.yuv.yuv;
        return CutYuv16Src{ d.base + d.y.off + n * d.y.sn, d.base + d.u.off + n * d.u.sn, d.base + d.v.off + n * d.v.sn, d.y.sr, d.y.sp, d.u.sr, d.u.sp, d.v.sr,
            d.v.sp, d.subX, d.subY, S.yuv.shift, S.yuv.mask, d.k };
    }
    static __device__ __forceinline__ float val(code_t v)
    {
        return float(v);
    }
};

// upright pixel (r, c) -> stored pixel (rs, cs): the header's orientation mapping, as orient_tile states it for a rectangle
__device__ __forceinline__ void cut_to_source(const OrientSrc& o, int r, int c, int& rs, int& cs)
{
    const int p = o.swap ? c : r, q = o.swap ? r : c;
    rs = o.revR ? o.Hs - 1 - p : p;
    cs = o.revC ? o.Ws - 1 - q : q;
}

// One crop's sampling grid
struct CutGrid
{
    float bx, by, stepx, stepy;
    int Hu, Wu, s;
    float norm; // float(1.0 / (s * s))
};

// One output pixel (i, j), every channel: the ONE statement of the sampling rule, for both forms.  fetch(r, c, p) yields the C exact
// floats of upright pixel (r, c).
template <class FETCH>
__device__ __forceinline__ void cut_pixel(const CutGrid& g, int i, int j, FETCH&& fetch, float (&val)[3])
{
    float acc[3] = { 0.f, 0.f, 0.f };
    for (int a = 0; a < g.s; a++)
    {
        const float vy = cut_coord(g.by, g.stepy, i * g.s + a, g.Hu);
        const int r0 = cut_floor(vy, g.Hu), r1 = min(r0 + 1, g.Hu - 1);
        const float fy = vy - float(r0);
        for (int b = 0; b < g.s; b++)
        {
            const float vx = cut_coord(g.bx, g.stepx, j * g.s + b, g.Wu);
            const int c0 = cut_floor(vx, g.Wu), c1 = min(c0 + 1, g.Wu - 1);
            const float fx = vx - float(c0);
            float p00[3], p01[3], p10[3], p11[3];
            fetch(r0, c0, p00);
            fetch(r0, c1, p01);
            fetch(r1, c0, p10);
            fetch(r1, c1, p11);
#pragma unroll
            for (int c = 0; c < 3; c++)
            {
                const float top = p00[c] + fx * (p01[c] - p00[c]);
                const float bot = p10[c] + fx * (p11[c] - p10[c]);
                acc[c] = acc[c] + (top + fy * (bot - top));
            }
        }
    }
#pragma unroll
    for (int c = 0; c < 3; c++)
    {
        val[c] = acc[c] * g.norm;
    }
}

// float32 -> bfloat16, round to nearest even (NaN: the quiet NaN)
__device__ __forceinline__ uint16_t cut_bf16(float v)
{
    const uint32_t u = __float_as_uint(v);
    if (v != v)
    {
        return uint16_t(0x7fc0);
    }
    return uint16_t((u + 0x7fffu + ((u >> 16) & 1u)) >> 16);
}

// float32 -> float16, round to nearest even, in integer steps (subnormal halves through one f32 add: beside 0.5f a float's ulp is
// 2^-24, the subnormal halves' own).  Not `_Float16(v)`: with the product val * unit in front of it the compiler selects
// v_fma_mixlo_f16, which rounds the exact product ONCE to f16, where the definition narrows the f32 product (two roundings; they differ
// on about one value in 10^4)
__device__ __forceinline__ uint16_t cut_f16(float v)
{
    const uint32_t u = __float_as_uint(v), sign = (u >> 16) & 0x8000u, a = u & 0x7fffffffu;
    if (a > 0x7f800000u)
    {
        return uint16_t(sign | 0x7e00u);
    }
    if (a >= 0x47800000u) // 65536 and beyond (what rounds up to it from below carries into the exponent by itself)
    {
        return uint16_t(sign | 0x7c00u);
    }
    if (a < 0x38800000u) // below 2^-14
    {
        return uint16_t(sign | (__float_as_uint(__uint_as_float(a) + 0.5f) - 0x3f000000u));
    }
    return uint16_t(sign | ((a + 0xfffu + ((a >> 13) & 1u) - 0x38000000u) >> 13));
}

// output pixel (i, j) of a crop in the spec's dtype and layout
__device__ __forceinline__ void cut_store(const CutArgs& a, uint8_t* crop, int i, int j, const float (&val)[3])
{
#pragma unroll
    for (int c = 0; c < 3; c++)
    {
        if (c < a.C)
        {
            const int64_t at = a.layout ? (int64_t(i) * a.ow + j) * a.C + c : (int64_t(c) * a.oh + i) * a.ow + j;
            switch (a.dtype)
            {
                case IM_U8: crop[at] = uint8_t(fminf(fmaxf(rintf(val[c]), 0.f), 255.f)); break;
                case IM_F16: reinterpret_cast<uint16_t*>(crop)[at] = cut_f16(val[c] * a.unit); break;
                case IM_BF16: reinterpret_cast<uint16_t*>(crop)[at] = cut_bf16(val[c] * a.unit); break;
                default: reinterpret_cast<float*>(crop)[at] = val[c] * a.unit;
            }
        }
    }
}

// rows [i0, i1) of a crop, lanes along output columns
template <class FETCH>
__device__ __forceinline__ void cut_rows(const CutArgs& a, const CutGrid& g, uint8_t* crop, int i0, int i1, FETCH&& fetch)
{
    for (int e = threadIdx.x; e < (i1 - i0) * a.ow; e += 256)
    {
        const int i = i0 + e / a.ow, j = e % a.ow;
        float val[3];
        cut_pixel(g, i, j, fetch, val);
        cut_store(a, crop, i, j, val);
    }
}

template <int KIND>
__global__ void __launch_bounds__(256) k_cut_crops(CutArgs a, CutSource S)
{
    using K = CutKind<KIND>;
    using code_t = typename K::code_t;
    __shared__ uint32_t stageW[CUT_LDS_BYTES / 4];
    code_t* stage = reinterpret_cast<code_t*>(stageW);
    const int slot = blockIdx.x;
    float box[4];
    int f;
    if (a.dets)
    {
        f = slot / a.K;
        const int i = slot - f * a.K;
        const int nf = a.counts[f];
        const int cnt = nf < 0 ? -1 : min(min(nf, a.K), a.maxHits);
        if (i == 0 && threadIdx.x == 0)
        {
            a.countsOut[f] = cnt;
        }
        if (i >= cnt)
        {
            return;
        }
        const acf_hip_detection d = a.dets[size_t(f) * a.maxHits + i];
        cut_box(d.x, d.y, d.w, d.h, a.inv, a.grow, box);
        if (a.boxesOut && threadIdx.x < 4)
        {
            a.boxesOut[int64_t(slot) * 4 + threadIdx.x] = box[threadIdx.x];
        }
    }
    else
    {
#pragma unroll
        for (int k = 0; k < 4; k++)
        {
            box[k] = a.boxes[int64_t(slot) * 4 + k];
        }
        f = a.frames[slot];
    }
    uint8_t* crop = a.dst + int64_t(slot) * a.cropBytes;
    if (!cut_box_ok(box[0], box[1], box[2], box[3]) || f < 0 || f >= a.nFrames)
    {
        if (((reinterpret_cast<uintptr_t>(crop) | uintptr_t(a.cropBytes)) & 3) == 0)
        {
            for (int64_t b = threadIdx.x; b < a.cropBytes / 4; b += 256)
            {
                reinterpret_cast<uint32_t*>(crop)[b] = 0u;
            }
        }
        else
        {
            for (int64_t b = threadIdx.x; b < a.cropBytes; b += 256)
            {
                crop[b] = 0;
            }
        }
        return;
    }
    CutGrid g;
    g.bx = box[0];
    g.by = box[1];
    g.stepx = box[2] / float(a.ow * a.s);
    g.stepy = box[3] / float(a.oh * a.s);
    g.Hu = a.Hu;
    g.Wu = a.Wu;
    g.s = a.s;
    g.norm = float(1.0 / double(a.s * a.s));
    const auto src = K::at(S, f);
    const OrientSrc o = a.o;
    const auto gather = [&](int r, int c, float(&p)[3]) {
        int rs, cs;
        cut_to_source(o, r, c, rs, cs);
        typename K::elem_t v[4];
        src.px(rs, cs, v);
#pragma unroll
        for (int k = 0; k < 3; k++)
        {
            p[k] = K::val(code_t(v[k]));
        }
    };
    if (cut_form(a.oh, a.ow, a.s, box[0], box[1], box[2], box[3], a.Hu, a.Wu, a.C, int(sizeof(code_t))))
    {
        cut_rows(a, g, crop, 0, a.oh, gather);
        return;
    }
    const int cLo = cut_floor(cut_coord(g.bx, g.stepx, 0, a.Wu), a.Wu);
    const int cHi = min(cut_floor(cut_coord(g.bx, g.stepx, a.ow * a.s - 1, a.Wu), a.Wu) + 1, a.Wu - 1);
    const int fw = cHi - cLo + 1, pitch = cut_pitch(fw);
    const int capRows = CUT_LDS_BYTES / (pitch * a.C * int(sizeof(code_t)));
    const int plane = capRows * pitch;
    const auto lastRow = [&](int i1) { return min(cut_floor(cut_coord(g.by, g.stepy, i1 * a.s - 1, a.Hu), a.Hu) + 1, a.Hu - 1); };
    int i0 = 0;
    while (i0 < a.oh)
    {
        const int rLo = cut_floor(cut_coord(g.by, g.stepy, i0 * a.s, a.Hu), a.Hu);
        int i1 = i0 + 1, rHi = lastRow(i1);
        if (rHi - rLo + 1 > capRows)
        {
            cut_rows(a, g, crop, i0, i1, gather);
            i0 = i1;
            continue;
        }
        while (i1 < a.oh)
        {
            const int r = lastRow(i1 + 1);
            if (r - rLo + 1 > capRows)
            {
                break;
            }
            rHi = r;
            i1++;
        }
        const OrientTile T = orient_tile(o, cLo, rLo, fw, rHi - rLo + 1);
        __syncthreads(); // (the band before has been sampled)
        for (int e = threadIdx.x; e < T.nsr * T.nsc; e += 256)
        {
            const int i = e / T.nsc, j = e - i * T.nsc;
            typename K::elem_t v[4];
            src.px(T.rs0 + i, T.cs0 + j, v);
            int yy, xx;
            T.up(i, j, yy, xx);
            code_t* at = stage + yy * pitch + xx;
#pragma unroll
            for (int k = 0; k < 3; k++)
            {
                if (k < a.C)
                {
                    at[k * plane] = code_t(v[k]);
                }
            }
        }
        __syncthreads();
        cut_rows(a, g, crop, i0, i1, [&](int r, int c, float(&p)[3]) {
            const code_t* at = stage + (r - rLo) * pitch + (c - cLo);
#pragma unroll
            for (int k = 0; k < 3; k++)
            {
                p[k] = k < a.C ? K::val(at[k * plane]) : 0.f;
            }
        });
        i0 = i1;
    }
}

} // namespace acfhip
