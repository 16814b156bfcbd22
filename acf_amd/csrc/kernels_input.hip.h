// kernels_input.hip.h — part of kernels.hip.h (included from there, in its order, and nowhere else: the parts share kernels.hip.h's
// includes, its layout / arithmetic contract and the helpers of the parts before them).
// rgbConvert (LUV / gray / HSV), the packed 8-bit ingest, the tensor and YUV ingests (upright: k_ingest_image / k_ingest_yuv; rotated and mirrored
// frames: k_ingest_image_oriented / k_ingest_yuv_oriented), the apps' resize to a minimum object width (alone: k_resize_u8; inside the tensor / YUV
// entries: k_ingest_resized; on rotated and mirrored frames: k_ingest_oriented_resized), and the plain convTri1 (k_smooth_tri1: the fallback of the vector smoothing).
#pragma once

namespace acfhip
{

// ------------------------------------------------------------------------
// rgbConvert (toolbox/rgbConvertMex.cpp)
// ------------------------------------------------------------------------
struct LuvConsts
{
    float mr[3], mg[3], mb[3];
    float minu, minv, un, vn, cun, cvn;
};

// rgb2luv_sse body (:129-187) when VEC, else the scalar rgb2luv (:69-83); the
// reference picks VEC iff n % 4 == 0.  lTable: 1064 floats built on the host
// exactly as rgb2luv_setup does (:39-58).
// x86: the table of the CPU whose _mm_rcp_ps the SSE body's one reciprocal (:161) reproduces (option "arith"), or null: 1 / x.
template <bool VEC>
__device__ __forceinline__ void luv_px(float r, float g, float b, const float* __restrict__ lTable, const LuvConsts& k, float& L, float& U, float& V,
    const uint32_t* __restrict__ x86 = nullptr)
{
    if (VEC)
    {
        const float x = (r * k.mr[0] + g * k.mg[0]) + b * k.mb[0];
        const float y = (r * k.mr[1] + g * k.mg[1]) + b * k.mb[1];
        const float z = (r * k.mr[2] + g * k.mg[2]) + b * k.mb[2];
        const float den = x + (1e-35f + (15.0f * y + 3.0f * z));
        const float zz = x86 ? x86_rcp(den, x86) : 1.0f / den;
        const float lf = 1024.0f * y;
        const float u = (52.0f * x) * zz - k.cun;
        const float v = (117.0f * y) * zz - k.cvn;
        L = lTable[(int)lf];
        U = L * u - k.minu;
        V = L * v - k.minv;
    }
    else
    {
        const float x = k.mr[0] * r + k.mg[0] * g + k.mb[0] * b;
        const float y = k.mr[1] * r + k.mg[1] * g + k.mb[1] * b;
        float z = k.mr[2] * r + k.mg[2] * g + k.mb[2] * b;
        L = lTable[(int)(y * 1024)];
        z = 1 / (x + 15 * y + 3 * z + (float)1e-35);
        U = L * (13 * 4 * x * z - 13 * k.un) - k.minu;
        V = L * (13 * 9 * y * z - 13 * k.vn) - k.minv;
    }
}

template <bool VEC>
__global__ void __launch_bounds__(256) k_rgb2luv(const float* __restrict__ in, float* __restrict__ out,
    const float* __restrict__ lTable, LuvConsts k, int n, int64_t in_fs, int64_t out_fs, const uint32_t* __restrict__ x86)
{
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n)
    {
        return;
    }
    const float* I = in + int64_t(blockIdx.z) * in_fs;
    float* J = out + int64_t(blockIdx.z) * out_fs;
    const float r = I[i], g = I[i + n], b = I[i + 2 * int64_t(n)];
    float L, U, V;
    luv_px<VEC>(r, g, b, lTable, k, L, U, V, x86);
    J[i] = L;
    J[i + n] = U;
    J[i + 2 * int64_t(n)] = V;
}

// rgb2gray (:241-252); REPL: the 1-plane input was replicated to 3 planes first
// (chnsPyramid.cpp:234-244), i.e. r == g == b.
template <bool REPL>
__global__ void __launch_bounds__(256) k_rgb2gray(const float* __restrict__ in, float* __restrict__ out, int n,
    int64_t in_fs, int64_t out_fs, float mr, float mg, float mb)
{
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n)
    {
        return;
    }
    const float* I = in + int64_t(blockIdx.z) * in_fs;
    const float r = I[i];
    const float g = REPL ? r : I[i + n];
    const float b = REPL ? r : I[i + 2 * int64_t(n)];
    out[int64_t(blockIdx.z) * out_fs + i] = r * mr + g * mg + b * mb;
}

// Replicate one plane to three (chnsPyramid.cpp:242-243), colorSpace "orig".
// rgb2hsv (toolbox/rgbConvertMex.cpp:194-238), nrm = 1: one pixel.  IEEE divisions; h * float(1 / 6.0).
__device__ __forceinline__ void hsv_px(float r, float g, float b, float& h, float& s, float& v)
{
    if (r == g && g == b)
    {
        h = 0.f;
        s = 0.f;
        v = r * 1.0f;
    }
    else
    {
        float maxv, minv;
        if (r >= g && r >= b)
        {
            maxv = r;
            minv = g < b ? g : b;
            h = (g - b) / (maxv - minv) + 6;
            if (h >= 6)
            {
                h -= 6;
            }
        }
        else if (g >= r && g >= b)
        {
            maxv = g;
            minv = r < b ? r : b;
            h = (b - r) / (maxv - minv) + 2;
        }
        else
        {
            maxv = b;
            minv = r < g ? r : g;
            h = (r - g) / (maxv - minv) + 4;
        }
        h *= (float)(1 / 6.0);
        s = 1 - minv / maxv;
        v = maxv * 1.0f;
    }
}

// three planes in, H, S, V out
__global__ void __launch_bounds__(256) k_rgb2hsv(const float* __restrict__ in, float* __restrict__ out, int n, int64_t in_fs, int64_t out_fs)
{
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= n)
    {
        return;
    }
    const float* I = in + int64_t(blockIdx.z) * in_fs;
    float* J = out + int64_t(blockIdx.z) * out_fs;
    const float r = I[i], g = I[n + i], b = I[2 * int64_t(n) + i];
    float h, s, v;
    hsv_px(r, g, b, h, s, v);
    J[i] = h;
    J[n + i] = s;
    J[2 * int64_t(n) + i] = v;
}

__global__ void __launch_bounds__(256) k_replicate3(const float* __restrict__ in, float* __restrict__ out, int n, int64_t in_fs, int64_t out_fs)
{
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n)
    {
        return;
    }
    const float v = in[int64_t(blockIdx.z) * in_fs + i];
    float* J = out + int64_t(blockIdx.z) * out_fs;
    J[i] = v;
    J[i + n] = v;
    J[i + 2 * int64_t(n)] = v;
}

// uint8_t channel planes -> f32 (exact), for the uint8_t cascade body (acfDetect1.cpp:157-166)
__global__ void __launch_bounds__(256) k_widen_u8(const uint8_t* __restrict__ in, float* __restrict__ out, int64_t n)
{
    const int64_t i = int64_t(blockIdx.x) * blockDim.x + threadIdx.x;
    if (i < n)
    {
        out[i] = float(in[i]);
    }
}

// ------------------------------------------------------------------------
// Packed 8-bit upright frames -> transposed planar f32.
//
// Restates the image entry of the detector: cvt8UC3To32FC3 = convertTo(CV_32FC3, 1/255) (ACF.cpp:114-119; OpenCV's
// 8u->32f cvtScale works in f32: float(v) * float(1/255.0)), I.t() (ACF.cpp:137,149) and the MatP plane split
// (MatP.cpp:51-73).  The colour conversion of chnsPyramid.cpp:230-263 is applied in registers when MODE asks for it,
// so the planar f32 RGB image never goes to HBM.
//
// A workgroup moves one 64 x 64 pixel tile: rows are read as dwords (coalesced along image-x) into LDS, then every
// lane takes 4 consecutive image-y of one image-x and writes one float4 per output plane (coalesced along image-y).
// The LDS row pitch is 65 dwords, so the 16 row-quads of a wave hit 16 distinct banks.
// ------------------------------------------------------------------------
enum
{
    IG_PLANAR = 0, // nOut planes, plane c = component c (after the ro/go/bo swizzle)
    IG_LUV_VEC = 1, // rgb2luv_sse body
    IG_LUV = 2,     // scalar rgb2luv
    IG_GRAY = 3     // rgb2gray
};

struct IngestArgs
{
    const uint8_t* in;
    float* out;
    const float* lTable;
    LuvConsts k;
    float mr, mg, mb;
    int H, W;        // upright rows, columns
    int cpp;         // bytes per pixel (1, 3, 4)
    int ro, go, bo;  // byte offsets of r, g, b inside a pixel
    int rowStride;   // bytes between image rows
    int64_t in_fs;   // bytes between frames
    int64_t out_fs;  // floats between output frames
    int nOut;        // IG_PLANAR: 1 or 3 planes
    int vecStore;    // H % 4 == 0: float4 stores
    const uint32_t* x86; // option "arith": the CPU tables for rgb2luv_sse's reciprocal (null: exact)
};

constexpr int IG_T = 64;
constexpr int IG_PITCH = 260; // bytes; 65 dwords

// One pixel of a lane's four (r, g, b already * 1/255) through the model's colour conversion, into column j of the planes' quads.
template <int MODE>
__device__ __forceinline__ void ingest_convert(const IngestArgs& a, float r, float g, float b, float (&o)[3][4], int j)
{
    if (MODE == IG_PLANAR)
    {
        o[0][j] = r;
        o[1][j] = g;
        o[2][j] = b;
    }
    else if (MODE == IG_GRAY)
    {
        o[0][j] = r * a.mr + g * a.mg + b * a.mb; // rgbConvertMex.cpp:241-252
    }
    else
    {
        luv_px<MODE == IG_LUV_VEC>(r, g, b, a.lTable, a.k, o[0][j], o[1][j], o[2][j], a.x86);
    }
}

// A lane's four consecutive image-y of every output plane: one float4 a plane, or the `left` (< 4) rows the tile still has.
template <int MODE>
__device__ __forceinline__ void ingest_store(const IngestArgs& a, const float (&o)[3][4], float* at, int64_t np, int left)
{
    const int nPl = (MODE == IG_PLANAR) ? a.nOut : (MODE == IG_GRAY ? 1 : 3);
#pragma unroll
    for (int c = 0; c < 3; c++)
    {
        if (c < nPl)
        {
            float* d = at + c * np;
            if (a.vecStore && left > 3)
            {
                *reinterpret_cast<float4*>(d) = make_float4(o[c][0], o[c][1], o[c][2], o[c][3]);
            }
            else
            {
#pragma unroll
                for (int j = 0; j < 4; j++)
                {
                    if (j < left)
                    {
                        d[j] = o[c][j];
                    }
                }
            }
        }
    }
}

// The store phase every ingest kernel ends in, behind the barrier that closes its load phase: of the workgroup's 64 x 64 tile (nx x ny
// at the frame's edges) a lane takes four consecutive image-y, yq .. yq + 3, of one image-x, xx, through the model's colour conversion
// and writes one float4 a plane (coalesced along image-y).  px(xx, yq, j, r, g, b) yields the already-scaled f32 r, g, b of tile pixel
// (yq + j, xx); it is called with j = 0 .. 3 in turn for one xx, so a kernel's functor may carry state from one j to the next (the
// chroma sample of a subsampled row pair).  Rows >= ny of the last quad are converted like the others and never stored, so px must
// yield something the conversion takes there too (rgb2luv indexes a table): bytes and clamped integers are in range whatever the LDS
// holds; a float tile yields zeros.
template <int MODE, class PX>
__device__ __forceinline__ void ingest_store_phase(const IngestArgs& a, int x0, int y0, int nx, int ny, PX&& px)
{
    const int yq = (threadIdx.x & 15) * 4;
    float* outF = a.out + int64_t(blockIdx.z) * a.out_fs;
    const int64_t np = int64_t(a.H) * a.W;
    for (int xx = threadIdx.x >> 4; xx < nx; xx += 16)
    {
        float o[3][4];
#pragma unroll
        for (int j = 0; j < 4; j++)
        {
            float r, g, b;
            px(xx, yq, j, r, g, b);
            ingest_convert<MODE>(a, r, g, b, o, j);
        }
        ingest_store<MODE>(a, o, outF + int64_t(x0 + xx) * a.H + y0 + yq, np, ny - yq);
    }
}

// The store phase on a 64 x 64 tile of packed bytes in LDS (pitch IG_PITCH; r, g, b at ro, go, bo of a pixel's cpp bytes): k_ingest_u8's,
// and the resized kernels' behind their resize.
template <int MODE>
__device__ __forceinline__ void ingest_store_tile(const IngestArgs& a, const uint8_t* tile, int cpp, int ro, int go, int bo, int x0, int y0, int nx, int ny)
{
    ingest_store_phase<MODE>(a, x0, y0, nx, ny, [&](int xx, int yq, int j, float& r, float& g, float& b) {
        const float sc = float(1.0 / 255.0);
        const uint8_t* p = tile + min(yq + j, IG_T - 1) * IG_PITCH + xx * cpp;
        r = float(p[ro]) * sc;
        g = float(p[go]) * sc;
        b = float(p[bo]) * sc;
    });
}

template <int MODE, bool ALIGNED>
__global__ void __launch_bounds__(256) k_ingest_u8(IngestArgs a)
{
    __shared__ uint32_t tileW[IG_T * IG_PITCH / 4];
    uint8_t* tile = reinterpret_cast<uint8_t*>(tileW);
    const int x0 = blockIdx.x * IG_T, y0 = blockIdx.y * IG_T;
    const int nx = min(IG_T, a.W - x0), ny = min(IG_T, a.H - y0);
    const uint8_t* src = a.in + int64_t(blockIdx.z) * a.in_fs + int64_t(y0) * a.rowStride + int64_t(x0) * a.cpp;
    const int nb = nx * a.cpp;
    if (ALIGNED)
    {
        // base, row stride and frame stride are multiples of 4 (host-checked) and x0 * cpp is a multiple of 64
        const int nd = (nb + 3) >> 2; // the last dword of a row may run into the next row: still inside the frame
        const int lastOk = (y0 + ny == a.H && blockIdx.z == gridDim.z - 1) ? (nb >> 2) : nd; // ... except at the very end
        for (int i = threadIdx.x; i < ny * 64; i += 256)
        {
            const int yy = i >> 6, j = i & 63;
            if (j < nd)
            {
                const uint8_t* rp = src + int64_t(yy) * a.rowStride;
                uint32_t v;
                if (j < lastOk || yy + 1 < ny)
                {
                    v = reinterpret_cast<const uint32_t*>(rp)[j];
                }
                else
                {
                    v = 0;
                    for (int b = 0; b < nb - 4 * j; b++)
                    {
                        v |= uint32_t(rp[4 * j + b]) << (8 * b);
                    }
                }
                tileW[yy * (IG_PITCH / 4) + j] = v;
            }
        }
    }
    else
    {
        for (int i = threadIdx.x; i < ny * 256; i += 256)
        {
            const int yy = i >> 8, j = i & 255;
            if (j < nb)
            {
                tile[yy * IG_PITCH + j] = src[int64_t(yy) * a.rowStride + j];
            }
        }
    }
    __syncthreads();
    ingest_store_tile<MODE>(a, tile, a.cpp, a.ro, a.go, a.bo, x0, y0, nx, ny);
}

// ------------------------------------------------------------------------
// Upright images of any element strides (u8 / f16 / bf16 / f32) -> transposed planar f32: the image entry for CV_32FC3 as well as
// CV_8UC3 (ACF.cpp:135-141: I.t(), then the MatP split, MatP.cpp:51-73) on what a tensor library holds — element (n, c, y, x) at
// in[n * sn + c * sc + y * sy + x * sx].  k_ingest_u8's shape: a workgroup owns 64 x 64 pixels; the load phase runs lanes along
// image-x, widens every element to f32 as it arrives (u8: float(v) * float(1 / 255.0) as k_ingest_u8; f16 / bf16: exact) and
// stores it to an LDS tile of floats; the store phase is k_ingest_u8's (four consecutive image-y of one image-x a lane, the
// model's colour conversion in registers, one float4 a plane).
//
// Load forms (ImageArgs::form, chosen on the host from the strides and the pointer; all give the same planes):
//   IM_GENERIC  one element a lane, any strides: the baseline
//   IM_ROWVEC   sx == 1, every row start a multiple of four elements: four elements a lane in one load (4 / 8 / 16 bytes); the
//               nx % 4 elements at a row's end one by one
//   IM_PACKED   sc == +-1, sx == 3 or 4 (interleaved pixels, alpha skipped, channels forwards or backwards): the row's addressed
//               span [first element of pixel x0, last element of pixel x0 + nx - 1] is read as aligned dwords by consecutive
//               lanes (4 / 2 / 1 elements) and every element goes to its plane; the dwords that straddle the span's ends one
//               element at a time
// No load covers an address outside [first, last] element the same row of the same plane set addresses, so a view that ends
// with its allocation is safe.
//
// LDS: plane c at c * IM_PLANE floats, image row r in slot (r & 3) * 16 + (r >> 2) at a pitch of 66 dwords (the regrouping of
// k_ingest_yuv420).  Bank = dword address % 32, counted per 32-lane half (ds_read_b32 / ds_write_b32):
//   store phase (reads)  a half is 16 row-quads x 2 adjacent image-x; read j takes rows 4k + j = slots 16j + k, k = 0 .. 15:
//                        addresses 66k + {0, 1} -> banks 2k + {0, 1}: 32 distinct banks, conflict-free, for each plane's read
//   IM_GENERIC (writes)  a half writes 32 consecutive image-x of one row and plane: 32 distinct banks, conflict-free
//   IM_ROWVEC (writes)   a lane holds 4 consecutive dwords, a half two rows 16 slots = 1056 = 0 (mod 32) dwords apart: one
//                        ds_write_b32 of element i puts lanes at 4q + i, q = 0 .. 15, twice: 8 banks, 4-way (as b32; the
//                        slot pitch is 8-byte aligned, so the compiler may pair them into ds_write_b64)
//   IM_PACKED (writes)   a wave takes one row, its lanes the row's dwords: 32 consecutive elements of a row are ~11 pixels in all
//                        three planes; the planes are 64 * 66 + 11 dwords apart, so channel c of pixel x lands on bank
//                        x + 11c + const.  Enumerated over every lane group and row alignment: f32 (one element a lane)
//                        conflict-free; f16 / bf16 (element t of consecutive lanes' dwords: every 2nd element) 2-way; u8 (every
//                        4th) 4-way at stride_x 3, conflict-free at 4
// (degrees computed from the address maps above with the bank rule; the SQ_LDS_BANK_CONFLICT counter was not read:
// profiles/image_entry.md)
// 3 x (64 x 66 + 11) floats = 50820 bytes: three workgroups a CU.
// ------------------------------------------------------------------------
enum
{
    IM_U8 = 0, // = ACF_HIP_T_*
    IM_F16 = 1,
    IM_BF16 = 2,
    IM_F32 = 3
};
enum
{
    IM_GENERIC = 0,
    IM_ROWVEC = 1,
    IM_PACKED = 2
};

struct ImageArgs
{
    const void* in;
    int64_t sn, sc, sy, sx; // strides in elements: frames, channels, image rows, image columns
    int nIn;                // planes read: 1 (r = g = b = the plane) or 3
    int form;               // IM_GENERIC / IM_ROWVEC / IM_PACKED
};

template <int DT>
struct ImgElem;
template <>
struct ImgElem<IM_U8>
{
    using raw = uint8_t;
    static __device__ __forceinline__ float cvt(raw v)
    {
        return float(v) * float(1.0 / 255.0);
    }
};
template <>
struct ImgElem<IM_F16>
{
    using raw = uint16_t;
    static __device__ __forceinline__ float cvt(raw v)
    {
        return float(__builtin_bit_cast(_Float16, v));
    }
};
template <>
struct ImgElem<IM_BF16>
{
    using raw = uint16_t;
    static __device__ __forceinline__ float cvt(raw v)
    {
        return __uint_as_float(uint32_t(v) << 16);
    }
};
template <>
struct ImgElem<IM_F32>
{
    using raw = uint32_t;
    static __device__ __forceinline__ float cvt(raw v)
    {
        return __uint_as_float(v);
    }
};

constexpr int IM_PITCH = 66;                     // dwords
constexpr int IM_PLANE = IG_T * IM_PITCH + 11;   // dwords
__device__ __forceinline__ int im_slot(int r)
{
    return (r & 3) * 16 + (r >> 2);
}

// IM_PACKED: `rows` rows (sy elements apart) of npx interleaved pixels of sx (3 or 4) elements, r, g, b at 0, 1, 2 of a pixel (rev:
// at 2, 1, 0), the first row's first addressed element at `span`.  A row's addressed span [0, L) is read as the aligned dwords that
// hold a piece of it — a wave takes a row, its lanes the row's dwords in turn (four rows a pass; two passes' loads in flight); a dword
// over one end of the span element by element — and every element goes to place(plane, row, pixel, raw element).
template <int DT, class PLACE>
__device__ __forceinline__ void im_load_packed(const typename ImgElem<DT>::raw* span, int64_t sy, int npx, int sx, int rev, int rows, PLACE&& place)
{
    using raw = typename ImgElem<DT>::raw;
    constexpr int PER = 4 / int(sizeof(raw));          // elements a dword
    const int L = (npx - 1) * sx + 3;                  // elements a row addresses
    const int ndMax = (L * int(sizeof(raw)) + 6) >> 2; // dwords that can hold a piece of it, whatever the row's alignment
#pragma unroll 2
    for (int i = threadIdx.x >> 6; i < rows; i += 4)
    {
        const raw* rp = span + int64_t(i) * sy;
        const int mis = int(reinterpret_cast<uintptr_t>(rp) & 3) / int(sizeof(raw)); // elements of rp's dword in front of rp
        for (int d = threadIdx.x & 63; d < ndMax; d += 64)
        {
            const int e0 = d * PER - mis; // span index of dword d's first element
            if (e0 >= L)
            {
                continue;
            }
            raw v[PER];
            if (e0 >= 0 && e0 + PER <= L)
            {
                const uint32_t w = *reinterpret_cast<const uint32_t*>(rp + e0);
#pragma unroll
                for (int t = 0; t < PER; t++)
                {
                    v[t] = raw(w >> (8 * int(sizeof(raw)) * t));
                }
            }
            else
            {
#pragma unroll
                for (int t = 0; t < PER; t++) // a dword over one end of the span: only the elements inside it
                {
                    const int e = e0 + t;
                    v[t] = (e >= 0 && e < L) ? rp[e] : raw(0);
                }
            }
#pragma unroll
            for (int t = 0; t < PER; t++)
            {
                const int e = e0 + t;
                if (e >= 0 && e < L)
                {
                    const int x = sx == 4 ? e >> 2 : e / 3, m = e - x * sx;
                    if (m < 3) // (m == 3: the skipped fourth element)
                    {
                        place(rev ? 2 - m : m, i, x, v[t]);
                    }
                }
            }
        }
    }
}

// The store phase on the float tile (both image kernels; the reads' banks are derived above)
template <int MODE>
__device__ __forceinline__ void im_store_phase(const IngestArgs& a, const float* tile, int nIn, int x0, int y0, int nx, int ny)
{
    const int p1 = nIn == 3 ? IM_PLANE : 0, p2 = 2 * p1; // one plane: r = g = b (chnsPyramid.cpp:234-244)
    ingest_store_phase<MODE>(a, x0, y0, nx, ny, [&](int xx, int yq, int j, float& r, float& g, float& b) {
        const float* t = tile + im_slot(yq + j) * IM_PITCH + xx;
        const bool in = yq + j < ny; // (the LDS of rows beyond the tile was never written)
        r = in ? t[0] : 0.f;
        g = in ? t[p1] : 0.f;
        b = in ? t[p2] : 0.f;
    });
}

template <int DT, int MODE>
__global__ void __launch_bounds__(256) k_ingest_image(IngestArgs a, ImageArgs s)
{
    using E = ImgElem<DT>;
    using raw = typename E::raw;
    __shared__ float tile[3 * IM_PLANE];
    const int x0 = blockIdx.x * IG_T, y0 = blockIdx.y * IG_T;
    const int nx = min(IG_T, a.W - x0), ny = min(IG_T, a.H - y0);
    const raw* src = static_cast<const raw*>(s.in) + int64_t(blockIdx.z) * s.sn + int64_t(y0) * s.sy + int64_t(x0) * s.sx;
    if (s.form == IM_ROWVEC)
    {
        // sx == 1; the base and sn, sc, sy are multiples of four elements (host-checked) and x0 is a multiple of 64
        struct alignas(4 * sizeof(raw)) Quad
        {
            raw v[4];
        };
        const int nq = nx >> 2;
        // (constant trip counts, so that the loads of all the passes are in flight together)
#pragma unroll
        for (int c = 0; c < 3; c++)
        {
            if (c < s.nIn)
            {
                const raw* pc = src + int64_t(c) * s.sc;
                float* tc = tile + c * IM_PLANE;
#pragma unroll
                for (int pass = 0; pass < IG_T * 16 / 256; pass++)
                {
                    const int i = threadIdx.x + pass * 256;
                    const int yy = i >> 4, q = i & 15;
                    const raw* rp = pc + int64_t(yy) * s.sy + 4 * q;
                    float* t = tc + im_slot(yy) * IM_PITCH + 4 * q;
                    if (yy < ny && q < nq)
                    {
                        const Quad v = *reinterpret_cast<const Quad*>(rp);
#pragma unroll
                        for (int j = 0; j < 4; j++)
                        {
                            t[j] = E::cvt(v.v[j]);
                        }
                    }
                    else if (yy < ny && q == nq)
                    {
                        for (int j = 0; 4 * q + j < nx; j++) // the row's tail: element by element
                        {
                            t[j] = E::cvt(rp[j]);
                        }
                    }
                }
            }
        }
    }
    else if (s.form == IM_PACKED)
    {
        // sc == +-1, sx == 3 or 4, three planes; the base is a multiple of the element size (host-checked)
        const int rev = s.sc < 0;
        im_load_packed<DT>(src - (rev ? 2 : 0), s.sy, nx, int(s.sx), rev, ny,
            [&](int c, int i, int x, raw v) { tile[c * IM_PLANE + im_slot(i) * IM_PITCH + x] = E::cvt(v); });
    }
    else
    {
        for (int c = 0; c < s.nIn; c++)
        {
            const raw* pc = src + int64_t(c) * s.sc;
            float* tc = tile + c * IM_PLANE;
#pragma unroll 8
            for (int pass = 0; pass < IG_T * IG_T / 256; pass++)
            {
                const int i = threadIdx.x + pass * 256;
                const int yy = i >> 6, xx = i & 63;
                if (yy < ny && xx < nx)
                {
                    tc[im_slot(yy) * IM_PITCH + xx] = E::cvt(pc[int64_t(yy) * s.sy + int64_t(xx) * s.sx]);
                }
            }
        }
    }
    __syncthreads();
    im_store_phase<MODE>(a, tile, s.nIn, x0, y0, nx, ny);
}

// ------------------------------------------------------------------------
// YUV 4:2:0 video frames (NV12 / NV21) -> 8-bit R, G, B: cvtColor(COLOR_YUV2RGB_NV12 / _NV21), the call the apps make before
// Detector::operator()(const cv::Mat&).  OpenCV is not part of the reference tree: this is the published algorithm of
// imgproc/src/color_yuv.simd.hpp restated (BT.601 limited range, 20-bit fixed point, int32, arithmetic shift; the chroma pair of a
// 2 x 2 block shared by its four pixels, no interpolation) — PARITY UNPINNED.
// Frame: H rows of W luma bytes, rowStride apart; at chromaOff H / 2 rows of W / 2 byte pairs (U, V; vFirst: V, U), same stride.
//
// The ONE statement of that formula, for every acf_hip_yuv_format (the video entries) and sample width:
//   CF   false: the default format, {8, 0, BT601, 0}, with cvtColor's constants inline — immediates, so every default instantiation is
//        the kernel it was before there were formats; true: the constants of acf_hip_yuv_coeffs, an argument (YuvCoef)
//   ACC  int for 8-bit samples: int32 holds every sum for all six matrix / range rows (|219 * CY| + 2^19 + |CUB| * 128 < 2^31);
//        int64_t above: 20 fractional bits and 16-bit samples do not fit int32 ((1023 - 64) * CY + CUB * 512 > 2^31), so the sums are
//        64-bit (a v_mad_i64_i32 for the luma term, 64-bit adds and shifts behind it)
// ------------------------------------------------------------------------
struct YuvCoef
{
    int yoff, cmid, omax;
    int cy, cvr, cvg, cug, cub;
    float sc; // float(1.0 / omax): a sample as a plane value
};
template <class ACC>
struct YuvChromaT
{
    ACC ruv, guv, buv;
};
using YuvChroma = YuvChromaT<int>;
template <class T>
using YuvAcc = std::conditional_t<sizeof(T) == 1, int, int64_t>; // by sample type
template <bool CF, class ACC = int>
__device__ __forceinline__ YuvChromaT<ACC> yuv_chroma(int u, int v, const YuvCoef& k)
{
    const ACC cvr = CF ? k.cvr : 1673527, cvg = CF ? k.cvg : -852492, cug = CF ? k.cug : -409993, cub = CF ? k.cub : 2116026;
    u -= CF ? k.cmid : 128;
    v -= CF ? k.cmid : 128;
    return { (1 << 19) + cvr * v, (1 << 19) + cvg * v + cug * u, (1 << 19) + cub * u };
}
// R, G, B in [0, omax].  |sum| < 2^38 (16-bit samples, constants below 2^22), so sum >> 20 fits int32: the clamp is a 32-bit one
template <bool CF, class ACC>
__device__ __forceinline__ void yuv_rgb(int Y, const YuvChromaT<ACC>& c, const YuvCoef& k, int& r, int& g, int& b)
{
    const int omax = CF ? k.omax : 255;
    const ACC y = ACC(max(0, Y - (CF ? k.yoff : 16))) * (CF ? k.cy : 1220542);
    r = min(max(int((y + c.ruv) >> 20), 0), omax);
    g = min(max(int((y + c.guv) >> 20), 0), omax);
    b = min(max(int((y + c.buv) >> 20), 0), omax);
}
// ... as the plane values a store phase's px yields: the integers times sc = float(1.0 / omax)
template <bool CF, class ACC>
__device__ __forceinline__ void yuv_px(int Y, const YuvChromaT<ACC>& c, const YuvCoef& k, float sc, float& r, float& g, float& b)
{
    int R, G, B;
    yuv_rgb<CF>(Y, c, k, R, G, B);
    r = float(R) * sc;
    g = float(G) * sc;
    b = float(B) * sc;
}

struct YuvSrc
{
    const uint8_t* in;
    int H, W;          // even
    int rowStride;     // bytes between rows, luma and chroma alike
    int vFirst;        // NV21
    int64_t chromaOff; // bytes from a frame's first luma byte to its first chroma byte
    int64_t in_fs;     // bytes between frames
    YuvCoef k;         // CF instantiations only (a format other than the default)
};

// The unfused form: tight packed RGB bytes [H][W][3] per frame (in front of k_resize_u8, acf_hip_op_yuv420_to_rgb, and the
// fallback yuv_unfused of k_ingest_yuv420).  One thread per 2 x 2 block; byte accesses, so any base and stride.
__global__ void __launch_bounds__(256) k_yuv420_to_rgb8(YuvSrc s, uint8_t* __restrict__ dst)
{
    const int bx = blockIdx.x * 64 + (threadIdx.x & 63), by = blockIdx.y * 4 + (threadIdx.x >> 6);
    if (2 * bx >= s.W || 2 * by >= s.H)
    {
        return;
    }
    const uint8_t* __restrict__ F = s.in + int64_t(blockIdx.z) * s.in_fs;
    const uint8_t* __restrict__ C = F + s.chromaOff + int64_t(by) * s.rowStride + 2 * bx;
    const YuvChroma c = yuv_chroma<false>(C[s.vFirst], C[1 - s.vFirst], s.k);
    uint8_t* __restrict__ D = dst + int64_t(blockIdx.z) * s.H * s.W * 3;
#pragma unroll
    for (int j = 0; j < 2; j++)
    {
        const uint8_t* __restrict__ L = F + int64_t(2 * by + j) * s.rowStride + 2 * bx;
        uint8_t* __restrict__ d = D + (int64_t(2 * by + j) * s.W + 2 * bx) * 3;
#pragma unroll
        for (int i = 0; i < 2; i++)
        {
            int r, g, b;
            yuv_rgb<false>(L[i], c, s.k, r, g, b);
            d[3 * i] = uint8_t(r);
            d[3 * i + 1] = uint8_t(g);
            d[3 * i + 2] = uint8_t(b);
        }
    }
}

// The hot path: NV12 / NV21 -> transposed planar f32, the model's colour conversion in registers: k_ingest_u8's tile and lane
// assignment (a workgroup owns 64 x 64 pixels; a lane takes four consecutive image-y of one image-x and stores one float4 a
// plane), with the 8-bit R, G, B of the integer formula in between, times float(1 / 255.0) as there — so the planes are those of
// k_ingest_u8 on the converted RGB frame, bit for bit.  a.in / cpp / ro / go / bo / rowStride / in_fs of IngestArgs are not read.
//
// LDS: 64 luma rows and 32 chroma rows of 16 dwords.  In the convert phase a 32-lane half (the unit bank conflicts count in;
// 32 banks for byte reads and dword writes) is 16 row-quads x 2 adjacent image-x, which share a dword: 16 addresses, luma rows
// 4k + j and chroma rows 2k + i, k = 0 .. 15.  At any plain pitch p those are 4kp (2kp) dwords apart: at most 8 (16) banks.  So
// the rows are stored regrouped — luma row r in slot (r & 3) * 16 + (r >> 2), chroma row r in slot (r & 1) * 16 + (r >> 1) —
// at a pitch of 17 dwords: the 16 rows of one read are then 17 dwords apart, 17k mod 32 = k (k even), 16 + k (k odd): 16
// distinct banks.  In the load phase a half writes 16 dwords of each of two adjacent rows r, r + 1 (r even), 16 slots =
// 272 = 16 (mod 32) dwords apart: 32 distinct banks.  (96 x 17 dwords = 6528 bytes.)
constexpr int YG_PITCH = 68; // bytes; 17 dwords
__device__ __forceinline__ int yg_luma_slot(int r)
{
    return (r & 3) * 16 + (r >> 2);
}
__device__ __forceinline__ int yg_chroma_slot(int r)
{
    return IG_T + (r & 1) * 16 + (r >> 1);
}

template <int MODE, bool ALIGNED, bool CF = false>
__global__ void __launch_bounds__(256) k_ingest_yuv420(IngestArgs a, YuvSrc s)
{
    __shared__ uint32_t tileW[(IG_T + IG_T / 2) * YG_PITCH / 4];
    uint8_t* tile = reinterpret_cast<uint8_t*>(tileW);
    const int x0 = blockIdx.x * IG_T, y0 = blockIdx.y * IG_T;
    const int nx = min(IG_T, a.W - x0), ny = min(IG_T, a.H - y0); // both even
    const uint8_t* luma = s.in + int64_t(blockIdx.z) * s.in_fs + int64_t(y0) * s.rowStride + x0;
    const uint8_t* chroma = s.in + int64_t(blockIdx.z) * s.in_fs + s.chromaOff + int64_t(y0 >> 1) * s.rowStride + x0;
    const int nRows = ny + (ny >> 1); // luma rows, then chroma rows: nx bytes each
    if (ALIGNED)
    {
        // base, row stride, chroma offset and frame stride are multiples of 4 (host-checked) and x0 is a multiple of 64;
        // a row's last dword is whole or holds one byte pair (nx is even): that pair is read as 16 bits, nothing beyond the row
        for (int i = threadIdx.x; i < nRows * 16; i += 256)
        {
            const int row = i >> 4, j = i & 15;
            if (4 * j < nx)
            {
                const uint8_t* rp = (row < ny ? luma + int64_t(row) * s.rowStride : chroma + int64_t(row - ny) * s.rowStride) + 4 * j;
                const uint32_t v = (4 * j + 4 <= nx) ? *reinterpret_cast<const uint32_t*>(rp) : uint32_t(*reinterpret_cast<const uint16_t*>(rp));
                tileW[(row < ny ? yg_luma_slot(row) : yg_chroma_slot(row - ny)) * (YG_PITCH / 4) + j] = v;
            }
        }
    }
    else
    {
        for (int i = threadIdx.x; i < nRows * 64; i += 256)
        {
            const int row = i >> 6, j = i & 63;
            if (j < nx)
            {
                const uint8_t* rp = row < ny ? luma + int64_t(row) * s.rowStride : chroma + int64_t(row - ny) * s.rowStride;
                tile[(row < ny ? yg_luma_slot(row) : yg_chroma_slot(row - ny)) * YG_PITCH + j] = rp[j];
            }
        }
    }
    __syncthreads();
    // ingest_store_phase written out for this kernel (kept apart deliberately: profiles/ingest_refactor.md): the chroma pair of a 2 x 2
    // block once for its two rows
    const int yq = (threadIdx.x & 15) * 4;
    const float sc = float(1.0 / 255.0);
    float* outF = a.out + int64_t(blockIdx.z) * a.out_fs;
    const int64_t np = int64_t(a.H) * a.W;
    for (int xx = threadIdx.x >> 4; xx < nx; xx += 16)
    {
        float o[3][4];
#pragma unroll
        for (int i = 0; i < 2; i++)
        {
            const uint8_t* cp = tile + yg_chroma_slot((yq >> 1) + i) * YG_PITCH + (xx & ~1);
            const YuvChroma c = yuv_chroma<CF>(cp[s.vFirst], cp[1 - s.vFirst], s.k);
#pragma unroll
            for (int jj = 0; jj < 2; jj++)
            {
                const int j = 2 * i + jj;
                int r, g, b;
                yuv_rgb<CF>(tile[yg_luma_slot(yq + j) * YG_PITCH + xx], c, s.k, r, g, b);
                ingest_convert<MODE>(a, float(r) * sc, float(g) * sc, float(b) * sc, o, j);
            }
        }
        ingest_store<MODE>(a, o, outF + int64_t(x0 + xx) * a.H + y0 + yq, np, ny - yq);
    }
}

// ------------------------------------------------------------------------
// YUV frames of three planes, each with its own offset and byte strides (acf_hip_yuv_desc: I420 / YV12 / I422 / I444 planar, YUYV /
// UYVY / YVYU packed 4:2:2, NV12 / NV21, separately allocated planes, odd sizes) -> 8-bit R, G, B by yuv_chroma / yuv_rgb above.
// Pixel (r, c) of frame n: Y at y.off + n * y.sn + r * y.sr + c * y.sp, U and V likewise at (r >> subY, c >> subX): no interpolation.
// The cvtColor codes for I420 / YV12 / YUY2 / UYVY / YVYU share the fixed-point helpers of NV12 / NV21 in OpenCV's published
// imgproc/src/color_yuv.simd.hpp; I422 / I444 are the same per-pixel formula — PARITY UNPINNED.
// ------------------------------------------------------------------------
struct YuvPlane
{
    int64_t off, sn, sr, sp; // bytes: first sample, between frames, between the plane's rows, between its samples
};
struct YuvDescSrc
{
    const uint8_t* base;
    YuvPlane y, u, v;
    int subX, subY;        // 0 or 1
    int yPos, uPos, vPos;  // YD_PACKED422: byte of Y0 (Y1 two further), U, V inside the macropixel at `mp`
    int64_t mp;            // YD_PACKED422: offset of the first macropixel (4-aligned with base)
    YuvCoef k;             // CF instantiations only (a format other than the default)
};
enum
{
    YD_GENERIC = 0,   // byte loads, any strides
    YD_PLANAR = 1,    // all three sp == 1; base + off, sr, sn multiples of 4: dword loads
    YD_PACKED422 = 2  // 4:2:2 macropixels of four bytes; base + mp, sr, sn multiples of 4: one dword = two pixels
};

// The descriptor form of k_yuv420_to_rgb8: tight packed RGB bytes [rows][cols][3] per frame.  One thread per pixel; byte accesses.
template <bool CF = false>
__global__ void __launch_bounds__(256) k_yuv_to_rgb8(YuvDescSrc s, int rows, int cols, uint8_t* __restrict__ dst)
{
    const int c = blockIdx.x * 64 + (threadIdx.x & 63), r = blockIdx.y * 4 + (threadIdx.x >> 6);
    if (c >= cols || r >= rows)
    {
        return;
    }
    const int64_t n = blockIdx.z;
    const int cr = r >> s.subY, cc = c >> s.subX;
    const uint8_t* __restrict__ B = s.base;
    const int Y = B[s.y.off + n * s.y.sn + int64_t(r) * s.y.sr + int64_t(c) * s.y.sp];
    const int U = B[s.u.off + n * s.u.sn + int64_t(cr) * s.u.sr + int64_t(cc) * s.u.sp];
    const int V = B[s.v.off + n * s.v.sn + int64_t(cr) * s.v.sr + int64_t(cc) * s.v.sp];
    int R, G, Bl;
    yuv_rgb<CF>(Y, yuv_chroma<CF>(U, V, s.k), s.k, R, G, Bl);
    uint8_t* d = dst + ((n * rows + r) * cols + c) * 3;
    d[0] = uint8_t(R);
    d[1] = uint8_t(G);
    d[2] = uint8_t(Bl);
}

// The hot path: k_ingest_yuv420's shape (a workgroup owns 64 x 64 pixels; the load phase runs lanes along the rows of each plane into
// LDS byte tiles; then a lane takes four consecutive image-y of one image-x, converts and stores one float4 a plane through
// ingest_convert / ingest_store) for any acf_hip_yuv_desc, so the planes are those of k_ingest_u8 on the converted RGB frame, bit
// for bit.  Sizes may be odd (IG_LUV, the scalar rgb2luv body, is reachable here): the tile then has ceil(ny / 2^subY) chroma
// rows of ceil(nx / 2^subX) samples.  a.in / cpp / ro / go / bo / rowStride / in_fs of IngestArgs are not read.
//
// Load forms (FORM, chosen on the host from the descriptor and the base's alignment alone; all give the same tiles):
//   YD_PLANAR     every plane's rows as dwords by consecutive lanes; the nb % 4 bytes at a row's end one by one
//   YD_PACKED422  a lane's dword is one macropixel = two pixels: Y0, Y1 to the luma tile, U and V to theirs; the half macropixel
//                 at an odd row end byte by byte
//   YD_GENERIC    one sample a lane, any strides
// No load covers a byte outside the span the same row of the same plane addresses (YD_PACKED422: of the macropixels the row
// addresses), so a plane may end with its allocation.
//
// LDS: three byte tiles (Y, U, V) of 64 slots x 17 dwords; luma row r in slot (r & 3) * 16 + (r >> 2) as k_ingest_yuv420, chroma
// row r in the same slot when subY == 0, in (r & 1) * 16 + (r >> 1) when subY == 1.  Bank = dword address % 32 per 32-lane half:
//   convert phase (byte reads)  a half is 16 row-quads x 2 adjacent image-x, which share a dword of each tile (columns xx or
//                               xx >> 1): read j takes luma rows 4k + j = slots 16j + k and chroma rows (4k + j) >> subY = slots
//                               16j + k or 16(j >> 1) + k, k = 0 .. 15: 17k mod 32: 16 distinct banks, conflict-free, for each tile
//   YD_PLANAR (dword writes)    luma, and chroma with subX == 0: a half writes the 16 dwords of rows r, r + 1 (r even), 16 slots =
//                               272 = 16 (mod 32) dwords apart: 32 distinct banks.  Chroma with subX == 1: the 8 dwords of rows
//                               r .. r + 3: slots 0, 16, 1, 17 (subY == 1) or 0, 16, 32, 48 (subY == 0) -> bank offsets 0, 16, 17,
//                               1 or 0, 16, 0, 16: 2-way (no extra cycles on ds_write_b32)
//   YD_PACKED422                a half is the 32 macropixels of one row: 16-bit luma writes two lanes a dword, chroma byte writes
//                               four lanes a dword, over 16 and 8 distinct banks
//   YD_GENERIC (byte writes)    a half writes 32 consecutive samples of one row: four lanes a dword, 8 distinct banks
// (degrees derived from the address maps above with the bank rule; whether sub-dword writes of several lanes to one dword
// serialise, and the SQ_LDS_BANK_CONFLICT counter: not measured.)  3 x 64 x 17 dwords = 13056 bytes.
// ------------------------------------------------------------------------
constexpr int YD_TILE = IG_T * YG_PITCH; // bytes between the Y, U and V tiles
constexpr int Y16_PITCH = 66;               // k_ingest_yuv16's tiles (their layout is derived there): samples; 33 dwords
constexpr int Y16_TILE = IG_T * Y16_PITCH;  // samples between the Y, U and V tiles
// The tiles by sample type: T = uint8_t (k_ingest_yuv) or uint16_t (k_ingest_yuv16)
template <class T>
struct YdTile
{
    static constexpr int PER = 4 / int(sizeof(T));                      // samples a dword
    static constexpr int PITCH = sizeof(T) == 1 ? YG_PITCH : Y16_PITCH; // samples
    static constexpr int TILE = IG_T * PITCH;                           // samples between the Y, U and V tiles
};

__device__ __forceinline__ int yd_slot(int r, int subY)
{
    return subY ? (r & 1) * 16 + (r >> 1) : (r & 3) * 16 + (r >> 2);
}

// YD_PLANAR / YD16_PLANAR: rows x ns samples of one plane (first byte p, sr bytes apart) to a tile of T; 1 << lg dwords a tile row,
// PASSES * 256 >= rows << lg (constant trip counts, so that the loads of all the passes are in flight together).  The samples behind a
// row's last whole dword: bytes one by one; of 16-bit words there is one, read as one 16-bit load.  16-bit words are shifted and masked
// on the way in (shift, mask: not read for bytes).
template <class T, int PASSES>
__device__ __forceinline__ void yd_load_rows_vec(const uint8_t* __restrict__ p, int64_t sr, int rows, int ns, int lg, int slotSubY, int shift, uint32_t mask,
    uint32_t* tileW)
{
    constexpr int PER = YdTile<T>::PER;
#pragma unroll
    for (int pass = 0; pass < PASSES; pass++)
    {
        const int i = threadIdx.x + pass * 256;
        const int row = i >> lg, j = i & ((1 << lg) - 1);
        if (row < rows && PER * j < ns)
        {
            const uint8_t* rp = p + int64_t(row) * sr + 4 * j;
            uint32_t v;
            if (PER * j + PER <= ns)
            {
                v = *reinterpret_cast<const uint32_t*>(rp);
            }
            else if constexpr (sizeof(T) == 2)
            {
                v = uint32_t(*reinterpret_cast<const uint16_t*>(rp));
            }
            else
            {
                v = 0;
                for (int b = 0; b < ns - 4 * j; b++)
                {
                    v |= uint32_t(rp[b]) << (8 * b);
                }
            }
            if constexpr (sizeof(T) == 2)
            {
                v = (((v & 0xffffu) >> shift) & mask) | ((((v >> 16) >> shift) & mask) << 16);
            }
            tileW[yd_slot(row, slotSubY) * (YdTile<T>::PITCH / PER) + j] = v;
        }
    }
}

// YD_GENERIC: rows x cols samples of one plane (sp apart in a row); 1 << lg lanes a tile row
__device__ __forceinline__ void yd_load_rows_generic(const uint8_t* __restrict__ p, int64_t sr, int64_t sp, int rows, int cols, int lg, int slotSubY, uint8_t* tile)
{
    for (int i = threadIdx.x; i < (rows << lg); i += 256)
    {
        const int row = i >> lg, col = i & ((1 << lg) - 1);
        if (col < cols)
        {
            tile[yd_slot(row, slotSubY) * YG_PITCH + col] = p[int64_t(row) * sr + int64_t(col) * sp];
        }
    }
}

// YD_PACKED422: the macropixel at rp (four bytes: Y0 at yPos, Y1 two further, U and V at uPos, vPos) as one dword when `whole`; else
// — an odd row's last pixel — the three bytes of its first half only (Y1 = 0)
__device__ __forceinline__ void yd_macropixel(const uint8_t* rp, bool whole, const YuvDescSrc& s, uint32_t& Y0, uint32_t& Y1, uint32_t& U, uint32_t& V)
{
    if (whole)
    {
        const uint32_t w = *reinterpret_cast<const uint32_t*>(rp);
        Y0 = (w >> (8 * s.yPos)) & 255;
        Y1 = (w >> (8 * s.yPos + 16)) & 255;
        U = (w >> (8 * s.uPos)) & 255;
        V = (w >> (8 * s.vPos)) & 255;
    }
    else
    {
        Y0 = rp[s.yPos];
        Y1 = 0;
        U = rp[s.uPos];
        V = rp[s.vPos];
    }
}

// The store phase on three tiles (Y, U, V) of T, chroma at the planes' own resolution: k_ingest_yuv's and k_ingest_yuv16's.  sc: float(1.0 / omax)
template <int MODE, bool CF, class T>
__device__ __forceinline__ void yd_store_phase(const IngestArgs& a, const YuvDescSrc& s, const T* tile, float sc, int x0, int y0, int nx, int ny)
{
    constexpr int PITCH = YdTile<T>::PITCH, TILE = YdTile<T>::TILE;
    const int subX = s.subX, subY = s.subY;
    YuvChromaT<YuvAcc<T>> c{}; // of the chroma row that tile row yq + j lies in: kept from one j to the next
    ingest_store_phase<MODE>(a, x0, y0, nx, ny, [&](int xx, int yq, int j, float& r, float& g, float& b) {
        if (j == 0 || (j >> subY) != ((j - 1) >> subY)) // a new chroma row (uniform: subY is)
        {
            const int at = yd_slot((yq + j) >> subY, subY) * PITCH + (xx >> subX);
            c = yuv_chroma<CF, YuvAcc<T>>(tile[TILE + at], tile[2 * TILE + at], s.k);
        }
        yuv_px<CF>(tile[yd_slot(yq + j, 0) * PITCH + xx], c, s.k, sc, r, g, b);
    });
}

template <int MODE, int FORM, bool CF = false>
__global__ void __launch_bounds__(256) k_ingest_yuv(IngestArgs a, YuvDescSrc s)
{
    __shared__ uint32_t tileW[3 * YD_TILE / 4];
    uint8_t* tile = reinterpret_cast<uint8_t*>(tileW);
    const int x0 = blockIdx.x * IG_T, y0 = blockIdx.y * IG_T;
    const int nx = min(IG_T, a.W - x0), ny = min(IG_T, a.H - y0);
    const int subX = s.subX, subY = s.subY;
    const int cnx = (nx + subX) >> subX, cny = (ny + subY) >> subY; // chroma samples a tile row, chroma rows (x0, y0 are even)
    const int64_t n = blockIdx.z;
    if (FORM == YD_PACKED422)
    {
        // subX == 1, subY == 0; the three planes share sr and sn; base + mp, sr, sn are multiples of 4 (host-checked) and x0 * 2 is
        const uint8_t* src = s.base + s.mp + n * s.y.sn + int64_t(y0) * s.y.sr + int64_t(x0) * 2;
        uint16_t* tile16 = reinterpret_cast<uint16_t*>(tile);
#pragma unroll 4
        for (int pass = 0; pass < IG_T * 32 / 256; pass++)
        {
            const int i = threadIdx.x + pass * 256;
            const int row = i >> 5, q = i & 31;
            if (row < ny && 2 * q < nx)
            {
                const uint8_t* rp = src + int64_t(row) * s.y.sr + 4 * q;
                uint32_t Y0, Y1, U, V;
                yd_macropixel(rp, 2 * q + 1 < nx, s, Y0, Y1, U, V);
                const int at = yd_slot(row, 0) * YG_PITCH;
                tile16[(at >> 1) + q] = uint16_t(Y0 | (Y1 << 8));
                tile[YD_TILE + at + q] = uint8_t(U);
                tile[2 * YD_TILE + at + q] = uint8_t(V);
            }
        }
    }
    else
    {
        const uint8_t* py = s.base + s.y.off + n * s.y.sn + int64_t(y0) * s.y.sr + int64_t(x0) * s.y.sp;
        const uint8_t* pu = s.base + s.u.off + n * s.u.sn + int64_t(y0 >> subY) * s.u.sr + int64_t(x0 >> subX) * s.u.sp;
        const uint8_t* pv = s.base + s.v.off + n * s.v.sn + int64_t(y0 >> subY) * s.v.sr + int64_t(x0 >> subX) * s.v.sp;
        if (FORM == YD_PLANAR)
        {
            // sp == 1; base + off, sr, sn of every plane are multiples of 4 (host-checked) and x0 >> subX is a multiple of 32
            yd_load_rows_vec<uint8_t, 4>(py, s.y.sr, ny, nx, 4, 0, 0, 0, tileW);
            yd_load_rows_vec<uint8_t, 4>(pu, s.u.sr, cny, cnx, 4 - subX, subY, 0, 0, tileW + YD_TILE / 4);
            yd_load_rows_vec<uint8_t, 4>(pv, s.v.sr, cny, cnx, 4 - subX, subY, 0, 0, tileW + 2 * YD_TILE / 4);
        }
        else
        {
            yd_load_rows_generic(py, s.y.sr, s.y.sp, ny, nx, 6, 0, tile);
            yd_load_rows_generic(pu, s.u.sr, s.u.sp, cny, cnx, 6 - subX, subY, tile + YD_TILE);
            yd_load_rows_generic(pv, s.v.sr, s.v.sp, cny, cnx, 6 - subX, subY, tile + 2 * YD_TILE);
        }
    }
    __syncthreads();
    yd_store_phase<MODE, CF>(a, s, tile, float(1.0 / 255.0), x0, y0, nx, ny);
}

// ------------------------------------------------------------------------
// YUV frames of 9 .. 16-bit samples (acf_hip_yuv_format with bits > 8: P010 / P012 / P016, yuv420p10le, I210, I410, Y210 ...): every
// sample is one little-endian 16-bit word at the descriptor's BYTE offsets and strides, sample = (word >> shift) & ((1 << bits) - 1).
// R, G, B in [0, omax] by the formula of acf_hip_yuv_coeffs in exact integers: 20 fractional bits and 16-bit samples do not fit
// int32 ((1023 - 64) * CY + CUB * 512 > 2^31), so the sums are int64 (a v_mad_i64_i32 for the luma term, 64-bit adds and shifts behind
// it); plane value = float(R) * float(1.0 / omax), so the planes are those of k_ingest_image on a tight packed float32 RGB image
// holding these values, bit for bit.  H.273 gives the matrices; there is no OpenCV counterpart — PARITY UNPINNED.
// ------------------------------------------------------------------------
struct Yuv16Src
{
    YuvDescSrc yuv;    // byte offsets and strides, all even (host-checked); yuv.k: the format's constants
    int shift, mask;   // sample = (word >> shift) & mask
    int vFirst;        // YD16_PAIRS: a chroma dword is (V, U)
};
enum
{
    YD16_GENERIC = 0, // 16-bit loads, any even offsets and strides
    YD16_PLANAR = 1,  // all three sp == 2; base + off, sr, sn of every plane multiples of 4: a dword holds two samples
    YD16_PAIRS = 2    // luma as YD16_PLANAR; U and V interleaved 16-bit pairs, 4-aligned: a chroma dword is one (U, V) or (V, U) pair
};

// The conversion alone for more than 8 bits: tight packed [rows][cols][3] per frame, uint16 samples in [0, omax].  One thread a pixel.
// (k_yuv_to_rgb8 with 16-bit words and the 64-bit accumulator; the two are kept apart deliberately: profiles/ingest_refactor.md)
__global__ void __launch_bounds__(256) k_video_to_rgb16(Yuv16Src S, int rows, int cols, uint16_t* __restrict__ dst)
{
    const int c = blockIdx.x * 64 + (threadIdx.x & 63), r = blockIdx.y * 4 + (threadIdx.x >> 6);
    if (c >= cols || r >= rows)
    {
        return;
    }
    const YuvDescSrc& s = S.yuv;
    const int64_t n = blockIdx.z;
    const int cr = r >> s.subY, cc = c >> s.subX;
    const uint8_t* __restrict__ B = s.base;
    const auto at = [&](const YuvPlane& p, int pr, int pc) {
        return (int(*reinterpret_cast<const uint16_t*>(B + p.off + n * p.sn + int64_t(pr) * p.sr + int64_t(pc) * p.sp)) >> S.shift) & S.mask;
    };
    int R, G, Bl;
    yuv_rgb<true>(at(s.y, r, c), yuv_chroma<true, int64_t>(at(s.u, cr, cc), at(s.v, cr, cc), s.k), s.k, R, G, Bl);
    uint16_t* d = dst + ((n * rows + r) * cols + c) * 3;
    d[0] = uint16_t(R);
    d[1] = uint16_t(G);
    d[2] = uint16_t(Bl);
}

// The hot path: k_ingest_yuv's shape for 16-bit words.  A workgroup owns 64 x 64 pixels; the load phase runs lanes along the rows of
// each plane into three LDS tiles of 16-bit samples, masked and shifted on the way in; then the shared store phase: a lane takes four
// consecutive image-y of one image-x through ingest_convert / ingest_store, one float4 a plane.  Sizes may be odd (IG_LUV is reachable):
// ceil(ny / 2^subY) chroma rows of ceil(nx / 2^subX) samples.  a.in / cpp / ro / go / bo / rowStride / in_fs of IngestArgs are not read.
//
// Load forms (FORM, chosen on the host from the descriptor and the base's alignment alone; all give the same tiles):
//   YD16_PLANAR   every plane's rows as dwords (two samples) by consecutive lanes; an odd row's last sample as one 16-bit load
//   YD16_PAIRS    luma as YD16_PLANAR; a lane's chroma dword is one pair: one sample to the U tile, one to the V tile
//   YD16_GENERIC  one 16-bit load a lane and sample, any even strides (packed 4:2:2 of words — Y210 — runs here)
// No load covers a byte outside the [first, last] span the same row of the same plane addresses (YD16_PAIRS: of the pairs the row
// addresses), so a plane may end with its allocation.
//
// LDS: three tiles (Y, U, V) of 64 slots x 33 dwords (66 samples, 64 used); row r of a plane in slot yd_slot(r, its subY): luma
// (r & 3) * 16 + (r >> 2), chroma the same when subY == 0, (r & 1) * 16 + (r >> 1) when subY == 1.  Bank = dword address % 32 per
// 32-lane half (MI355X LDS rule for 4-byte and narrower accesses); 16 slots are 16 * 33 = 528 = 16 (mod 32) dwords apart, one slot 1:
//   store phase (16-bit reads)  a half is 16 row-quads x 2 adjacent image-x (xx even, xx + 1), which share a dword of the luma tile
//                               (column xx >> 1) and a dword or a sample of the chroma tiles: read j takes luma rows 4k + j = slots
//                               16j + k and chroma rows (4k + j) >> subY = slots 16j + k or 16(j >> 1) + k, k = 0 .. 15: banks
//                               16j + k + const (mod 32): 16 distinct banks, conflict-free, for each tile
//   YD16_PLANAR (dword writes)  luma, and chroma with subX == 0: a half writes the 32 dwords of one row: 32 distinct banks.  Chroma
//                               with subX == 1: the 16 dwords of rows r, r + 1 (r even): 16 slots apart with either row order =
//                               16 (mod 32) dwords: 32 distinct banks
//   YD16_PAIRS chroma           a half is the 32 pairs of one row: 16-bit writes, two lanes a dword, 16 distinct banks a tile
//   YD16_GENERIC                a half writes 32 consecutive samples of one row: two lanes a dword, 16 distinct banks
// (degrees derived from the address maps with the bank rule; whether 16-bit writes of two lanes to one dword serialise, and the
// SQ_LDS_BANK_CONFLICT counter: not measured.)  3 x 64 x 33 dwords = 25344 bytes: six workgroups a CU by LDS.  By the compiler's resource
// report (-Rpass-analysis=kernel-resource-usage, gfx950; all twelve instantiations): 35 .. 44 VGPRs, 63 .. 88 SGPRs, no scratch, 6 waves a SIMD.
// YD16_GENERIC: rows x cols samples of one plane (sp bytes apart in a row); 1 << lg lanes a tile row
__device__ __forceinline__ void y16_load_rows_generic(const uint8_t* __restrict__ p, int64_t sr, int64_t sp, int rows, int cols, int lg, int slotSubY, int shift,
    int mask, uint16_t* tile)
{
#pragma unroll 4
    for (int i = threadIdx.x; i < (rows << lg); i += 256)
    {
        const int row = i >> lg, col = i & ((1 << lg) - 1);
        if (col < cols)
        {
            const int w = *reinterpret_cast<const uint16_t*>(p + int64_t(row) * sr + int64_t(col) * sp);
            tile[yd_slot(row, slotSubY) * Y16_PITCH + col] = uint16_t((w >> shift) & mask);
        }
    }
}

template <int MODE, int FORM>
__global__ void __launch_bounds__(256) k_ingest_yuv16(IngestArgs a, Yuv16Src S)
{
    __shared__ uint32_t tileW[3 * Y16_TILE / 2];
    uint16_t* tile = reinterpret_cast<uint16_t*>(tileW);
    const YuvDescSrc& s = S.yuv;
    const int x0 = blockIdx.x * IG_T, y0 = blockIdx.y * IG_T;
    const int nx = min(IG_T, a.W - x0), ny = min(IG_T, a.H - y0);
    const int subX = s.subX, subY = s.subY;
    const int cnx = (nx + subX) >> subX, cny = (ny + subY) >> subY; // chroma samples a tile row, chroma rows (x0, y0 are even)
    const int64_t n = blockIdx.z;
    const int shift = S.shift, mask = S.mask;
    const uint8_t* py = s.base + s.y.off + n * s.y.sn + int64_t(y0) * s.y.sr + int64_t(x0) * s.y.sp;
    const uint8_t* pu = s.base + s.u.off + n * s.u.sn + int64_t(y0 >> subY) * s.u.sr + int64_t(x0 >> subX) * s.u.sp;
    const uint8_t* pv = s.base + s.v.off + n * s.v.sn + int64_t(y0 >> subY) * s.v.sr + int64_t(x0 >> subX) * s.v.sp;
    if (FORM == YD16_PLANAR)
    {
        // sp == 2; base + off, sr, sn of every plane are multiples of 4 (host-checked) and (x0 >> subX) * 2 is
        yd_load_rows_vec<uint16_t, 8>(py, s.y.sr, ny, nx, 5, 0, shift, uint32_t(mask), tileW);
        yd_load_rows_vec<uint16_t, 8>(pu, s.u.sr, cny, cnx, 5 - subX, subY, shift, uint32_t(mask), tileW + Y16_TILE / 2);
        yd_load_rows_vec<uint16_t, 8>(pv, s.v.sr, cny, cnx, 5 - subX, subY, shift, uint32_t(mask), tileW + 2 * (Y16_TILE / 2));
    }
    else if (FORM == YD16_PAIRS)
    {
        // luma as planar; chroma: u.sp == v.sp == 4, the two planes 2 bytes apart with one sr and sn, the lower one 4-aligned with base
        yd_load_rows_vec<uint16_t, 8>(py, s.y.sr, ny, nx, 5, 0, shift, uint32_t(mask), tileW);
        const uint8_t* pc = S.vFirst ? pv : pu; // the pair's first word
        const int lg = 6 - subX;
#pragma unroll 4
        for (int i = threadIdx.x; i < (cny << lg); i += 256)
        {
            const int row = i >> lg, col = i & ((1 << lg) - 1);
            if (col < cnx)
            {
                const uint32_t w = *reinterpret_cast<const uint32_t*>(pc + int64_t(row) * s.u.sr + 4 * col);
                const uint32_t lo = ((w & 0xffffu) >> shift) & uint32_t(mask), hi = ((w >> 16) >> shift) & uint32_t(mask);
                const int at = yd_slot(row, subY) * Y16_PITCH + col;
                tile[Y16_TILE + at] = uint16_t(S.vFirst ? hi : lo);
                tile[2 * Y16_TILE + at] = uint16_t(S.vFirst ? lo : hi);
            }
        }
    }
    else
    {
        y16_load_rows_generic(py, s.y.sr, s.y.sp, ny, nx, 6, 0, shift, mask, tile);
        y16_load_rows_generic(pu, s.u.sr, s.u.sp, cny, cnx, 6 - subX, subY, shift, mask, tile + Y16_TILE);
        y16_load_rows_generic(pv, s.v.sr, s.v.sp, cny, cnx, 6 - subX, subY, shift, mask, tile + 2 * Y16_TILE);
    }
    __syncthreads();
    yd_store_phase<MODE, true>(a, s, tile, s.k.sc, x0, y0, nx, ny);
}

// ------------------------------------------------------------------------
// Rotated and mirrored frames (acf_hip_*_oriented, orientation codes 1 .. 7; code 0 runs the kernels above): the source frame S of
// Hs x Ws pixels is read where it lies and the planes are those of the upright frame U = np.rot90(S[:, ::-1] if mirror else S, -rot).
// Upright pixel (r, c) is source pixel (rs, cs):
//     swap == 0 (rot 0 / 2):  rs = revR ? Hs - 1 - r : r,  cs = revC ? Ws - 1 - c : c
//     swap == 1 (rot 1 / 3):  rs = revR ? Hs - 1 - c : c,  cs = revC ? Ws - 1 - r : r
// (rot 1: swap, revR; rot 2: revR, revC; rot 3: swap, revC; mirror flips revC.)  All three are runtime arguments.
//
// A workgroup owns 64 x 64 UPRIGHT pixels, as every ingest kernel; they are one 64 x 64 (ragged: nsr x nsc) rectangle of the source,
// whose first row / column is anywhere (Hs - y0 - ny ...), not on a multiple of 64.  Both kernels work the same way:
//   load phase   lanes run along the SOURCE rows of that rectangle, whichever way the frame is turned, with the wide loads of the
//                un-oriented kernels (below), so the loads are coalesced in every orientation;
//   placement    every element goes to the LDS tile at its UPRIGHT position (orient_up): the reversals and, for swap, the transpose
//                happen here, and the chroma sample of a subsampled plane is chosen here, in source coordinates, and written to
//                each of the (up to four) pixels of the rectangle that take it;
//   store phase  the shared one, on a tile that holds the upright pixels: a lane takes four consecutive image-y of one image-x through
//                the model's colour conversion and stores one float4 a plane (coalesced along image-y).
// Profile names: *_oriented_rows (swap == 0) and *_oriented_cols (swap == 1) with a wide load form, *_oriented_generic with the
// element-wise one.  For swap the four image-y a lane stores ARE four neighbouring source pixels of one source row, so planar sources
// could go from registers to the float4 store without LDS; the tile is kept for them too — one placement and one store phase for every
// layout (packed pixels, macropixels and subsampled chroma need the stage anyway), and LDS traffic is not what bounds a kernel that
// moves 1 .. 12 bytes in and 4 .. 12 bytes out per pixel through HBM (profiles/oriented_entry.md holds what was measured).
//
// Because the rectangle starts anywhere, a row's wide loads are the ALIGNED words that hold a piece of it (at most 17 quads / dwords
// for 64 elements); a word is loaded whole only when all of it lies inside the rectangle, else its elements inside the rectangle one by
// one.  So no load covers an address outside the [first, last] span the same row of the same plane addresses.
//
// LDS banks (bank = dword address % 32, per 32-lane half), the image kernel (float tile of k_ingest_image: row r in slot
// (r & 3) * 16 + (r >> 2), pitch 66 dwords, planes 64 * 66 + 11 apart):
//   store phase (reads)      k_ingest_image's: conflict-free
//   rows, IM_ROWVEC writes   a lane's element t of quad q goes to upright x = +-(4q + t) + const of one slot; a half is 17 quads of
//                            one row then 15 of the next (another slot: a multiple of 66 dwords away): stride-4 columns -> 8 banks a
//                            row, 4-way, as k_ingest_image's IM_ROWVEC
//   cols, IM_ROWVEC writes   element t of quad q goes to upright row 4q' + t' (the quads of the rectangle are not those of the
//                            upright rows unless Ws % 4 == 0), column = the source row: per ds_write the lanes of one source row
//                            write slots 16 t' + q', 66 dwords apart -> banks 2q' + const, 16 or 17 distinct; the second source row
//                            of the half is one column (one bank) further: 2-way at worst
//   IM_PACKED / IM_GENERIC   rows: as k_ingest_image.  cols: consecutive pixels of a source row go down one tile column, rows
//                            r, r + 1, .. -> slots 16 apart = 1056 = 0 (mod 32) dwords for r & 3 = 0 .. 2, then + 66: the pixels of
//                            one lane group fall on 8 .. 9 banks, up to 4-way for f32 (one pixel a lane), less for the narrower
//                            types whose lanes share pixels.
// The YUV kernel (three byte tiles Y, U, V at the UPRIGHT resolution, each 64 slots x 17 dwords as k_ingest_yuv's luma tile):
//   store phase (byte reads) the luma pattern of k_ingest_yuv for all three tiles: 16 distinct banks, conflict-free
//   rows, dword loads        four bytes of a lane go to four adjacent bytes of one slot (forwards or backwards): one dword or two
//   cols, dword loads        four bytes of a lane go to four slots 16 apart (272 = 16 (mod 32) dwords): 2 banks a lane; the lanes
//                            of a source row walk 17 dwords a quad: conflict degree <= 4 on byte writes
// (degrees derived from the address maps with the bank rule; SQ_LDS_BANK_CONFLICT was not read.)
// ------------------------------------------------------------------------
struct OrientSrc
{
    int Hs, Ws;           // source rows, columns
    int swap, revR, revC; // the map above
};

// The source rectangle of a workgroup's upright tile, and where its elements go
struct OrientTile
{
    int rs0, cs0, nsr, nsc; // first source row / column, rows, columns
    int swap, revR, revC;
    // upright tile position (yy, xx) of the rectangle's element (i, j)
    __device__ __forceinline__ void up(int i, int j, int& yy, int& xx) const
    {
        const int p = revR ? nsr - 1 - i : i, q = revC ? nsc - 1 - j : j;
        yy = swap ? q : p;
        xx = swap ? p : q;
    }
};
__device__ __forceinline__ OrientTile orient_tile(const OrientSrc& o, int x0, int y0, int nx, int ny)
{
    OrientTile t;
    t.swap = o.swap;
    t.revR = o.revR;
    t.revC = o.revC;
    t.nsr = o.swap ? nx : ny;
    t.nsc = o.swap ? ny : nx;
    const int r0 = o.swap ? x0 : y0, c0 = o.swap ? y0 : x0;
    t.rs0 = o.revR ? o.Hs - r0 - t.nsr : r0;
    t.cs0 = o.revC ? o.Ws - c0 - t.nsc : c0;
    return t;
}

constexpr int OR_WORDS = 17; // aligned 4-element words that can hold a piece of 64 consecutive elements

struct ImageOrientedSrc
{
    ImageArgs im; // the description at Hs x Ws; form: the load form, by imageLoadForm's conditions
    OrientSrc o;
};

template <int DT, int MODE>
__global__ void __launch_bounds__(256) k_ingest_image_oriented(IngestArgs a, ImageOrientedSrc S)
{
    using E = ImgElem<DT>;
    using raw = typename E::raw;
    __shared__ float tile[3 * IM_PLANE];
    const ImageArgs& s = S.im;
    const int x0 = blockIdx.x * IG_T, y0 = blockIdx.y * IG_T;
    const int nx = min(IG_T, a.W - x0), ny = min(IG_T, a.H - y0);
    const OrientTile T = orient_tile(S.o, x0, y0, nx, ny);
    const auto place = [&](int c, int i, int j, raw v) {
        int yy, xx;
        T.up(i, j, yy, xx);
        tile[c * IM_PLANE + im_slot(yy) * IM_PITCH + xx] = E::cvt(v);
    };
    // the frame's row T.rs0, column 0 (the row starts keep the alignment the host checked)
    const raw* rows = static_cast<const raw*>(s.in) + int64_t(blockIdx.z) * s.sn + int64_t(T.rs0) * s.sy;
    if (s.form == IM_ROWVEC)
    {
        // sx == 1; the base and sn, sc, sy are multiples of four elements (host-checked)
        struct alignas(4 * sizeof(raw)) Quad
        {
            raw v[4];
        };
        const int e0 = T.cs0 & ~3, e1 = T.cs0 + T.nsc; // the first quad's first column; one past the last column
        for (int c = 0; c < s.nIn; c++)
        {
            const raw* pc = rows + int64_t(c) * s.sc;
#pragma unroll 2
            for (int idx = threadIdx.x; idx < T.nsr * OR_WORDS; idx += 256)
            {
                const int i = idx / OR_WORDS, col = e0 + 4 * (idx - i * OR_WORDS);
                if (col >= e1)
                {
                    continue;
                }
                const raw* rp = pc + int64_t(i) * s.sy + col;
                if (col >= T.cs0 && col + 4 <= e1)
                {
                    const Quad v = *reinterpret_cast<const Quad*>(rp);
#pragma unroll
                    for (int t = 0; t < 4; t++)
                    {
                        place(c, i, col + t - T.cs0, v.v[t]);
                    }
                }
                else
                {
                    for (int t = 0; t < 4; t++) // a quad over one end of the rectangle: only the elements inside it
                    {
                        if (col + t >= T.cs0 && col + t < e1)
                        {
                            place(c, i, col + t - T.cs0, rp[t]);
                        }
                    }
                }
            }
        }
    }
    else if (s.form == IM_PACKED)
    {
        // k_ingest_image's IM_PACKED on the rectangle's rows
        const int rev = s.sc < 0;
        im_load_packed<DT>(rows + int64_t(T.cs0) * s.sx - (rev ? 2 : 0), s.sy, T.nsc, int(s.sx), rev, T.nsr, place);
    }
    else
    {
        // one element a lane, lanes along the source row, any strides
        for (int c = 0; c < s.nIn; c++)
        {
            const raw* pc = rows + int64_t(c) * s.sc + int64_t(T.cs0) * s.sx;
#pragma unroll 4
            for (int idx = threadIdx.x; idx < T.nsr * IG_T; idx += 256)
            {
                const int i = idx >> 6, j = idx & 63;
                if (j < T.nsc)
                {
                    place(c, i, j, pc[int64_t(i) * s.sy + int64_t(j) * s.sx]);
                }
            }
        }
    }
    __syncthreads();
    im_store_phase<MODE>(a, tile, s.nIn, x0, y0, nx, ny);
}

// The YUV twin.  Load forms (YuvOrientedSrc::form, chosen on the host from the description and the base's alignment alone; all give
// the same tiles):
//   YD_PLANAR     (yuvLoadForm's conditions) every plane's rows as aligned dwords by consecutive lanes
//   YD_PACKED422  (yuvLoadForm's conditions) a lane's dword is one macropixel = two source pixels; the rectangle may start or end on
//                 half a macropixel: the dword is still inside the row's macropixels, and only the pixels inside the rectangle are placed
//   YO_SEMI       luma rows as YD_PLANAR; chroma is one plane of byte pairs (U, V or V, U: NV12 / NV21 of any size and strides, 4-aligned):
//                 a lane's dword is two chroma samples
//   YD_GENERIC    one sample a lane, any strides
constexpr int YO_SEMI = 3;

struct YuvOrientedSrc
{
    YuvDescSrc yuv; // the description at Hs x Ws (yPos .. mp as yuvLoadForm fills them)
    OrientSrc o;
    int form;
    int vFirst;     // YO_SEMI: the pair is V, U
};

// one sample v of plane `tile` (plane row pr, plane column pc; lsy, lsx: the plane's subsampling shifts) to every pixel of the
// rectangle that takes it
__device__ __forceinline__ void yo_spread(const OrientTile& T, uint8_t* tile, int pr, int pc, int lsy, int lsx, uint8_t v)
{
    for (int dy = 0; dy <= lsy; dy++)
    {
        const int i = (pr << lsy) + dy - T.rs0;
        if (i < 0 || i >= T.nsr)
        {
            continue;
        }
        for (int dx = 0; dx <= lsx; dx++)
        {
            const int j = (pc << lsx) + dx - T.cs0;
            if (j >= 0 && j < T.nsc)
            {
                int yy, xx;
                T.up(i, j, yy, xx);
                tile[yd_slot(yy, 0) * YG_PITCH + xx] = v;
            }
        }
    }
}

// YD_GENERIC: the samples of one plane that the rectangle takes, one a lane
__device__ __forceinline__ void yo_load_generic(const OrientTile& T, const uint8_t* __restrict__ frame, const YuvPlane& p, int lsy, int lsx, uint8_t* tile)
{
    const int pr0 = T.rs0 >> lsy, nPr = ((T.rs0 + T.nsr - 1) >> lsy) - pr0 + 1;
    const int pc0 = T.cs0 >> lsx, nPc = ((T.cs0 + T.nsc - 1) >> lsx) - pc0 + 1;
    for (int idx = threadIdx.x; idx < nPr * IG_T; idx += 256)
    {
        const int pr = pr0 + (idx >> 6), pc = pc0 + (idx & 63);
        if (pc < pc0 + nPc)
        {
            yo_spread(T, tile, pr, pc, lsy, lsx, frame[int64_t(pr) * p.sr + int64_t(pc) * p.sp]);
        }
    }
}

// YD_PLANAR: the same with the aligned dwords of each plane row (sp == 1; frame + row starts are multiples of 4)
__device__ __forceinline__ void yo_load_vec(const OrientTile& T, const uint8_t* __restrict__ frame, const YuvPlane& p, int lsy, int lsx, uint8_t* tile)
{
    const int pr0 = T.rs0 >> lsy, nPr = ((T.rs0 + T.nsr - 1) >> lsy) - pr0 + 1;
    const int pc0 = T.cs0 >> lsx, pc1 = ((T.cs0 + T.nsc - 1) >> lsx) + 1; // [pc0, pc1)
    const int e0 = pc0 & ~3;
#pragma unroll 2
    for (int idx = threadIdx.x; idx < nPr * OR_WORDS; idx += 256)
    {
        const int r = idx / OR_WORDS, col = e0 + 4 * (idx - r * OR_WORDS), pr = pr0 + r;
        if (col >= pc1)
        {
            continue;
        }
        const uint8_t* rp = frame + int64_t(pr) * p.sr + col;
        if (col >= pc0 && col + 4 <= pc1)
        {
            const uint32_t w = *reinterpret_cast<const uint32_t*>(rp);
#pragma unroll
            for (int t = 0; t < 4; t++)
            {
                yo_spread(T, tile, pr, col + t, lsy, lsx, uint8_t(w >> (8 * t)));
            }
        }
        else
        {
            for (int t = 0; t < 4; t++) // a dword over one end of the rectangle's samples: only those inside
            {
                if (col + t >= pc0 && col + t < pc1)
                {
                    yo_spread(T, tile, pr, col + t, lsy, lsx, rp[t]);
                }
            }
        }
    }
}

// CF: the conversion's constants go through LDS (36 bytes, written first, read behind the barrier into vector registers): the load
// phase runs at the scalar register limit, and nine more live scalars spilled to scratch
template <bool CF>
__device__ __forceinline__ YuvCoef* yo_coef_lds()
{
    if constexpr (CF)
    {
        __shared__ YuvCoef kS;
        return &kS;
    }
    else
    {
        return nullptr;
    }
}

template <int MODE, bool CF = false>
__global__ void __launch_bounds__(256) k_ingest_yuv_oriented(IngestArgs a, YuvOrientedSrc S)
{
    __shared__ uint32_t tileW[3 * YD_TILE / 4];
    uint8_t* tile = reinterpret_cast<uint8_t*>(tileW);
    const YuvDescSrc& s = S.yuv;
    if (CF && threadIdx.x == 0)
    {
        *yo_coef_lds<CF>() = s.k;
    }
    const int x0 = blockIdx.x * IG_T, y0 = blockIdx.y * IG_T;
    const int nx = min(IG_T, a.W - x0), ny = min(IG_T, a.H - y0);
    const OrientTile T = orient_tile(S.o, x0, y0, nx, ny);
    const int subX = s.subX, subY = s.subY;
    const int64_t n = blockIdx.z;
    const uint8_t* fy = s.base + s.y.off + n * s.y.sn;
    const uint8_t* fu = s.base + s.u.off + n * s.u.sn;
    const uint8_t* fv = s.base + s.v.off + n * s.v.sn;
    if (S.form == YD_PACKED422)
    {
        // subX == 1, subY == 0; the three planes share sr and sn; base + mp, sr, sn are multiples of 4 (host-checked)
        const uint8_t* src = s.base + s.mp + n * s.y.sn + int64_t(T.rs0) * s.y.sr;
        const int m0 = T.cs0 >> 1, nm = ((T.cs0 + T.nsc - 1) >> 1) - m0 + 1; // the macropixels a row of the rectangle touches: <= 33
#pragma unroll 2
        for (int idx = threadIdx.x; idx < T.nsr * IG_T; idx += 256)
        {
            const int i = idx >> 6, q = idx & 63;
            if (q >= nm)
            {
                continue;
            }
            const int m = m0 + q;
            const uint8_t* rp = src + int64_t(i) * s.y.sr + 4 * int64_t(m);
            uint32_t Y[2], U, V;
            yd_macropixel(rp, 2 * m + 1 < S.o.Ws, s, Y[0], Y[1], U, V);
#pragma unroll
            for (int t = 0; t < 2; t++)
            {
                const int j = 2 * m + t - T.cs0;
                if (j >= 0 && j < T.nsc)
                {
                    int yy, xx;
                    T.up(i, j, yy, xx);
                    const int at = yd_slot(yy, 0) * YG_PITCH + xx;
                    tile[at] = uint8_t(Y[t]);
                    tile[YD_TILE + at] = uint8_t(U);
                    tile[2 * YD_TILE + at] = uint8_t(V);
                }
            }
        }
    }
    else if (S.form == YD_PLANAR)
    {
        yo_load_vec(T, fy, s.y, 0, 0, tile);
        yo_load_vec(T, fu, s.u, subY, subX, tile + YD_TILE);
        yo_load_vec(T, fv, s.v, subY, subX, tile + 2 * YD_TILE);
    }
    else if (S.form == YO_SEMI)
    {
        // subX == 1; y.sp == 1; the chroma pairs are four-aligned with their rows, as the luma rows (host-checked)
        yo_load_vec(T, fy, s.y, 0, 0, tile);
        const uint8_t* fc = S.vFirst ? fv : fu; // the pair's first byte
        const int uAt = 8 * S.vFirst, vAt = 8 - uAt;
        const int pr0 = T.rs0 >> subY, nPr = ((T.rs0 + T.nsr - 1) >> subY) - pr0 + 1;
        const int pc0 = T.cs0 >> 1, pc1 = ((T.cs0 + T.nsc - 1) >> 1) + 1; // pairs [pc0, pc1)
        const int e0 = pc0 & ~1;
#pragma unroll 2
        for (int idx = threadIdx.x; idx < nPr * OR_WORDS; idx += 256)
        {
            const int r = idx / OR_WORDS, col = e0 + 2 * (idx - r * OR_WORDS), pr = pr0 + r;
            if (col >= pc1)
            {
                continue;
            }
            const uint8_t* rp = fc + int64_t(pr) * s.u.sr + 2 * col;
            uint32_t w;
            if (col >= pc0 && col + 2 <= pc1)
            {
                w = *reinterpret_cast<const uint32_t*>(rp);
            }
            else
            {
                const int t = col >= pc0 ? 0 : 1; // the one pair inside
                w = (uint32_t(rp[2 * t]) | (uint32_t(rp[2 * t + 1]) << 8)) << (16 * t);
            }
#pragma unroll
            for (int t = 0; t < 2; t++)
            {
                if (col + t >= pc0 && col + t < pc1)
                {
                    yo_spread(T, tile + YD_TILE, pr, col + t, subY, 1, uint8_t(w >> (16 * t + uAt)));
                    yo_spread(T, tile + 2 * YD_TILE, pr, col + t, subY, 1, uint8_t(w >> (16 * t + vAt)));
                }
            }
        }
    }
    else
    {
        yo_load_generic(T, fy, s.y, 0, 0, tile);
        yo_load_generic(T, fu, s.u, subY, subX, tile + YD_TILE);
        yo_load_generic(T, fv, s.v, subY, subX, tile + 2 * YD_TILE);
    }
    __syncthreads();
    const YuvCoef k = CF ? *yo_coef_lds<CF>() : YuvCoef{};
    ingest_store_phase<MODE>(a, x0, y0, nx, ny, [&](int xx, int yq, int j, float& r, float& g, float& b) {
        const int at = yd_slot(yq + j, 0) * YG_PITCH + xx; // all three tiles are at the upright resolution
        yuv_px<CF>(tile[at], yuv_chroma<CF>(tile[YD_TILE + at], tile[2 * YD_TILE + at], k), k, float(1.0 / 255.0), r, g, b);
    });
}

// ------------------------------------------------------------------------
// The apps' resize to a minimum object width (src/app/acf/acf.cpp:117-148 `Resizer`, GPUDetectionPipeline.cpp:250-266):
// cv::resize of the packed 8-bit image by scale = winSize.width / minWidth, INTER_AREA when reducing, INTER_LINEAR else.
// OpenCV is not part of the reference tree: the arithmetic is the published algorithm of imgproc/resize.cpp for CV_8U,
// written down in DESIGN.md 6b (and restated on the CPU by the test checker) — PARITY UNPINNED.  One thread per
// output pixel (all channels); the tap tables are built on the host in double precision (host_plan.cpp).
//   RZ_LINEAR    x: {sx, a0, a1, two} per column, y: {r0, r1, b0, b1} per row; 11-bit fixed point:
//                (((b0 * (h0 >> 4)) >> 16) + ((b1 * (h1 >> 4)) >> 16) + 2) >> 2 with h = S[sx] * a0 + S[sx + 1] * a1
//   RZ_AREA      fractional scales: per output column / row a run of {source index, float weight}; per source row
//                buf = sum S * alpha (taps ascending, from 0), then sum = beta * buf (first row), sum += beta * buf; cvRound
//   RZ_AREA_INT  integral scales: (a + b + c + d + 2) >> 2 for 2 x 2, else cvRound(int sum * float(1 / area)); cells that
//                reach past the source: cvRound(float(sum) / count) over the pixels inside
// ------------------------------------------------------------------------
enum
{
    RZ_LINEAR = 0,
    RZ_AREA = 1,
    RZ_AREA_INT = 2
};
// The tap tables and source size of one resize: what the per-pixel arithmetic reads besides the source
struct ResizeTaps
{
    int32_t rows, cols;  // source size
    int32_t mode, isx, isy;
    const int4* xlin;   // RZ_LINEAR [dcols]
    const int4* ylin;   // RZ_LINEAR [drows]
    const int2* xrun;   // RZ_AREA [dcols] {first tap, count}
    const int2* yrun;   // RZ_AREA [drows]
    const int2* xtap;   // RZ_AREA {source column, float bits}
    const int2* ytap;
};
struct ResizeArgs
{
    const uint8_t* src;
    uint8_t* dst;
    int32_t cn, stride, drows, dcols;
    int64_t src_fs, dst_fs; // bytes per frame
    ResizeTaps t;
};
__device__ __forceinline__ uint8_t rz_sat_u8(float v)
{
    const int i = __float2int_rn(v); // cvRound: round half to even
    return uint8_t(min(max(i, 0), 255));
}

// Source accessors of rz_pixel: px(y, x, v) gives the cn (<= 4) channels of source pixel (y, x) as ints 0 .. 255, all at once.
// A packed 8-bit frame: cn interleaved bytes a pixel
struct RzPackedSrc
{
    const uint8_t* S; // the frame
    int stride, cn;
    __device__ __forceinline__ void px(int y, int x, int (&v)[4]) const
    {
        const uint8_t* p = S + int64_t(y) * stride + x * cn;
#pragma unroll
        for (int c = 0; c < 4; c++)
        {
            v[c] = c < cn ? p[c] : 0;
        }
    }
};

// One output pixel (dx, dy) of the resize, every channel: the ONE statement of the three forms' arithmetic (k_resize_u8 on a packed
// frame, k_ingest_resized on an image's strides or a YUV description).  Channels are independent, so reading a source pixel once for
// all of them changes no bit.
template <class SRC>
__device__ __forceinline__ void rz_pixel(const SRC& s, const ResizeTaps& a, int dx, int dy, uint8_t (&out)[4])
{
    int v[4];
    if (a.mode == RZ_LINEAR)
    {
        const int4 X = a.xlin[dx], Y = a.ylin[dy];
        int p0[4], p1[4], q0[4] = { 0, 0, 0, 0 }, q1[4] = { 0, 0, 0, 0 };
        s.px(Y.x, X.x, p0);
        s.px(Y.y, X.x, p1);
        if (X.w) // (beyond xmax the second tap is not read: S[sx] * 2048)
        {
            s.px(Y.x, X.x + 1, q0);
            s.px(Y.y, X.x + 1, q1);
        }
#pragma unroll
        for (int c = 0; c < 4; c++)
        {
            const int h0 = X.w ? p0[c] * X.y + q0[c] * X.z : p0[c] * 2048;
            const int h1 = X.w ? p1[c] * X.y + q1[c] * X.z : p1[c] * 2048;
            out[c] = uint8_t((((Y.z * (h0 >> 4)) >> 16) + ((Y.w * (h1 >> 4)) >> 16) + 2) >> 2);
        }
        return;
    }
    if (a.mode == RZ_AREA_INT)
    {
        const int sy0 = dy * a.isy, sx0 = dx * a.isx;
        const bool partial = sy0 + a.isy > a.rows || sx0 + a.isx > a.cols;
        const int ny = min(a.isy, a.rows - sy0), nx = min(a.isx, a.cols - sx0);
        const float sc = 1.f / float(a.isx * a.isy);
        int sum[4] = { 0, 0, 0, 0 };
        for (int y = 0; y < ny; y++)
        {
            for (int x = 0; x < nx; x++)
            {
                s.px(sy0 + y, sx0 + x, v);
#pragma unroll
                for (int c = 0; c < 4; c++)
                {
                    sum[c] += v[c];
                }
            }
        }
        const int count = max(ny, 0) * max(nx, 0);
#pragma unroll
        for (int c = 0; c < 4; c++)
        {
            if (partial)
            {
                out[c] = count > 0 ? rz_sat_u8(float(sum[c]) / float(count)) : uint8_t(0);
            }
            else
            {
                out[c] = (a.isx == 2 && a.isy == 2) ? uint8_t((sum[c] + 2) >> 2) : rz_sat_u8(float(sum[c]) * sc);
            }
        }
        return;
    }
    const int2 xr = a.xrun[dx], yr = a.yrun[dy];
    float sum[4] = { 0.f, 0.f, 0.f, 0.f };
    for (int j = 0; j < yr.y; j++)
    {
        const int2 ty = a.ytap[yr.x + j];
        float buf[4] = { 0.f, 0.f, 0.f, 0.f };
        for (int k = 0; k < xr.y; k++)
        {
            const int2 tx = a.xtap[xr.x + k];
            s.px(ty.x, tx.x, v);
#pragma unroll
            for (int c = 0; c < 4; c++)
            {
                buf[c] = buf[c] + float(v[c]) * __int_as_float(tx.y);
            }
        }
#pragma unroll
        for (int c = 0; c < 4; c++)
        {
            const float t = __int_as_float(ty.y) * buf[c];
            sum[c] = j == 0 ? t : sum[c] + t;
        }
    }
#pragma unroll
    for (int c = 0; c < 4; c++)
    {
        out[c] = rz_sat_u8(sum[c]);
    }
}

__global__ void __launch_bounds__(256) k_resize_u8(ResizeArgs a)
{
    const int dx = blockIdx.x * 64 + (threadIdx.x & 63), dy = blockIdx.y * 4 + (threadIdx.x >> 6);
    if (dx >= a.dcols || dy >= a.drows)
    {
        return;
    }
    const RzPackedSrc s{ a.src + int64_t(blockIdx.z) * a.src_fs, a.stride, a.cn };
    uint8_t* __restrict__ D = a.dst + int64_t(blockIdx.z) * a.dst_fs + (int64_t(dy) * a.dcols + dx) * a.cn;
    uint8_t o[4];
    rz_pixel(s, a.t, dx, dy, o);
#pragma unroll
    for (int c = 0; c < 4; c++)
    {
        if (c < a.cn)
        {
            D[c] = o[c];
        }
    }
}

// ------------------------------------------------------------------------
// The apps' resize inside the tensor and YUV entries (acf_hip_pyramid_image_resized / _yuv_resized): the caller's bytes -> the
// converted planar f32 image at the reduced size in one kernel, defined as the existing entries composed — acf_hip_yuv_to_rgb8 (or the
// addressed bytes as an interleaved image), k_resize_u8's arithmetic (rz_pixel), k_ingest_u8 — bit for bit.  cvtColor and cv::resize
// stay restated: PARITY UNPINNED.
//
// k_ingest_u8's shape: a workgroup of 256 threads owns a 64 x 64 tile of the REDUCED image.
//   phase 1  lanes run along reduced-image x (a wave = one tile row, 16 rows a wave): rz_pixel over a source accessor (the image's
//            n / c / y / x element strides; or Y at (r, c), U and V at (r >> sub_y, c >> sub_x) through yuv_chroma / yuv_rgb, once per
//            source pixel for its three channels), the bytes into k_ingest_u8's LDS byte tile (pitch 260; r, g, b at 0, 1, 2 of 3)
//   phase 2  ingest_store_tile: k_ingest_u8's store phase
// No load touches a byte outside what the description addresses at the source size: rz_pixel reads source pixels inside
// [0, rows) x [0, cols) only (RZ_LINEAR's second tap only where the table's fourth field says so; partial area cells clamp).
//
// LDS (bank = dword address % 32, per 32-lane half): phase 1 writes bytes 3 * xx + c of one row: a half covers 24 dwords, up to two
// lanes a dword for one c (byte writes of several lanes to one dword: whether they serialise was not measured); phase 2 reads as
// k_ingest_u8 does (16 row-quads a half at a pitch of 65 dwords: 16 distinct banks).  64 x 260 = 16640 bytes.
// ------------------------------------------------------------------------
struct RzImageSrc
{
    const uint8_t* in; // frame n's element (0, 0, 0)
    int64_t sc, sy, sx;
    int nIn;
    __device__ __forceinline__ void px(int y, int x, int (&v)[4]) const
    {
        const uint8_t* p = in + int64_t(y) * sy + int64_t(x) * sx;
        v[0] = p[0];
        v[1] = nIn == 3 ? p[sc] : 0;
        v[2] = nIn == 3 ? p[2 * sc] : 0;
        v[3] = 0;
    }
};
template <bool CF>
struct RzYuvSrcT
{
    const uint8_t *py, *pu, *pv; // frame n's first sample of each plane
    int64_t ysr, ysp, usr, usp, vsr, vsp;
    int subX, subY;
    YuvCoef k; // CF only
    __device__ __forceinline__ void px(int y, int x, int (&v)[4]) const
    {
        const int cr = y >> subY, cc = x >> subX;
        const int Y = py[int64_t(y) * ysr + int64_t(x) * ysp];
        const int U = pu[int64_t(cr) * usr + int64_t(cc) * usp];
        const int V = pv[int64_t(cr) * vsr + int64_t(cc) * vsp];
        yuv_rgb<CF>(Y, yuv_chroma<CF>(U, V, k), k, v[0], v[1], v[2]);
        v[3] = 0;
    }
};
using RzYuvSrc = RzYuvSrcT<false>;
enum
{
    RS_IMAGE = 0,
    RS_YUV = 1,
    RS_YUV_CF = 2 // RS_YUV with the conversion's constants from yuv.k (a format other than the default)
};
struct ResizedSrc
{
    ImageArgs im;   // RS_IMAGE (u8 elements; form is not read)
    YuvDescSrc yuv; // RS_YUV
    ResizeTaps t;
};
// rz_pixel's global accessor of frame n for SRC: of the image description, or of the YUV one
template <int SRC>
__device__ __forceinline__ auto rz_global_src(const ResizedSrc& s, int64_t n)
{
    if constexpr (SRC == RS_IMAGE)
    {
        return RzImageSrc{ static_cast<const uint8_t*>(s.im.in) + n * s.im.sn, s.im.sc, s.im.sy, s.im.sx, s.im.nIn };
    }
    else
    {
        const YuvDescSrc& d = s.yuv;
        return RzYuvSrcT<SRC == RS_YUV_CF>{ d.base + d.y.off + n * d.y.sn, d.base + d.u.off + n * d.u.sn, d.base + d.v.off + n * d.v.sn, d.y.sr, d.y.sp, d.u.sr, d.u.sp,
            d.v.sr, d.v.sp, d.subX, d.subY, d.k };
    }
}
// Phase 1 of k_ingest_oriented_resized's two forms, for a lane with a tile column (lanes run along reduced-image x, a wave a tile row: xx = threadIdx.x & 63
// < nx, which the caller checks before it builds `src`: with that check in here, by the compiler's resource report, the kernels took
// 14 .. 18 more scalar registers and some lost a wave of occupancy): rz_pixel over `src` for rows yFirst, yFirst + 4, .. < yEnd of
// column xx, the bytes into k_ingest_u8's byte tile as r, g, b at 0, 1, 2 of 3
template <class SRC>
__device__ __forceinline__ void rz_fill_tile(const SRC& src, const ResizeTaps& t, int cn, int x0, int y0, int xx, int yFirst, int yEnd, uint8_t* tile)
{
    for (int yy = yFirst; yy < yEnd; yy += 4)
    {
        uint8_t o[4];
        rz_pixel(src, t, x0 + xx, y0 + yy, o);
        uint8_t* p = tile + yy * IG_PITCH + 3 * xx;
        p[0] = o[0];
        p[1] = cn == 3 ? o[1] : o[0]; // one plane: r = g = b (chnsPyramid.cpp:234-244), as k_ingest_u8 reads a 1-byte pixel
        p[2] = cn == 3 ? o[2] : o[0];
    }
}

template <int SRC, int MODE>
__global__ void __launch_bounds__(256) k_ingest_resized(IngestArgs a, ResizedSrc s)
{
    __shared__ uint32_t tileW[IG_T * IG_PITCH / 4];
    uint8_t* tile = reinterpret_cast<uint8_t*>(tileW);
    const int x0 = blockIdx.x * IG_T, y0 = blockIdx.y * IG_T;
    const int nx = min(IG_T, a.W - x0), ny = min(IG_T, a.H - y0);
    const int64_t n = blockIdx.z;
    const int xx = threadIdx.x & 63;
    if (xx < nx)
    {
        // rz_fill_tile's loop written out, the accessor built inside it (kept apart deliberately: profiles/ingest_refactor.md)
        const int cn = SRC != RS_IMAGE ? 3 : s.im.nIn;
        for (int yy = threadIdx.x >> 6; yy < ny; yy += 4)
        {
            uint8_t o[4];
            rz_pixel(rz_global_src<SRC>(s, n), s.t, x0 + xx, y0 + yy, o);
            uint8_t* t = tile + yy * IG_PITCH + 3 * xx;
            t[0] = o[0];
            t[1] = cn == 3 ? o[1] : o[0]; // one plane: r = g = b, as rz_fill_tile
            t[2] = cn == 3 ? o[2] : o[0];
        }
    }
    __syncthreads();
    ingest_store_tile<MODE>(a, tile, 3, 0, 1, 2, x0, y0, nx, ny);
}

// ------------------------------------------------------------------------
// The apps' resize on rotated and mirrored frames (acf_hip_pyramid_image_oriented_resized / _yuv_oriented_resized, codes 1 .. 7; code 0
// runs k_ingest_resized): the stored frame S of Hs x Ws is read where it lies, and the planes are those of k_ingest_resized on a tight
// upright u8 image holding U = np.rot90(S[:, ::-1] if mirror else S, -rot) — orient FIRST, then rz_pixel with the tap tables of U's size,
// as the reference's GL front end does (GPUACF.cpp: rotate -> smooth -> reduce) — bit for bit.  cvtColor and cv::resize stay restated:
// PARITY UNPINNED.  The chroma sample of a subsampled plane is chosen in SOURCE coordinates, as the oriented entries do.
//
// STAGED (k_ingest_oriented_resized_image / _yuv; taken for quarter turns, see planOrientedResized).  k_ingest_resized gathers per output pixel from global memory with lanes along
// reduced-image x; with a quarter turn every lane of a wave would read another stored row.  Here a workgroup of 256 threads owns a
// 64 x 64 tile of the REDUCED upright image and marches it in bands of `band` reduced rows (chosen on the host, orientedResizedBand, so
// that every band's footprint fits the stage; 64 = one band):
//   footprint  rz_span: the first and last tap of the band's first and last row and of the tile's first and last column (xlin / ylin,
//              xrun / xtap, dx * isx), clipped to U; orient_tile maps that rectangle of U to a rectangle of S (nsr x nsc from rs0, cs0)
//   load       lanes run along the STORED rows of the rectangle, whichever way the frame is turned: with S.vec (imageLoadForm's
//              IM_ROWVEC / yuvLoadForm's YD_PLANAR conditions) a lane takes the aligned quad of source columns 4q .. 4q + 3: one dword a
//              plane (a 2 x-subsampled chroma plane: one 16-bit load); else one pixel a lane, byte loads.  A word is loaded whole only
//              when all of it lies inside the row of its plane ([0, Ws), chroma [0, ceil(Ws / 2))), else its bytes inside one by one:
//              no load covers an address outside the [first, last] span of the row and plane it belongs to.  YUV goes through
//              yuv_chroma / yuv_rgb here, once per source pixel (chroma at (rs >> subY, cs >> subX))
//   stage      pixel (i, j) of the rectangle is ONE dword r | g << 8 | b << 16 (one plane: the byte) at i * pitch + j, pitch = nsc | 1
//   resize     rz_pixel, unchanged, over RzStageSrc, which applies the orientation in its index arithmetic (base + y * ay + x * ax:
//              ay, ax are +-pitch and +-1, swapped for quarter turns); lanes along reduced-image x, a wave a row, the bytes into
//              k_ingest_u8's LDS byte tile as k_ingest_resized writes them
//   store      ingest_store_tile, once the last band is in
// LDS: stage OS_STAGE = 8448 dwords (33792 bytes: a 64 x 64 tile at scale 1 / 2 is 64 + 64 rows of 129 dwords = two bands; at 1 / 4 a band
// of 8 reduced rows is 32 rows of 257) + the byte tile 16640 = 50432 bytes a workgroup: three workgroups a CU of 160 KiB.  A band
// below OS_MIN_BAND = 8 rows (scales under 1 / 4: two barriers for less than two rows a wave) takes the generic form instead.
// By the compiler's resource report (-Rpass-analysis=kernel-resource-usage, gfx950): staged 52 VGPRs (image) / 63 (YUV), 106 SGPRs, no
// scratch, 50432 bytes of LDS, occupancy 3 waves a SIMD (LDS-bound); generic 48 / 62 VGPRs, 16640 bytes, 8 waves a SIMD.
// Banks (bank = dword address % 32, per 32-lane half; derived from the address maps.  Not measured: SQ_LDS_BANK_CONFLICT, whether byte
// writes of several lanes to one dword of the byte tile serialise, the byte load form's time, scales other than 1 / 2 and 80 / 150,
// image sources; profiles/oriented_resized_entry.md holds what was):
//   stage writes, vec    a lane's element t goes to dword 4q + t + const of one row: a half is 32 quads, stride 4 -> 8 banks, 4-way (as
//                        IM_ROWVEC's); the rows of one half are `pitch` apart, which only shifts the pattern
//   stage writes, bytes  a half writes 32 consecutive dwords of a row (or the end of one row and the start of the next, pitch apart):
//                        conflict-free, or 2-way where the two runs overlap mod 32
//   rz_pixel reads       one tap of 32 consecutive reduced x.  rot 0 / 2 (ax = +-1): the taps are 1 / scale dwords apart on average:
//                        scale 1 / 2: stride 2, 2-way; 1 / 4: stride 4, 4-way; 80 / 150: stride 1.875, 30 + distinct dwords over 60: at
//                        most 2-way; enlarging: neighbours share a dword (broadcast).  rot 1 / 3 (ax = +-pitch, odd): stride pitch / scale:
//                        an odd pitch times 2 (4): the same 2-way (4-way); fractional: as rot 0 / 2.  The mirror only changes signs.
//   byte tile            as k_ingest_resized
// GENERIC (k_ingest_oriented_resized_image_generic / _yuv_generic; STAGED = false; taken for rot 0 / 2, where its lanes run along the stored
// rows already and the stage was measured slower, and for scales under 1 / 4): k_ingest_resized's phase 1 with the orientation map in
// front of the global accessors (RzOrientedSrc over RzImageSrc / RzYuvSrc): every lane gathers its own pixels, any description, any scale;
// 16640 bytes of LDS.  Both forms run the same rz_pixel on the same bytes: identical bits.
// ------------------------------------------------------------------------
constexpr int OS_STAGE = 8448;  // dwords
constexpr int OS_MIN_BAND = 8;  // reduced rows

// The first and last source index that reduced indices d0 .. d1 of one axis read (y: rows, else columns), clipped to [0, ssize): the
// kernel's footprint and the host's band choice (orientedResizedBand) from the same tables.  lin: {sx, a0, a1, two} / {r0, r1, b0, b1};
// run: {first tap, count}; tap: {source index, weight}; is: RZ_AREA_INT's cell.
__host__ __device__ inline void rz_span(int mode, int is, int ssize, const int32_t* lin, const int32_t* run, const int32_t* tap, bool y, int d0, int d1, int& first,
    int& last)
{
    if (mode == RZ_LINEAR)
    {
        first = lin[4 * d0];
        last = y ? lin[4 * d1 + 1] : lin[4 * d1] + (lin[4 * d1 + 3] ? 1 : 0);
    }
    else if (mode == RZ_AREA_INT)
    {
        first = d0 * is;
        last = (d1 + 1) * is - 1;
    }
    else
    {
        first = tap[2 * run[2 * d0]];
        last = tap[2 * (run[2 * d1] + (run[2 * d1 + 1] > 0 ? run[2 * d1 + 1] - 1 : 0))];
    }
    first = first < 0 ? 0 : (first > ssize - 1 ? ssize - 1 : first);
    last = last > ssize - 1 ? ssize - 1 : (last < first ? first : last);
}

// rz_pixel's accessor on the stage: upright pixel (y, x) of U is the dword at base + y * ay + x * ax
struct RzStageSrc
{
    const uint32_t* st;
    int base, ay, ax;
    __device__ __forceinline__ void px(int y, int x, int (&v)[4]) const
    {
        const uint32_t w = st[base + y * ay + x * ax];
        v[0] = int(w & 255);
        v[1] = int((w >> 8) & 255);
        v[2] = int((w >> 16) & 255);
        v[3] = 0;
    }
};

// rz_pixel's global accessors behind the orientation map: upright pixel (y, x) of U is source pixel (rs, cs) of S
template <class IN>
struct RzOrientedSrc
{
    IN in;
    OrientSrc o;
    __device__ __forceinline__ void px(int y, int x, int (&v)[4]) const
    {
        const int p = o.swap ? x : y, q = o.swap ? y : x;
        in.px(o.revR ? o.Hs - 1 - p : p, o.revC ? o.Ws - 1 - q : q, v);
    }
};

struct OrientedResizedSrc
{
    ResizedSrc r;  // the description at Hs x Ws; the tap tables of U's size
    OrientSrc o;
    int band;      // STAGED: reduced rows a band
    int vec;       // STAGED: the wide load form
};

// n (1 .. 3) bytes at p as the low bytes of a dword
__device__ __forceinline__ uint32_t os_bytes(const uint8_t* p, int n)
{
    uint32_t v = 0;
    for (int b = 0; b < n; b++)
    {
        v |= uint32_t(p[b]) << (8 * b);
    }
    return v;
}

// STAGED load phase, an image of u8 elements: the rectangle T of frame `in` (element (0, 0, 0)) to the stage
__device__ __forceinline__ void os_stage_image(const ImageArgs& s, const uint8_t* in, const OrientTile& T, int Ws, int pitch, int vec, uint32_t* stage)
{
    const int nIn = s.nIn;
    if (vec)
    {
        // sx == 1; the base and sn, sc, sy are multiples of four (host-checked): every row start is
        const int q0 = T.cs0 >> 2, nq = ((T.cs0 + T.nsc - 1) >> 2) - q0 + 1;
#pragma unroll 2
        for (int idx = threadIdx.x; idx < T.nsr * nq; idx += 256)
        {
            const int i = idx / nq, col = 4 * (q0 + idx - i * nq);
            const uint8_t* rp = in + int64_t(T.rs0 + i) * s.sy + col;
            const bool whole = col + 4 <= Ws;
            uint32_t w[3] = { 0, 0, 0 };
#pragma unroll
            for (int c = 0; c < 3; c++)
            {
                if (c < nIn)
                {
                    const uint8_t* pc = rp + int64_t(c) * s.sc;
                    w[c] = whole ? *reinterpret_cast<const uint32_t*>(pc) : os_bytes(pc, Ws - col);
                }
            }
#pragma unroll
            for (int t = 0; t < 4; t++)
            {
                const int j = col + t - T.cs0;
                if (j >= 0 && j < T.nsc)
                {
                    stage[i * pitch + j] = ((w[0] >> (8 * t)) & 255) | (((w[1] >> (8 * t)) & 255) << 8) | (((w[2] >> (8 * t)) & 255) << 16);
                }
            }
        }
    }
    else
    {
#pragma unroll 2
        for (int idx = threadIdx.x; idx < T.nsr * T.nsc; idx += 256)
        {
            const int i = idx / T.nsc, j = idx - i * T.nsc;
            const uint8_t* p = in + int64_t(T.rs0 + i) * s.sy + int64_t(T.cs0 + j) * s.sx;
            uint32_t w = p[0];
            if (nIn == 3)
            {
                w |= (uint32_t(p[s.sc]) << 8) | (uint32_t(p[2 * s.sc]) << 16);
            }
            stage[i * pitch + j] = w;
        }
    }
}

// STAGED load phase, a YUV description: the rectangle T of frame n, converted once per source pixel, to the stage
template <bool CF>
__device__ __forceinline__ void os_stage_yuv(const YuvDescSrc& s, int64_t n, const OrientTile& T, int Ws, int pitch, int vec, uint32_t* stage)
{
    const uint8_t* fy = s.base + s.y.off + n * s.y.sn;
    const uint8_t* fu = s.base + s.u.off + n * s.u.sn;
    const uint8_t* fv = s.base + s.v.off + n * s.v.sn;
    const int subX = s.subX, subY = s.subY;
    if (vec)
    {
        // sp == 1; base + off, sr, sn of every plane are multiples of 4 (host-checked): every plane row start is
        const int cW = (Ws + subX) >> subX; // chroma samples a row
        const int q0 = T.cs0 >> 2, nq = ((T.cs0 + T.nsc - 1) >> 2) - q0 + 1;
#pragma unroll 2
        for (int idx = threadIdx.x; idx < T.nsr * nq; idx += 256)
        {
            const int i = idx / nq, col = 4 * (q0 + idx - i * nq), rs = T.rs0 + i, cr = rs >> subY;
            const uint8_t* yp = fy + int64_t(rs) * s.y.sr + col;
            const uint32_t Y = col + 4 <= Ws ? *reinterpret_cast<const uint32_t*>(yp) : os_bytes(yp, Ws - col);
            uint32_t U, V;
            if (subX)
            {
                const int cc = col >> 1; // even: the pair (cc, cc + 1) is 2-aligned
                const uint8_t* up = fu + int64_t(cr) * s.u.sr + cc;
                const uint8_t* vp = fv + int64_t(cr) * s.v.sr + cc;
                const bool whole = cc + 2 <= cW;
                U = whole ? uint32_t(*reinterpret_cast<const uint16_t*>(up)) : uint32_t(up[0]);
                V = whole ? uint32_t(*reinterpret_cast<const uint16_t*>(vp)) : uint32_t(vp[0]);
            }
            else
            {
                const uint8_t* up = fu + int64_t(cr) * s.u.sr + col;
                const uint8_t* vp = fv + int64_t(cr) * s.v.sr + col;
                const bool whole = col + 4 <= Ws;
                U = whole ? *reinterpret_cast<const uint32_t*>(up) : os_bytes(up, Ws - col);
                V = whole ? *reinterpret_cast<const uint32_t*>(vp) : os_bytes(vp, Ws - col);
            }
#pragma unroll
            for (int t = 0; t < 4; t++)
            {
                const int j = col + t - T.cs0;
                if (j >= 0 && j < T.nsc)
                {
                    const int ct = 8 * (t >> subX);
                    int r, g, b;
                    yuv_rgb<CF>(int((Y >> (8 * t)) & 255), yuv_chroma<CF>(int((U >> ct) & 255), int((V >> ct) & 255), s.k), s.k, r, g, b);
                    stage[i * pitch + j] = uint32_t(r) | (uint32_t(g) << 8) | (uint32_t(b) << 16);
                }
            }
        }
    }
    else
    {
#pragma unroll 2
        for (int idx = threadIdx.x; idx < T.nsr * T.nsc; idx += 256)
        {
            const int i = idx / T.nsc, j = idx - i * T.nsc, rs = T.rs0 + i, cs = T.cs0 + j;
            const int cr = rs >> subY, cc = cs >> subX;
            const int Y = fy[int64_t(rs) * s.y.sr + int64_t(cs) * s.y.sp];
            const int U = fu[int64_t(cr) * s.u.sr + int64_t(cc) * s.u.sp];
            const int V = fv[int64_t(cr) * s.v.sr + int64_t(cc) * s.v.sp];
            int r, g, b;
            yuv_rgb<CF>(Y, yuv_chroma<CF>(U, V, s.k), s.k, r, g, b);
            stage[i * pitch + j] = uint32_t(r) | (uint32_t(g) << 8) | (uint32_t(b) << 16);
        }
    }
}

template <int SRC, int MODE, bool STAGED>
__global__ void __launch_bounds__(256) k_ingest_oriented_resized(IngestArgs a, OrientedResizedSrc S)
{
    __shared__ uint32_t tileW[IG_T * IG_PITCH / 4];
    __shared__ uint32_t stage[STAGED ? OS_STAGE : 1];
    uint8_t* tile = reinterpret_cast<uint8_t*>(tileW);
    const ResizeTaps& tp = S.r.t; // of U: tp.rows x tp.cols
    const int x0 = blockIdx.x * IG_T, y0 = blockIdx.y * IG_T;
    const int nx = min(IG_T, a.W - x0), ny = min(IG_T, a.H - y0);
    const int64_t n = blockIdx.z;
    const int xx = threadIdx.x & 63;
    const int cn = SRC != RS_IMAGE ? 3 : S.r.im.nIn;
    if (!STAGED)
    {
        if (xx < nx)
        {
            const RzOrientedSrc<decltype(rz_global_src<SRC>(S.r, n))> src{ rz_global_src<SRC>(S.r, n), S.o };
            rz_fill_tile(src, tp, cn, x0, y0, xx, threadIdx.x >> 6, ny, tile);
        }
    }
    else
    {
        const int32_t* xlin = reinterpret_cast<const int32_t*>(tp.xlin);
        const int32_t* ylin = reinterpret_cast<const int32_t*>(tp.ylin);
        const int32_t* xrun = reinterpret_cast<const int32_t*>(tp.xrun);
        const int32_t* yrun = reinterpret_cast<const int32_t*>(tp.yrun);
        const int32_t* xtap = reinterpret_cast<const int32_t*>(tp.xtap);
        const int32_t* ytap = reinterpret_cast<const int32_t*>(tp.ytap);
        int fx0, fx1;
        rz_span(tp.mode, tp.isx, tp.cols, xlin, xrun, xtap, false, x0, x0 + nx - 1, fx0, fx1);
        for (int yb = 0; yb < ny; yb += S.band)
        {
            const int nb = min(S.band, ny - yb);
            int fy0, fy1;
            rz_span(tp.mode, tp.isy, tp.rows, ylin, yrun, ytap, true, y0 + yb, y0 + yb + nb - 1, fy0, fy1);
            const OrientTile T = orient_tile(S.o, fx0, fy0, fx1 - fx0 + 1, fy1 - fy0 + 1);
            const int pitch = T.nsc | 1;
            if (yb)
            {
                __syncthreads(); // the band before is read
            }
            if (SRC != RS_IMAGE)
            {
                os_stage_yuv<SRC == RS_YUV_CF>(S.r.yuv, n, T, S.o.Ws, pitch, S.vec, stage);
            }
            else
            {
                os_stage_image(S.r.im, static_cast<const uint8_t*>(S.r.im.in) + n * S.r.im.sn, T, S.o.Ws, pitch, S.vec, stage);
            }
            __syncthreads();
            // rectangle element (i, j) of upright (y, x): p = (swap ? x - fx0 : y - fy0), q = the other; i = revR ? nsr - 1 - p : p, j likewise
            const int sR = T.revR ? -1 : 1, sC = T.revC ? -1 : 1;
            const int pOff = T.swap ? fx0 : fy0, qOff = T.swap ? fy0 : fx0;
            const int base = ((T.revR ? T.nsr - 1 : 0) - sR * pOff) * pitch + (T.revC ? T.nsc - 1 : 0) - sC * qOff;
            const RzStageSrc src{ stage, base, T.swap ? sC : sR * pitch, T.swap ? sR * pitch : sC };
            if (xx < nx)
            {
                rz_fill_tile(src, tp, cn, x0, y0, xx, yb + (threadIdx.x >> 6), yb + nb, tile);
            }
        }
    }
    __syncthreads();
    ingest_store_tile<MODE>(a, tile, 3, 0, 1, 2, x0, y0, nx, ny);
}

// ------------------------------------------------------------------------
// convTri1 with the pyramid's in-place aliasing (toolbox/convConst.cpp:445-525;
// chnsCompute.cpp:239, chnsPyramid.cpp:404).
//
// Because source and destination are the same buffer in the reference, the
// x tap of column i reads the OUTPUT of column i-1:
//     T_i[y] = nrm*((O_{i-1}[y] + p*I_i[y]) + I_{i+1}[y])      (O_{-1} := I_0)
//     O_i[y] = (T_i[y-1] + p*T_i[y]) + T_i[y+1]                (edges: (1+p)*T)
// a recursion along image-x with a 3-tap exchange along image-y every step.
// It cannot be tiled along x without changing bits, so one workgroup owns a
// whole plane: threads run along y (R interleaved rows each), the previous
// output column stays in registers (the kernel is out-of-place: it never
// re-reads what it wrote), and the y exchange goes through a double-buffered
// LDS column with one barrier per image column.
// ------------------------------------------------------------------------
struct SmoothJob
{
    int32_t h, w, nplanes, out_cs; // out_cs: destination column stride (hP)
    int64_t in_off, out_off;       // float offsets inside a frame's source / destination buffer
    int64_t in_ps, out_ps;         // plane strides
};

// Columns are loaded SM_CH at a time, one whole chunk ahead of the chunk being
// filtered, into two register sets that swap roles (main loop unrolled over two
// chunks: no copies).  The main loop is straight-line code: row and column indices
// are clamped instead of guarded and rows beyond the plane store to a dump slot,
// because vmcnt completes in order and the compiler only keeps the next chunk's loads
// in flight across a column step when it sees no branch between them.
#define SM_CH 8

template <int R, bool ALIASED>
__global__ void __launch_bounds__(1024) k_smooth_tri1(const float* __restrict__ in, float* __restrict__ out,
    const SmoothJob* __restrict__ jobs, int64_t in_fs, int64_t out_fs, float p, int ldsStride, float* __restrict__ dump)
{
    extern __shared__ float lds[]; // 2 * ldsStride floats
    const SmoothJob job = jobs[blockIdx.y];
    if ((int)blockIdx.x >= job.nplanes)
    {
        return;
    }
    const int h = job.h, w = job.w;
    const float* __restrict__ I = in + int64_t(blockIdx.z) * in_fs + job.in_off + int64_t(blockIdx.x) * job.in_ps;
    float* __restrict__ O = out + int64_t(blockIdx.z) * out_fs + job.out_off + int64_t(blockIdx.x) * job.out_ps;
    const int tid = threadIdx.x, nt = blockDim.x;
    const float nrm = 1.0f / ((p + 2) * (p + 2));
    const float p1 = 1 + p;
    int yk[R], ym[R], yp[R]; // this thread's rows (clamped) and their neighbours
    bool ok[R];
#pragma unroll
    for (int k = 0; k < R; k++)
    {
        const int y = tid + k * nt;
        ok[k] = y < h;
        yk[k] = min(y, h - 1);
        ym[k] = max(yk[k] - 1, 0);
        yp[k] = min(yk[k] + 1, h - 1);
    }
    float c0[SM_CH][R], c1[SM_CH][R], prev[R], lastIn[R];
#define SM_LOAD(BUF, I0)                                                          \
    _Pragma("unroll") for (int j = 0; j < SM_CH; j++)                             \
    {                                                                             \
        const float* __restrict__ col = I + int64_t(min((I0) + j, w - 1)) * h;    \
        _Pragma("unroll") for (int k = 0; k < R; k++)                             \
        {                                                                         \
            BUF[j][k] = col[yk[k]];                                               \
        }                                                                         \
    }
    // one column: CUR = column i, NXT = column i+1 (already clamped to w-1 by the loads)
#define SM_COL(I_, CUR, NXT)                                                      \
    {                                                                             \
        const int i_ = (I_);                                                      \
        float* Tb = lds + (i_ & 1) * ldsStride;                                   \
        float T[R];                                                               \
        _Pragma("unroll") for (int k = 0; k < R; k++)                             \
        {                                                                         \
            const float Im = CUR[k];                                              \
            const float Ir = NXT[k]; /* column min(i+1, w-1): Ir = Im at the last column (:508-512) */ \
            const float Il = ALIASED ? ((i_ == 0) ? Im : prev[k]) : ((i_ == 0) ? Im : lastIn[k]);     \
            T[k] = nrm * (Il + p * Im + Ir);                                      \
            lastIn[k] = Im;                                                       \
            Tb[yk[k]] = T[k]; /* rows beyond the plane rewrite row h-1 with its own value */          \
        }                                                                         \
        __syncthreads();                                                          \
        float* __restrict__ oc = O + int64_t(i_) * job.out_cs;                    \
        _Pragma("unroll") for (int k = 0; k < R; k++)                             \
        {                                                                         \
            const float tm = Tb[ym[k]], tp = Tb[yp[k]];                           \
            const float mid = tm + p * T[k] + tp;                                 \
            const float top = p1 * T[k] + tp;                                     \
            const float bot = tm + p1 * T[k];                                     \
            const float o = (yk[k] == 0) ? top : ((yk[k] == h - 1) ? bot : mid);  \
            prev[k] = o;                                                          \
            float* __restrict__ dst = ok[k] ? (oc + yk[k]) : (dump + (tid & 63)); \
            *dst = o;                                                             \
        }                                                                         \
    }
#pragma unroll
    for (int k = 0; k < R; k++)
    {
        prev[k] = lastIn[k] = 0.f;
    }
    SM_LOAD(c0, 0);
    int i = 0;
    // main loop: two full chunks per iteration; needs columns i .. i + 2*SM_CH (the lookahead column is clamped)
    for (; i + 2 * SM_CH <= w; i += 2 * SM_CH)
    {
        SM_LOAD(c1, i + SM_CH);
#pragma unroll
        for (int j = 0; j < SM_CH; j++)
        {
            if (j < SM_CH - 1)
            {
                SM_COL(i + j, c0[j], c0[j + 1]);
            }
            else
            {
                SM_COL(i + j, c0[j], c1[0]);
            }
        }
        SM_LOAD(c0, i + 2 * SM_CH);
#pragma unroll
        for (int j = 0; j < SM_CH; j++)
        {
            if (j < SM_CH - 1)
            {
                SM_COL(i + SM_CH + j, c1[j], c1[j + 1]);
            }
            else
            {
                SM_COL(i + SM_CH + j, c1[j], c0[0]);
            }
        }
    }
    // tail: fewer than 2*SM_CH columns left; c0 holds columns i .. i+SM_CH-1 (clamped)
    if (i < w)
    {
        SM_LOAD(c1, i + SM_CH);
#pragma unroll
        for (int j = 0; j < SM_CH; j++)
        {
            if (i + j < w) // uniform
            {
                if (j < SM_CH - 1)
                {
                    SM_COL(i + j, c0[j], c0[j + 1]);
                }
                else
                {
                    SM_COL(i + j, c0[j], c1[0]);
                }
            }
        }
#pragma unroll
        for (int j = 0; j < SM_CH; j++)
        {
            if (i + SM_CH + j < w) // uniform
            {
                if (j < SM_CH - 1)
                {
                    SM_COL(i + SM_CH + j, c1[j], c1[j + 1]);
                }
                else
                {
                    SM_COL(i + SM_CH + j, c1[j], c1[j]);
                }
            }
        }
    }
#undef SM_LOAD
#undef SM_COL
}

} // namespace acfhip
