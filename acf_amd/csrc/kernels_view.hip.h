// kernels_view.hip.h — affine views of the stored frame (acf_hip_pyramid_view / acf_hip_run_view; the header's "affine views of the
// stored frame" section is the definition): k_ingest_view makes frame i of the batch the view views[i] of stored frame frames[i] —
// tilted, magnified, reduced, cut out — straight from the frame as the descriptor, the format and the orientation code describe it,
// and ends in the store phase of every ingest kernel (ingest_store_phase: float4 a plane along image-y, the model's colour conversion
// in registers).  No reference counterpart: the sampling rule is this library's own, cut_crops' bilinear rule under an affine map,
// every operation an f32 operation rounded once (the build has -ffp-contract=off), so that a numpy restatement gives the same bits
// (tests/view_ref.py).
//
// Grid (tiles x, tiles y, views), 256 lanes, a workgroup a 64 x 64 tile of the view's frame (the ingest kernels' tile: the store phase
// is theirs).  Everything a workgroup decides (the view, the frame, the form, the rectangle) depends on blockIdx alone: uniform.  Two
// forms, chosen per tile by view_form (= acf_hip_view_form), same bits:
//   staged   the clamped coordinates of the tile's four corner samples span a rectangle of U (an affine coordinate is monotone in
//            each of the two sample indices, every step of view_coord being monotone under round-to-nearest, so its extremes over
//            the tile lie at the corners); widened by one pixel before and two behind (the 2 x 2 neighbourhood and a pixel of
//            slack) and clamped to U it is the rectangle orient_tile gives of the stored frame; that is loaded once, lanes along the
//            STORED rows whatever the turn, through the source's accessor (YUV converted once per stored pixel) into LDS as code
//            values (u8, u16 or the f32 bits), one plane a channel, and sampled from there.  Coefficients that overflow or hold NaN
//            break the monotony, so NO LDS index is formed from an unchecked coordinate: a sample whose 2 x 2 neighbourhood is not
//            wholly inside the rectangle fetches through the accessor like a gather.
//   gather   every sample fetches its four neighbours through the accessor: when the rectangle holds more than four stored pixels a
//            sample (strong reductions: the stage would load more than the gathers do) or does not fit the stage (wide codes under a
//            tilt, three f32 channels).
// The accessors, CutKind and the clamping are k_cut_crops' (kernels_cut.hip.h): only pixels inside [0, Hs) x [0, Ws) are addressed,
// the coordinate is clamped before it becomes an index (NaN becomes 0) and the index once more, so no bit pattern of a view makes a
// load leave the description's extent.  A frame index outside [0, n_frames) reads nothing: the frame of all-zero code values.
//
// LDS: VIEW_LDS_BYTES = 32 KiB a workgroup and nothing else (the store phase samples straight from the stage: there is no tile of
// converted pixels as in the other ingest kernels, which hold ~17 KB), so five workgroups (20 waves) a CU by LDS of the CU's 160 KiB.
// The kernel waits on memory in the load phase and in the gathers and on LDS latency in the sampler, so resident waves are what hides
// it (k_cut_crops' argument).  32 KiB holds the 67 x 67 rectangle of an upright tile of every source but three f32 channels
// (3 x 67 x 67 x 4 = 54 KB: always gathered), an RGB byte tile at any tilt (45 degrees: 94 x 94 x 3 = 26.5 KB) and at reductions up
// to ~1.5 (99 x 99 x 3 = 29.4 KB; at 2 the four-pixels rule gathers anyway), 16-bit video upright (27 KB) but not tilted beyond a
// few degrees.  A smaller tile would stage more of those, but the tile is the store phase's: 64 image-y a column are what makes
// its float4 stores whole 256-byte runs.  Layout [C][rows][pitch] code values, pitch = the rectangle's width made odd.  Banks
// (derived from the address maps with the bank rule — narrow reads: (a / 4) % 32, per 32-lane half —; SQ_LDS_BANK_CONFLICT was not
// read): a half-wave of the store phase holds 16 row quads (rows 4 apart) of two adjacent columns.  Upright byte codes: rows 4 apart
// are `pitch` dwords apart, odd, so the 16 quads fall on 16 banks and the second column on the same dwords or their neighbours: 2-way
// at worst.  Upright f32 codes: 4 x pitch dwords apart = 4 (mod 8): 16 quads on 8 banks, 2-way.  Under a tilt the map is the view's.
// The loaders of a quarter turn write down a column, pitch elements apart — odd, so consecutive lanes fall on different banks for
// f32 codes and share a dword at most pairwise for narrow ones.
#pragma once

namespace acfhip
{

constexpr int VIEW_LDS_BYTES = 32 * 1024;

// the second argument of k_ingest_view: the stored frames (CutSource: either family), the views and what they read
struct ViewSrc
{
    CutSource S;
    const float* views;    // [n][6]
    const int32_t* frames; // [n], or null: view i reads stored frame i
    int nFrames;
    OrientSrc o;
    int Hu, Wu, C, s;
    float unit;
};

// One view's sampling grid
struct ViewGrid
{
    float m[6];
    int Hu, Wu, s;
    float inv;  // float(1.0 / s)
    float norm; // float(1.0 / (s * s))
};

__host__ __device__ inline ViewGrid view_grid(const float* m, int s, int Hu, int Wu)
{
    ViewGrid g;
    for (int k = 0; k < 6; k++)
    {
        g.m[k] = m[k];
    }
    g.Hu = Hu;
    g.Wu = Wu;
    g.s = s;
    g.inv = float(1.0 / double(s));
    g.norm = float(1.0 / double(s * s));
    return g;
}
// the position of sample i of pixel k along an axis of the view's frame
__host__ __device__ inline float view_pos(int k, int s, int i, float inv)
{
    return (float(k * s + i) + 0.5f) * inv;
}
// clamped into the frame (border replication); NaN becomes 0
__host__ __device__ inline float view_clamp(float u, int n)
{
    const float hi = float(n - 1);
    u = u > 0.f ? u : 0.f;
    return u < hi ? u : hi;
}
// the clamped coordinates in U of position (px, py) of the view's frame
__host__ __device__ inline void view_coord(const ViewGrid& g, float px, float py, float& u, float& v)
{
    u = view_clamp((((g.m[0] * px) + (g.m[1] * py)) + g.m[2]) - 0.5f, g.Wu);
    v = view_clamp((((g.m[3] * px) + (g.m[4] * py)) + g.m[5]) - 0.5f, g.Hu);
}

// The rectangle of U a tile of nx x ny pixels at (x0, y0) stages: columns cLo .. cHi, rows rLo .. rHi
struct ViewRect
{
    int cLo, cHi, rLo, rHi;
};
__host__ __device__ inline ViewRect view_rect(const ViewGrid& g, int x0, int y0, int nx, int ny)
{
    const float pxs[2] = { view_pos(x0, g.s, 0, g.inv), view_pos(x0 + nx - 1, g.s, g.s - 1, g.inv) };
    const float pys[2] = { view_pos(y0, g.s, 0, g.inv), view_pos(y0 + ny - 1, g.s, g.s - 1, g.inv) };
    int cLo = g.Wu - 1, cHi = 0, rLo = g.Hu - 1, rHi = 0;
    for (int k = 0; k < 4; k++)
    {
        float u, v;
        view_coord(g, pxs[k & 1], pys[k >> 1], u, v);
        const int c = cut_floor(u, g.Wu), r = cut_floor(v, g.Hu);
        cLo = c < cLo ? c : cLo;
        cHi = c > cHi ? c : cHi;
        rLo = r < rLo ? r : rLo;
        rHi = r > rHi ? r : rHi;
    }
    ViewRect R;
    R.cLo = cLo > 0 ? cLo - 1 : 0;
    R.rLo = rLo > 0 ? rLo - 1 : 0;
    R.cHi = cHi + 2 < g.Wu ? cHi + 2 : g.Wu - 1;
    R.rHi = rHi + 2 < g.Hu ? rHi + 2 : g.Hu - 1;
    return R;
}
// acf_hip_view_form: 0 staged, 1 gather.  Gather when the tile's rectangle holds more than four stored pixels a sample (a sample
// fetches four: beyond that the stage would load more than the gathers do) or does not fit the stage.
__host__ __device__ inline int view_form(const ViewGrid& g, const ViewRect& R, int nx, int ny, int C, int sampleBytes)
{
    const int fw = R.cHi - R.cLo + 1, fh = R.rHi - R.rLo + 1;
    if (int64_t(fw) * fh > 4 * int64_t(nx * g.s) * (ny * g.s))
    {
        return 1;
    }
    return int64_t(cut_pitch(fw)) * fh * C * sampleBytes > VIEW_LDS_BYTES ? 1 : 0;
}

// One pixel (r, c) of the view's frame, every channel: the ONE statement of the sampling rule, for both forms.  fetch(r0, r1, c0, c1, p)
// yields the exact floats of the four upright pixels p[0] = (r0, c0), p[1] = (r0, c1), p[2] = (r1, c0), p[3] = (r1, c1).
template <class FETCH>
__device__ __forceinline__ void view_pixel(const ViewGrid& g, int r, int c, FETCH&& fetch, float (&val)[3])
{
    float acc[3] = { 0.f, 0.f, 0.f };
    for (int a = 0; a < g.s; a++)
    {
        const float py = view_pos(r, g.s, a, g.inv);
        for (int b = 0; b < g.s; b++)
        {
            const float px = view_pos(c, g.s, b, g.inv);
            float u, v;
            view_coord(g, px, py, u, v);
            const int c0 = cut_floor(u, g.Wu), c1 = min(c0 + 1, g.Wu - 1);
            const int r0 = cut_floor(v, g.Hu), r1 = min(r0 + 1, g.Hu - 1);
            const float fx = u - float(c0), fy = v - float(r0);
            float p[4][3];
            fetch(r0, r1, c0, c1, p);
#pragma unroll
            for (int k = 0; k < 3; k++)
            {
                const float top = p[0][k] + fx * (p[1][k] - p[0][k]);
                const float bot = p[2][k] + fx * (p[3][k] - p[2][k]);
                acc[k] = acc[k] + (top + fy * (bot - top));
            }
        }
    }
#pragma unroll
    for (int k = 0; k < 3; k++)
    {
        val[k] = acc[k] * g.norm;
    }
}

template <int KIND, int MODE>
__global__ void __launch_bounds__(256) k_ingest_view(IngestArgs a, ViewSrc V)
{
    using K = CutKind<KIND>;
    using code_t = typename K::code_t;
    __shared__ uint32_t stageW[VIEW_LDS_BYTES / 4];
    code_t* stage = reinterpret_cast<code_t*>(stageW);
    const int x0 = blockIdx.x * IG_T, y0 = blockIdx.y * IG_T;
    const int nx = min(IG_T, a.W - x0), ny = min(IG_T, a.H - y0);
    const int n = blockIdx.z;
    const int f = V.frames ? V.frames[n] : n;
    if (f < 0 || f >= V.nFrames) // reads nothing: the frame of all-zero code values
    {
        ingest_store_phase<MODE>(a, x0, y0, nx, ny, [&](int, int, int, float& r, float& g, float& b) { r = g = b = 0.f; });
        return;
    }
    const ViewGrid g = view_grid(V.views + int64_t(n) * 6, V.s, V.Hu, V.Wu);
    const ViewRect R = view_rect(g, x0, y0, nx, ny);
    const bool staged = view_form(g, R, nx, ny, V.C, int(sizeof(code_t))) == 0;
    const auto src = K::at(V.S, f);
    const OrientSrc o = V.o;
    const int nC = V.C;
    const float unit = V.unit;
    const int fw = R.cHi - R.cLo + 1, fh = R.rHi - R.rLo + 1, pitch = cut_pitch(fw), plane = fh * pitch;
    if (staged)
    {
        const OrientTile T = orient_tile(o, R.cLo, R.rLo, fw, fh);
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
                if (k < nC)
                {
                    at[k * plane] = code_t(v[k]);
                }
            }
        }
        __syncthreads();
    }
    const auto one = [&](int r, int c, float(&p)[3]) {
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
    const auto fetch = [&](int r0, int r1, int c0, int c1, float(&p)[4][3]) {
        if (staged && r0 >= R.rLo && r1 <= R.rHi && c0 >= R.cLo && c1 <= R.cHi)
        {
            const int t0 = (r0 - R.rLo) * pitch, t1 = (r1 - R.rLo) * pitch, d0 = c0 - R.cLo, d1 = c1 - R.cLo; // (all inside the stage: checked above)
#pragma unroll
            for (int k = 0; k < 3; k++)
            {
                const bool in = k < nC;
                const code_t* pl = stage + (in ? k : 0) * plane;
                p[0][k] = in ? K::val(pl[t0 + d0]) : 0.f;
                p[1][k] = in ? K::val(pl[t0 + d1]) : 0.f;
                p[2][k] = in ? K::val(pl[t1 + d0]) : 0.f;
                p[3][k] = in ? K::val(pl[t1 + d1]) : 0.f;
            }
            return;
        }
        one(r0, c0, p[0]);
        one(r0, c1, p[1]);
        one(r1, c0, p[2]);
        one(r1, c1, p[3]);
    };
    ingest_store_phase<MODE>(a, x0, y0, nx, ny, [&](int xx, int yq, int j, float& r, float& gg, float& b) {
        if (yq + j >= ny) // (a row beyond the tile: converted, never stored)
        {
            r = gg = b = 0.f;
            return;
        }
        float val[3];
        view_pixel(g, y0 + yq + j, x0 + xx, fetch, val);
        r = val[0] * unit;
        gg = nC == 3 ? val[1] * unit : r;
        b = nC == 3 ? val[2] * unit : r;
    });
}

} // namespace acfhip
