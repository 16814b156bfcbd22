// kernels_merge.hip.h — part of kernels.hip.h (included from there, in its order, and nowhere else).
// The detections of a batch of views merged into their stored frames on the device (the header's "merging the views' detections"
// section): every detection mapped into the upright stored frame U by its view, then k_nms's rule ACROSS the views of one stored frame.
#pragma once

namespace acfhip
{

// ---- the views' box arithmetic, host and device alike (acf_hip_view_quad / acf_hip_view_box): the corners in double from the float view
// and the int box, every operation rounded once
__host__ __device__ inline void view_corner(const float* m, int x, int y, int w, int h, int k, double (&p)[2]) // k: TL, TR, BR, BL
{
    const double x0 = x, y0 = y, x1 = double(x) + w, y1 = double(y) + h;
    const double px = (k == 1 || k == 2) ? x1 : x0, py = k >= 2 ? y1 : y0;
    p[0] = double(m[0]) * px + double(m[1]) * py + double(m[2]);
    p[1] = double(m[3]) * px + double(m[4]) * py + double(m[5]);
}
__host__ __device__ inline void view_quad_of(const float* m, int x, int y, int w, int h, float (&quad)[8])
{
    for (int k = 0; k < 4; k++)
    {
        double p[2];
        view_corner(m, x, y, w, h, k, p);
        quad[2 * k] = float(p[0]);
        quad[2 * k + 1] = float(p[1]);
    }
}
// (the box's extent is the difference of the unrounded extremes)
__host__ __device__ inline void view_box_of(const float* m, int x, int y, int w, int h, float (&box)[4])
{
    double lo[2] = { 0, 0 }, hi[2] = { 0, 0 };
    for (int k = 0; k < 4; k++)
    {
        double p[2];
        view_corner(m, x, y, w, h, k, p);
        for (int d = 0; d < 2; d++)
        {
            lo[d] = k == 0 || p[d] < lo[d] ? p[d] : lo[d];
            hi[d] = k == 0 || p[d] > hi[d] ? p[d] : hi[d];
        }
    }
    box[0] = float(lo[0]);
    box[1] = float(lo[1]);
    box[2] = float(hi[0] - lo[0]);
    box[3] = float(hi[1] - lo[1]);
}

// ------------------------------------------------------------------------
// k_merge_views: one workgroup per stored frame f.
//   0. the counts of the views of f (ascending view) are prefix-summed into off[0 .. nViews] in LDS; a concatenated index finds its
//      (view, index) by binary search there.  A contributing view with a count < 0 or > maxHits, or a total above NMS_CAP, makes the
//      frame unknowable: count -1, no record;
//   1. every entry is mapped (view_box_of); one whose box has a non-finite member or not (w > 0 and h > 0) is dropped.  type 0: the rest
//      in concatenation order.  Else k_nms's rule on the float boxes, every box term in f64: keys (scores below thr dropped), bitonic
//      sort of {orderable f64 key, concatenated index}, boxes in sorted order, sequential-outer / parallel-inner suppression,
//      compaction, prune;
//   2. the first min(S, K) survivors are written as records, quads and grown boxes; EVERY other slot of boxesOut / framesOut gets
//      zeros / -1, so that k_cut_crops may read all K slots of every frame at once.
// LDS: k_nms's 58 KB (float4 boxes in the int4's place) + the offsets — a block still starts beside a resident cascade tile workgroup.
// The box of an entry is recomputed from its detection and its view where it is needed, not stored twice.
// ------------------------------------------------------------------------
constexpr int MERGE_VIEWS_MAX = 1024;

struct MergeArgs
{
    const acf_hip_detection* dets; // [nViews][maxHits]
    const int32_t* counts;         // [nViews]
    int32_t maxHits;
    const float* views;            // [nViews][6]
    const int32_t* frame;          // [nViews], or null: view i belongs to frame i
    int32_t nViews, nFrames;
    int32_t type, ovrUnion, doPrune, maxCount;
    double overlap, thr, pruneRatio;
    int32_t K;
    float grow;
    acf_hip_merged_detection* out; // [nFrames][K]
    int32_t* countsOut;            // [nFrames]
    float* boxesOut;               // [nFrames][K][4], or null
    int32_t* framesOut;            // [nFrames][K], or null
    float* quadsOut;               // [nFrames][K][8], or null
};

__global__ void __launch_bounds__(1024) k_merge_views(MergeArgs a)
{
    extern __shared__ __align__(16) unsigned long long mrg_lds[]; // (the float4 boxes: 16 bytes whatever static LDS lies in front)
    unsigned long long* key = mrg_lds;                                  // [NMS_CAP]
    float4* box = reinterpret_cast<float4*>(key + NMS_CAP);             // [NMS_CAP] {x, y, w, h} in sorted order
    uint32_t* idx = reinterpret_cast<uint32_t*>(box + NMS_CAP);         // [NMS_CAP]
    uint8_t* kp = reinterpret_cast<uint8_t*>(idx + NMS_CAP);            // [NMS_CAP]
    __shared__ int s_off[MERGE_VIEWS_MAX + 1];
    __shared__ int s_drop, s_wave[16], s_cut, s_bad;
    const int frame = blockIdx.x, tid = threadIdx.x;
    const int lane = tid & 63, wv = tid >> 6;
    const int K = a.K;
    // ---- 0. the offsets: thread v holds view v's count
    if (tid == 0)
    {
        s_drop = 0;
        s_cut = 0x7fffffff;
        s_bad = 0;
    }
    if (tid < 16)
    {
        s_wave[tid] = 0;
    }
    __syncthreads();
    int cnt = 0;
    if (tid < a.nViews && (a.frame ? a.frame[tid] : tid) == frame)
    {
        const int c = a.counts[tid];
        if (c < 0 || c > a.maxHits)
        {
            s_bad = 1;
        }
        else
        {
            cnt = min(c, NMS_CAP + 1); // (so that the sum cannot wrap: 1024 views of at most NMS_CAP + 1)
        }
    }
    {
        int incl = cnt;
#pragma unroll
        for (int d = 1; d < 64; d <<= 1)
        {
            const int v = __shfl_up(incl, d);
            incl += (lane >= d) ? v : 0;
        }
        if (lane == 63)
        {
            s_wave[wv] = incl;
        }
        __syncthreads();
        int base = 0;
        for (int q = 0; q < 16; q++)
        {
            base += (q < wv) ? s_wave[q] : 0;
        }
        if (tid < a.nViews)
        {
            s_off[tid + 1] = base + incl;
        }
        if (tid == 0)
        {
            s_off[0] = 0;
        }
    }
    __syncthreads();
    const int n = s_off[a.nViews];
    const bool unknowable = s_bad || n > NMS_CAP;
    acf_hip_merged_detection* __restrict__ O = a.out + int64_t(frame) * K;
    float* __restrict__ BO = a.boxesOut ? a.boxesOut + int64_t(frame) * K * 4 : nullptr;
    int32_t* __restrict__ FO = a.framesOut ? a.framesOut + int64_t(frame) * K : nullptr;
    float* __restrict__ QO = a.quadsOut ? a.quadsOut + int64_t(frame) * K * 8 : nullptr;
    if (unknowable)
    {
        for (int i = tid; i < K; i += 1024)
        {
            if (BO)
            {
                BO[4 * i] = BO[4 * i + 1] = BO[4 * i + 2] = BO[4 * i + 3] = 0.f;
            }
            if (FO)
            {
                FO[i] = -1;
            }
        }
        if (tid == 0)
        {
            a.countsOut[frame] = -1;
        }
        return;
    }
    int P = 1;
    while (P < n)
    {
        P <<= 1;
    }
    // as in k_nms: the waves the sort does not need leave before its barriers
    const int T = min(1024, max(64, P >> 1));
    if (tid >= T)
    {
        return;
    }
    if (tid < 16)
    {
        s_wave[tid] = 0; // (read by every wave above; the waves that stay have passed the barrier behind those reads)
    }
    const bool sorted = a.type != 0;
    // ---- 1. keys (dropped and padding entries sort last); type 0: the validity flags in concatenation order
    for (int i = tid; i < P; i += T)
    {
        unsigned long long k = 0ull;
        uint32_t ix = 0xffffffffu;
        bool ok = false;
        if (i < n)
        {
            const int v = nms_list_of(s_off, a.nViews, i);
            const acf_hip_detection d = a.dets[int64_t(v) * a.maxHits + (i - s_off[v])];
            float b[4];
            view_box_of(a.views + 6 * v, d.x, d.y, d.w, d.h, b);
            ok = cut_box_ok(b[0], b[1], b[2], b[3]);
            if (sorted && ok && double(d.score) < a.thr)
            {
                ok = false;
            }
            if (!ok)
            {
                atomicAdd(&s_drop, 1);
            }
            else
            {
                k = nms_key(double(d.score));
                k = k ? k : 1ull;
                ix = uint32_t(i);
            }
        }
        if (sorted)
        {
            key[i] = k;
            idx[i] = ix;
        }
        else if (i < n)
        {
            idx[i] = uint32_t(i);
            kp[i] = ok ? 1 : 0;
        }
    }
    __syncthreads();
    const int m = sorted ? n - s_drop : n;
    if (sorted)
    {
        // ---- 2. bitonic sort, "before" = larger key, then smaller concatenated index (view, then index)
        nms_sort(key, idx, P, T, tid);
        // ---- boxes in sorted order
        for (int i = tid; i < m; i += T)
        {
            const int q = int(idx[i]);
            const int v = nms_list_of(s_off, a.nViews, q);
            const acf_hip_detection d = a.dets[int64_t(v) * a.maxHits + (q - s_off[v])];
            float b[4];
            view_box_of(a.views + 6 * v, d.x, d.y, d.w, d.h, b);
            box[i] = make_float4(b[0], b[1], b[2], b[3]);
            kp[i] = 1;
        }
        __syncthreads();
        // ---- 3. suppression, every term in f64
        for (int i = 0; i + 1 < m; i++)
        {
            if (a.type == 2 && !kp[i]) // uniform: every thread reads the same byte
            {
                continue;
            }
            const float4 bi = box[i];
            const double xsI = bi.x, xeI = double(bi.x) + double(bi.z), ysI = bi.y, yeI = double(bi.y) + double(bi.w);
            const double asI = double(bi.z) * double(bi.w);
            for (int j = i + 1 + tid; j < m; j += T)
            {
                if (!kp[j])
                {
                    continue;
                }
                const float4 bj = box[j];
                const double xsJ = bj.x, xeJ = double(bj.x) + double(bj.z), ysJ = bj.y, yeJ = double(bj.y) + double(bj.w);
                const double iw = (xeI < xeJ ? xeI : xeJ) - (xsI > xsJ ? xsI : xsJ);
                const double ih = (yeI < yeJ ? yeI : yeJ) - (ysI > ysJ ? ysI : ysJ);
                if (!(iw > 0 && ih > 0))
                {
                    continue;
                }
                const double asJ = double(bj.z) * double(bj.w);
                double o = iw * ih;
                const double u = a.ovrUnion ? ((asI + asJ) - o) : (asI < asJ ? asI : asJ);
                o /= u;
                if (o > a.overlap)
                {
                    kp[j] = 0;
                }
            }
            __syncthreads();
        }
    }
    // ---- 4. survivors in order (the keys are dead: reused as [total] concatenated indices in output order), then prune
    uint32_t* outIdx = reinterpret_cast<uint32_t*>(key);
    const int total = nms_compact(kp, idx, m, tid, s_wave, outIdx);
    int finalCount = total;
    if (sorted && a.doPrune && total > 1)
    {
        finalCount = nms_prune(outIdx, total, a.maxCount, a.pruneRatio, tid, T, &s_cut, [&](uint32_t q) {
            const int v = nms_list_of(s_off, a.nViews, int(q));
            return double(a.dets[int64_t(v) * a.maxHits + (int(q) - s_off[v])].score);
        });
    }
    // ---- 5. the K slots of the frame
    const int nOut = min(finalCount, K);
    for (int i = tid; i < K; i += T)
    {
        float gb[4] = { 0.f, 0.f, 0.f, 0.f };
        if (i < nOut)
        {
            const int q = int(outIdx[i]);
            const int v = nms_list_of(s_off, a.nViews, q);
            const int at = q - s_off[v];
            const acf_hip_detection d = a.dets[int64_t(v) * a.maxHits + at];
            const float* mv = a.views + 6 * v;
            float b[4];
            view_box_of(mv, d.x, d.y, d.w, d.h, b);
            acf_hip_merged_detection r;
            r.x = b[0];
            r.y = b[1];
            r.w = b[2];
            r.h = b[3];
            r.score = d.score;
            r.view = v;
            r.index = at;
            r.scale = d.scale;
            O[i] = r;
            if (QO)
            {
                float qd[8];
                view_quad_of(mv, d.x, d.y, d.w, d.h, qd);
#pragma unroll
                for (int k = 0; k < 8; k++)
                {
                    QO[8 * i + k] = qd[k];
                }
            }
            // acf_hip_crop_box's f32 steps on the float box
            const float cx = b[0] + b[2] * 0.5f, cy = b[1] + b[3] * 0.5f;
            const float w2 = b[2] * a.grow, h2 = b[3] * a.grow;
            gb[0] = cx - w2 * 0.5f;
            gb[1] = cy - h2 * 0.5f;
            gb[2] = w2;
            gb[3] = h2;
        }
        if (BO)
        {
            BO[4 * i] = gb[0];
            BO[4 * i + 1] = gb[1];
            BO[4 * i + 2] = gb[2];
            BO[4 * i + 3] = gb[3];
        }
        if (FO)
        {
            FO[i] = i < nOut ? frame : -1;
        }
    }
    if (tid == 0)
    {
        a.countsOut[frame] = finalCount;
    }
}

} // namespace acfhip
