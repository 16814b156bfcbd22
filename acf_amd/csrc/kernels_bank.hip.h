// kernels_bank.hip.h — part of kernels.hip.h (included from there, in its order, and nowhere else).
// The lists of a bank of classifiers joined per frame on the device (the header's "a bank of classifiers" section): model 0's raw list
// and the members' lists of one frame concatenated, then k_nms's rule on the int boxes ACROSS the models (or, `separate`, only between
// detections of the same model).
#pragma once

namespace acfhip
{

// ------------------------------------------------------------------------
// k_join_bank: one workgroup per frame f.
//   0. the counts of f's lists (model 0 .. nModels - 1) are prefix-summed into off[0 .. nModels] in LDS; a concatenated index finds
//      its (model, index) by nms_list_of.  A list with a count < 0 or > maxHits, or a total above NMS_CAP, makes the frame unknowable:
//      count -1, no record;
//   1. type 0: the entries in concatenation order.  Else k_nms's rule, term for term (int boxes, int products, the quotient in f64):
//      keys (scores below thr dropped), bitonic sort of {orderable f64 key, concatenated index}, boxes and models in sorted order,
//      sequential-outer / parallel-inner suppression — separate: only a j of i's model is tested —, compaction, prune;
//   2. the first min(S, K) survivors are written as records and grown boxes (cut_box: acf_hip_crop_box's f32 steps); EVERY other slot
//      of boxesOut / framesOut gets zeros / -1, so that k_cut_crops may read all K slots of every frame at once.
// LDS: k_nms's 58 KB + a model byte per entry — a block still starts beside a resident cascade tile workgroup.
// ------------------------------------------------------------------------
constexpr int BANK_MODELS_MAX = ACF_HIP_BANK_MAX + 1;

struct JoinArgs
{
    const acf_hip_detection* dets[BANK_MODELS_MAX]; // model m's lists [nFrames][maxHits]
    const int32_t* counts[BANK_MODELS_MAX];         // [nFrames]
    int32_t nModels, nFrames, maxHits;
    int32_t type, ovrUnion, doPrune, maxCount, separate;
    double overlap, thr, pruneRatio;
    int32_t K;
    float inv, grow;               // acf_hip_crop_box's
    acf_hip_bank_detection* out;   // [nFrames][K]
    int32_t* countsOut;            // [nFrames]
    float* boxesOut;               // [nFrames][K][4], or null
    int32_t* framesOut;            // [nFrames][K], or null
};

__global__ void __launch_bounds__(1024) k_join_bank(JoinArgs a)
{
    extern __shared__ __align__(16) unsigned long long jb_lds[]; // (the int4 boxes: 16 bytes whatever static LDS lies in front)
    unsigned long long* key = jb_lds;                                   // [NMS_CAP]
    int4* box = reinterpret_cast<int4*>(key + NMS_CAP);                 // [NMS_CAP] {xs, ys, xe, ye} in sorted order
    uint32_t* idx = reinterpret_cast<uint32_t*>(box + NMS_CAP);         // [NMS_CAP]
    uint8_t* kp = reinterpret_cast<uint8_t*>(idx + NMS_CAP);            // [NMS_CAP]
    uint8_t* mdl = kp + NMS_CAP;                                        // [NMS_CAP] the model of sorted entry i
    __shared__ int s_off[BANK_MODELS_MAX + 1];
    __shared__ int s_drop, s_wave[16], s_cut, s_bad;
    const int frame = blockIdx.x, tid = threadIdx.x;
    const int K = a.K;
    // ---- 0. the offsets (at most nine lists: one thread sums them)
    if (tid == 0)
    {
        s_drop = 0;
        s_cut = 0x7fffffff;
        int bad = 0, sum = 0;
        s_off[0] = 0;
#pragma unroll
        for (int m = 0; m < BANK_MODELS_MAX; m++) // (constant indices into the argument struct: no copy of it in scratch)
        {
            if (m >= a.nModels)
            {
                s_off[m + 1] = sum;
                continue;
            }
            const int c = a.counts[m][frame];
            if (c < 0 || c > a.maxHits)
            {
                bad = 1;
            }
            else
            {
                sum += min(c, NMS_CAP + 1); // (so that the sum cannot wrap)
            }
            s_off[m + 1] = sum;
        }
        s_bad = bad;
    }
    if (tid < 16)
    {
        s_wave[tid] = 0;
    }
    __syncthreads();
    const int n = s_off[a.nModels];
    const bool unknowable = s_bad || n > NMS_CAP;
    acf_hip_bank_detection* __restrict__ O = a.out + int64_t(frame) * K;
    float* __restrict__ BO = a.boxesOut ? a.boxesOut + int64_t(frame) * K * 4 : nullptr;
    int32_t* __restrict__ FO = a.framesOut ? a.framesOut + int64_t(frame) * K : nullptr;
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
    const int64_t at0 = int64_t(frame) * a.maxHits;
    // the detection of concatenated index q, and its model
    auto entry = [&](int q, int& m) -> const acf_hip_detection& {
        m = nms_list_of(s_off, a.nModels, q);
        const acf_hip_detection* list = a.dets[0];
#pragma unroll
        for (int k = 1; k < BANK_MODELS_MAX; k++) // (selects over constant indices, as above)
        {
            list = m == k ? a.dets[k] : list;
        }
        return list[at0 + (q - s_off[m])];
    };
    const bool sorted = a.type != 0;
    // ---- 1. keys (dropped and padding entries sort last); type 0: every entry in concatenation order
    for (int i = tid; i < P; i += T)
    {
        unsigned long long k = 0ull;
        uint32_t ix = 0xffffffffu;
        if (sorted && i < n)
        {
            int m;
            const double sc = double(entry(i, m).score);
            if (sc < a.thr)
            {
                atomicAdd(&s_drop, 1);
            }
            else
            {
                k = nms_key(sc);
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
            kp[i] = 1;
        }
    }
    __syncthreads();
    const int m = sorted ? n - s_drop : n;
    if (sorted)
    {
        // ---- 2. bitonic sort, "before" = larger key, then smaller concatenated index (model, then index)
        nms_sort(key, idx, P, T, tid);
        // ---- boxes and models in sorted order
        for (int i = tid; i < m; i += T)
        {
            int mo;
            const acf_hip_detection& d = entry(int(idx[i]), mo);
            box[i] = make_int4(d.x, d.y, d.x + d.w, d.y + d.h);
            mdl[i] = uint8_t(mo);
            kp[i] = 1;
        }
        __syncthreads();
        // ---- 3. suppression (k_nms's, + the model test)
        for (int i = 0; i + 1 < m; i++)
        {
            if (a.type == 2 && !kp[i]) // uniform: every thread reads the same byte
            {
                continue;
            }
            const int4 bi = box[i];
            const int mi = mdl[i];
            const int asI = (bi.z - bi.x) * (bi.w - bi.y);
            for (int j = i + 1 + tid; j < m; j += T)
            {
                if (!kp[j] || (a.separate && mdl[j] != mi))
                {
                    continue;
                }
                const int4 bj = box[j];
                const int iw = min(bi.z, bj.z) - max(bi.x, bj.x);
                const int ih = min(bi.w, bj.w) - max(bi.y, bj.y);
                if (iw <= 0 || ih <= 0)
                {
                    continue;
                }
                const int asJ = (bj.z - bj.x) * (bj.w - bj.y);
                double o = double(iw * ih);
                const double u = a.ovrUnion ? (double(asI + asJ) - o) : double(min(asI, asJ));
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
            int mo;
            return double(entry(int(q), mo).score);
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
            int mo;
            const acf_hip_detection d = entry(q, mo);
            acf_hip_bank_detection r;
            r.x = d.x;
            r.y = d.y;
            r.w = d.w;
            r.h = d.h;
            r.score = d.score;
            r.scale = d.scale;
            r.model = mo;
            r.index = q - s_off[mo];
            O[i] = r;
            cut_box(d.x, d.y, d.w, d.h, a.inv, a.grow, gb);
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
