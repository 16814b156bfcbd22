/*
 * acf_hip.h — C ABI of the MI355X (gfx950) ACF detection backend.
 *
 * This is the drop-in boundary for the chnsPyramid + acfDetect hot path of
 * elucideye/acf.  The reference has no C ABI of its own (its boundary is the
 * C++ class acf::Detector, src/lib/acf/acf/ACF.h:50-624); each entry point
 * below names the reference interface it stands in for.  The host-side C++
 * class in acf_amd/host/ (same method names as acf::Detector) dlopen()s this
 * library; tests and bench.py bind it with ctypes.
 *
 * Conventions
 *  - Every function returns an int status (ACF_HIP_OK == 0) and never throws.
 *    The reference returns 0 on the hot path and throws on precondition
 *    failures (ACF.cpp:135-141, wrappers.hpp:29-32); here those become codes.
 *  - A plane is float[w][h] with h (image height, image-y) contiguous: the
 *    reference's transposed planar layout (MatP, MatP.cpp:51-73; ACF.cpp:137).
 *    A frame is `d` planes back to back; a batch is frames back to back.
 *  - All sizes are given in upright-image terms (h = image height, w = image
 *    width).  The reference stores them in cv::Size with the members swapped
 *    ({width = h, height = w}, ACFIO.h:168-181); the host class does that
 *    translation, this ABI never sees cv::Size.
 *  - "dev" pointers are HIP device pointers; "host" pointers are ordinary
 *    memory.  No torch / OpenCV types appear in any signature.
 */
#ifndef ACF_HIP_H
#define ACF_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define ACF_HIP_ABI_VERSION 9

#if defined(__GNUC__)
#define ACF_HIP_API __attribute__((visibility("default")))
#else
#define ACF_HIP_API
#endif

enum {
    ACF_HIP_OK = 0,
    ACF_HIP_E_INVALID = 1,     /* bad argument / precondition (reference: CV_Assert) */
    ACF_HIP_E_UNSUPPORTED = 2, /* option the HIP path does not implement */
    ACF_HIP_E_NOMODEL = 3,     /* set_model not called */
    ACF_HIP_E_NOPLAN = 4,      /* plan not called */
    ACF_HIP_E_HIP = 5,         /* HIP runtime error, see acf_hip_last_error */
    ACF_HIP_E_NODEVICE = 6,    /* no gfx950 device visible */
    ACF_HIP_E_CAPACITY = 7     /* more detections than the planned capacity */
};

/* rgbConvert flags (rgbConvert.cpp:106-128) */
enum {
    ACF_HIP_CS_GRAY = 0,
    ACF_HIP_CS_RGB = 1,
    ACF_HIP_CS_LUV = 2,
    ACF_HIP_CS_HSV = 3,
    ACF_HIP_CS_ORIG = 4
};

/*
 * Model + options: the fields of Detector::Classifier (ACF.h:292-310) and of
 * the Options tree (ACF.h:68-275) that the hot path reads.  Tree arrays are
 * row-major [nTrees][nTreeNodes] (the layout after the load-time transpose,
 * ACFIO.cpp:61-67) and are copied by acf_hip_set_model.
 */
typedef struct acf_hip_params
{
    /* Classifier */
    int32_t nTrees;
    int32_t nTreeNodes;
    int32_t treeDepth; /* 1..8 fixed depth, 0 = walk child[] (acfDetect1.cpp:100-166) */
    const uint32_t* fids;
    const float* thrs;
    const float* hs;
    /* treeDepth 0 (may be NULL when treeDepth > 0): child[k] == 0 marks a leaf; otherwise node k carries a test and the walk goes on
     * at node child[k] - (ftr < thr) of the same tree, i.e. the pair sits at child[k] - 1 and child[k] (acfDetect1.cpp:146-155).
     * Contract, checked by acf_hip_check_model and refused by acf_hip_set_model: child[k] < nTreeNodes and child[k] - 1 > k (trees
     * are stored parent-first, so every walk ends after at most nTreeNodes / 2 steps).  Only nodes with a test are read: fids, thrs
     * and child of a leaf, hs of a node with a test, and every array of a slot no walk reaches may hold anything. */
    const uint32_t* child;

    /* Options: modelDs, modelDsPad, stride, cascThr (ACF.h:204-211) */
    int32_t modelDs_h, modelDs_w;
    int32_t modelDsPad_h, modelDsPad_w;
    int32_t stride;
    double cascThr;

    /* Options::Pyramid (ACF.h:97-202) */
    int32_t nPerOct, nOctUp, nApprox;
    int32_t nLambdas; /* 3 (colour, gradMag, gradHist), or 0: estimated from every image (chnsPyramid.cpp:341-374) */
    double lambdas[3];
    int32_t pad_h, pad_w;
    int32_t minDs_h, minDs_w;
    double smooth; /* final channel smoothing radius (chnsPyramid.cpp:399-407) */

    /* Options::Pyramid::Chns (ACF.h:99-182) */
    int32_t shrink;
    int32_t colorEnabled;
    double colorSmooth;
    int32_t colorSpace; /* ACF_HIP_CS_* */
    int32_t gradMagEnabled;
    int32_t colorChn;
    int32_t normRad;
    double normConst;
    int32_t full;
    int32_t gradHistEnabled;
    int32_t binSize; /* 0 = shrink */
    int32_t nOrients;
    int32_t softBin;
    int32_t isLuv; /* Detector::setIsLuv (ACF.h:560-567) */

    /* LDCF (BASELINE cfg 5: "k 5x5 filters per channel").  NO reference counterpart ("has not yet been added",
     * README.rst:8): the definition is the upstream toolbox's acfDetectImg — for every level,
     *   C(:,:,j) = conv2(chns(:,:,mod(j-1,nChns)+1), filters(:,:,j), 'same'),  j = 1 .. nChns*k   (zero-padded true convolution)
     *   level    = imResample(C, .5)                                                 (size round(.5 * size))
     * and the cascade then runs with shrink*2 over nChns*k channels (fids index nChns*k*(modelDsPad/(2*shrink))^2 cells).
     * ldcfFilters: [k][nChns][5][5] floats in the MATLAB memory order of fs(:,:,c,f): tap (dy, dx) at dy + 5*dx.
     * The summation order of the 25 taps (dx ascending, then dy ascending, one chain of
     * fused multiply-adds acc = fmaf(v, w, acc) from 0: a single rounding per tap) is this repo's own.
     * ldcfK == 0 or ldcfFilters == NULL: off. */
    int32_t ldcfK;
    const float* ldcfFilters;
} acf_hip_params;

/* One detection in upright image coordinates (ACF.cpp:302-312, Detection ACF.h:510-525). */
typedef struct acf_hip_detection
{
    int32_t x, y, w, h;
    float score;
    int32_t scale; /* pyramid level that produced it */
} acf_hip_detection;

/* bbNms (types max / maxg; ms and cover are pass-through stubs in the reference, bbNms.cpp:100-108) and
 * ObjectDetector::prune, run on the device on every frame's detections (bbNms.cpp:111-192,229-304;
 * ObjectDetector.cpp:28-44).  Equal scores keep their detection order (the reference's std::sort leaves it open). */
typedef struct acf_hip_nms_params
{
    int32_t type;       /* 0 none, 1 max, 2 maxg (greedy) */
    int32_t ovrDnmUnion;/* 1: overlap / union (ovrDnm "union"), 0: overlap / smaller area ("min") */
    double overlap;     /* suppress when the ratio exceeds this */
    double thr;         /* scores below thr are dropped first (reference default: -DBL_MAX) */
    int32_t prune;      /* 1: apply ObjectDetector::prune to the survivors */
    int32_t maxCount;   /* m_maxDetectionCount */
    double pruneRatio;  /* m_detectionScorePruneRatio */
} acf_hip_nms_params;

#define ACF_HIP_NMS_CAP 2048 /* detections per frame the device NMS takes; more is ACF_HIP_E_CAPACITY */

/* One cascade hit before box mapping: DetectionSink::add({c,r},h) (acfDetect1.cpp:39-47,92-95). */
typedef struct acf_hip_hit
{
    int32_t scale, c, r;
    float score;
} acf_hip_hit;

/* Geometry of one pyramid level as planned by acf_hip_plan. */
typedef struct acf_hip_level
{
    double scale;            /* Pyramid::scales (ACF.h:374) */
    double scalehw_h;        /* Pyramid::scaleshw, image-height axis */
    double scalehw_w;        /* Pyramid::scaleshw, image-width axis */
    int32_t isReal;          /* computed exactly (chnsPyramid.cpp:274-277) */
    int32_t realIndex;       /* level it is approximated from (itself if real) */
    int32_t hC, wC;          /* channel plane size before padding (cells) */
    int32_t hP, wP;          /* plane size after BORDER_REFLECT padding = what the cascade sees */
    int32_t nWinR, nWinC;    /* window grid height1, width1 (acfDetect1.cpp:258-259) */
    int64_t offset;          /* float offset of this level inside one frame's fused pyramid */
} acf_hip_level;

typedef struct acf_hip_ctx acf_hip_ctx;

/* ---- lifecycle ------------------------------------------------------- */

/* Bind a context to `device` and to `stream` (a hipStream_t, or NULL for a
 * stream owned by the context).  Replaces constructing an acf::Detector
 * (ACF.h:59-66); good() == (return value == ACF_HIP_OK). */
ACF_HIP_API int acf_hip_create(int device, void* stream, acf_hip_ctx** out);
/* Number of gfx950 devices visible to the process (0 and ACF_HIP_E_NODEVICE when there is none): what a multi-device host
 * (acf::HipDetectorPool, one context per device) iterates over. */
ACF_HIP_API int acf_hip_device_count(int* count);
ACF_HIP_API int acf_hip_destroy(acf_hip_ctx* ctx);
ACF_HIP_API int acf_hip_abi_version(void);
/* Last error text for this context (thread-compatible, like one Detector per thread). */
ACF_HIP_API const char* acf_hip_last_error(const acf_hip_ctx* ctx);

/* Runtime knobs, the counterpart of the reference's setters (ACF.h:495-595).
 * Keys: "taps" (0/1: keep per-stage intermediates readable through
 * acf_hip_read_tap, the role of setLogger's MatLoggerType tap,
 * chnsCompute.cpp:241-250,285-300; costs one extra full-resolution write; set
 * before acf_hip_plan), "profile" (0/1: record HIP events around every kernel,
 * read with acf_hip_profile_get), "scale_streams" (1, default: the real scales of a
 * batch run concurrently on streams of the context — lowest latency and best
 * throughput for ONE context; 0: everything on the context's stream in order, for
 * applications that run several contexts side by side on one GPU), "rank_cells" (1,
 * default: the cascade of a depth-2 model reads 16-bit threshold-rank cells — the
 * comparison `chns[cid] < thrs[node]` of acfDetect1.cpp:102-104 decided on
 * rank(cell) < rank index of the threshold, the same decision for every cell and
 * node, hence identical hits and scores — instead of the float pyramid; 0: floats),
 * "keep_pyramid" (1, default; 0: the caller wants detections only — acf_hip_run /
 * acf_hip_pyramid + acf_hip_detect — and when the levels leave as rank cells the float
 * pyramid is not written at all: acf_hip_read_level then fails with ACF_HIP_E_INVALID, and so
 * does acf_hip_detect_bank, whose members read the float pyramid),
 * "cascade_turns" (0, default; for applications that run several contexts on one device,
 * the way the reference runs one Detector per thread: bit 0 = a context's cascade tile
 * kernel waits for the tile kernel submitted before it on that device, whichever
 * context's, bit 2 = the level kernel takes its turns in the same chain (bit 1: in a
 * chain of its own) — these kernels are bound by VALU and LDS, and two of them side by
 * side displace each other where each could run beside another context's memory-bound
 * pyramid kernels; three contexts, cfg 2: +4 % frames/s with 5),
 * "tile_persist" (1, default: the cascade's tile kernel runs as persistent workgroups that
 * draw their tiles from a counter — best for a context that has the device to itself;
 * 0: one workgroup per tile, which lets other contexts' kernels find free LDS between
 * tiles — what an application with several contexts per device wants; n > 1: n workgroups),
 * "fused_grad" (1, default: gradMag is computed inside the gradient plane's smoothing
 * chain — the smoothed plane then makes no round trip through memory — for planes of
 * >= 2^20 pixels in batches of >= 16 frames, where that pays; 2: wherever that kernel
 * applies; 0: always as its own kernel),
 * "fused_tri" (1, default: convTri's x pass over M — chnsCompute.cpp:283's convTri(M, S,
 * normRad) — rides on that chain as well, so M is written once and not read back by a
 * kernel of its own, in batches of >= 64 frames of a context with "shared_device" set; 2:
 * wherever "fused_grad"'s kernel runs; 0: never.  The gradient plane is then one uncut
 * chain of column steps per frame),
 * "shared_device" (0, default; 1: this context runs beside other contexts on the same
 * device — acf::HipDetectorPool and the Python DetectorPool set it.  Kernel forms are then
 * chosen for the least total work instead of the shortest time alone: the smoothing
 * chains of batches >= 64 frames stay uncut — no warm-up columns, no verify / repair
 * launch — and "fused_tri" applies; 3 contexts x 96 frames at 1080p: +4.3 % frames/s,
 * one context alone: -7 %),
 * "graph" (0, default; 1: acf_hip_run captures its own launches into a HIP graph the
 * second time it is called with the same frames pointer and batch size, and replays it
 * from then on — one host call instead of ~45 launches, for callers that feed one
 * frame at a time from a fixed buffer; not with "profile", taps, image-specific
 * lambdas, "cascade_turns" or sub-batch contexts ("streams" > 1), where the call runs
 * plainly; any set_* / plan call drops the graph),
 * "level_segments" (0, default = auto: batches of at most 8 frames cut every level's column
 * chain into speculative segments that are verified bit for bit on the device and repaired by a
 * whole-chain launch where a hand-over differs — a single frame's latency 1.05 -> 0.78 ms;
 * bigger batches run one chain per plane; 1: never; n > 1: n segments whatever the batch),
 * "level_warm" (32, default: warm-up columns of a level segment, a positive multiple of 4),
 * "smooth_segments" / "smooth_warm" (the same for the image smoothing: 0 = as many segments as
 * fill the device, 64 warm-up columns), "count_repairs" (1: acf_hip_get_repairs counts the
 * planes the repair launches recomputed; synchronises, measurements only),
 * "smooth_force_redo" (tests: 1 = every plane with more than one segment is marked for the
 * repair launch whatever the verification found),
 * "cascade_tiles", "fused_levels", "fused_smooth", "streams" (kernel-form A/B
 * switches; all forms give identical results),
 * "arith" (0, default: the three sites where the reference's SSE kernels use _mm_rsqrt_ps /
 * _mm_rcp_ps — gradMag, gradMagNorm, rgb2luv_sse: toolbox/gradientMex.cpp:209-219,266,
 * toolbox/rgbConvertMex.cpp:161, toolbox/sse.hpp:185-192 — compute 1/sqrt and 1/x exactly;
 * 1: they return the bits of one x86 CPU's instructions, from the tables installed with
 * acf_hip_set_x86_tables — the pyramid and the detections are then what the reference's own
 * compiled kernels give on that CPU, bit for bit.  Every kernel form of the default path has
 * this arithmetic too (the tables ride in LDS beside the acos table): ~94 % of the default
 * tier's frames/s).
 *
 * Capacity: `max_hits` of acf_hip_plan bounds the hits kept per frame.  With stride < shrink
 * (the cascade then runs once per distinct cell offset and k_expand_hits writes every window
 * of a surviving offset) a frame whose EXPANDED total exceeds max_hits reports the overflow
 * in its count as always, but WHICH of its hits are retained is unspecified (slots are
 * reserved in thread order; a q x q group may be partly written).  "keep_pyramid" = 0 has no
 * effect for LDCF models, for stride < shrink and for tree depths 1, 3 and 4 on rank cells:
 * those paths read the float pyramid (their overflow queues do), so it is always written.
 *
 * Environment, read once per process: ACF_HIP_FORCE_FALLBACK=name[,name...] makes the named stages run their fallback form where
 * the default form would (identical results; the tests hold every form against the oracle that way; DESIGN.md §8 lists the names;
 * an unknown name aborts).  `triy_stored_u`: convTri's x pass (normRad 5) writes the blocked plane U and the fused y pass reads it
 * back, instead of the default — (T, U) checkpoints every 16 columns, an eighth of the plane, from which the y pass re-runs the
 * x pass over the M blocks (acf_hip_get_tri_forms reports which form a call took). */
ACF_HIP_API int acf_hip_set_option(acf_hip_ctx* ctx, const char* key, int value);

/* The reference's arithmetic at its three approximate sites (option "arith" = 1).  _mm_rcp_ps and _mm_rsqrt_ps
 * (toolbox/sse.hpp:185-192) are 12-bit approximations whose bits belong to the CPU.  On the CPUs probed (an Intel Xeon and an AMD
 * EPYC, each checked for all 2^32 inputs) they are functions of the input's sign, exponent (its parity for rsqrt) and top 12
 * mantissa bits:
 *   rcp4096[m >> 11]                      = bits of _mm_rcp_ps(x)   for x = 1.m in [1, 2)        (4096 entries)
 *   rsqrt8192[(odd << 12) | (m >> 11)]    = bits of _mm_rsqrt_ps(x) for x in [1, 2) (odd = 0) and [2, 4) (odd = 1)
 * and every other input follows by exponent arithmetic (zero / subnormal -> inf, inf -> 0, results below the normal range
 * -> 0, NaN quieted, rsqrt of a negative -> 0xffc00000).  A host that wants "what the reference gives HERE" fills the tables
 * from its own CPU (acf::HipDetector::setReferenceArithmetic does, acf_amd/host/HipDetector.h); tests install the build
 * host's (tests/golden/x86_rcp_rsqrt.npz) or probe the host they run on.  The tables are copied to the device; the call may be
 * repeated.  Sub-batch contexts ("streams" > 1) share their parent's tables. */
ACF_HIP_API int acf_hip_set_x86_tables(acf_hip_ctx* ctx, const uint32_t* rcp4096, const uint32_t* rsqrt8192);
/* Self-check of the device's table functions: position-mixed 64-bit digests of rcp (digest[0]) and rsqrt (digest[1]) over the
 * bit patterns first + i * stride, i < count — the sums the CPU oracle's acfo_x86_digest forms from the same tables, so the
 * two implementations are compared for every input without moving 2^32 results — and digest[2] = the number of those patterns
 * (taken as gradMag's M2: the negative non-NaN ones skipped) for which the column kernels' one-read form of
 * m = min(rsqrt(M2), 1e10), M = rcp(m) differs from the two table functions applied in turn: must be 0. */
ACF_HIP_API int acf_hip_selftest_x86(acf_hip_ctx* ctx, uint32_t first_bits, uint64_t count, uint32_t stride, uint64_t digest[3]);

/* Detector::getScales (static, chnsPyramid.cpp:461-529): host only, no context.
 * Writes up to `cap` scales and returns the total count in *n. */
ACF_HIP_API int acf_hip_get_scales(int nPerOct, int nOctUp, int minDs_h, int minDs_w, int shrink, int h, int w,
    double* scales, double* scaleshw_h, double* scaleshw_w, int cap, int* n);

/* The level geometry acf_hip_plan would produce for these options and frame
 * size, computed on the host without touching a device (what chnsPyramid's
 * bookkeeping, chnsPyramid.cpp:270-292, and createDetector's window grid,
 * acfDetect1.cpp:258-259, yield). */
ACF_HIP_API int acf_hip_plan_levels(const acf_hip_params* p, int h, int w, int d, acf_hip_level* out, int cap, int* nScales, int* nChns);

/* Is this classifier one the device may walk?  Host only, no context.  Always: the checks of acf_hip_set_model on nTrees, nTreeNodes,
 * treeDepth, the arrays, stride, shrink and modelDsPad, and for treeDepth 0 the child[] contract (acf_hip_params::child).  nChns > 0:
 * also every test's feature id < nChns * (modelDsPad_h / shrink) * (modelDsPad_w / shrink), the index space of cids[]
 * (acfDetect1.cpp:390-406); nChns = 0: structure only.  Leaves and unused slots are not inspected.  Returns ACF_HIP_OK or
 * ACF_HIP_E_INVALID; `why` (may be NULL) receives the reason, at most cap bytes with the terminator. */
ACF_HIP_API int acf_hip_check_model(const acf_hip_params* p, int nChns, char* why, int cap);

/* Upload classifier + options.  Refuses what acf_hip_check_model(p, 0, ..) refuses, so that no later entry launches a walk over a
 * child[] that does not end.  Replaces Detector::deserialize*() filling
 * `clf` and `opts` (ACF.h:277,312) and acfModify's effects (acfModify.cpp:139-143),
 * which the caller applies to the struct before the call. */
ACF_HIP_API int acf_hip_set_model(acf_hip_ctx* ctx, const acf_hip_params* p);

/* Plan for frames of h x w with `d` input planes (1 or 3; or 5 = three image planes followed by the gradient magnitude and
 * orientation that come WITH the image — the GL pipeline's LUVMO frames, chnsPyramid.cpp:248-255: M and O then replace
 * gradientMag at the first real scale, :318-322, which must be the image's own size: nOctUp = 0; they are used verbatim whatever
 * colorSpace and normRad say, as in the reference; 4 planes are refused on purpose, where the reference would drop the lone extra
 * plane) and up to `max_batch` frames per call and `max_hits` hits per frame: runs getScales
 * (chnsPyramid.cpp:461-529) and the real/approximate split
 * (chnsPyramid.cpp:272-292), builds resampling tables and allocates every
 * device buffer.  Nothing is allocated after this call. */
ACF_HIP_API int acf_hip_plan(acf_hip_ctx* ctx, int h, int w, int d, int max_batch, int max_hits);
ACF_HIP_API int acf_hip_num_levels(const acf_hip_ctx* ctx, int* nScales, int* nChns);
ACF_HIP_API int acf_hip_get_levels(const acf_hip_ctx* ctx, acf_hip_level* out, int cap);
/* Geometry of the LDCF levels the cascade reads when the model has ldcfK > 0 (hP, wP = round(.5 * size), window grid at
 * shrink*2, offsets inside one frame's LDCF pyramid); same count as acf_hip_get_levels.  ACF_HIP_E_INVALID without LDCF. */
ACF_HIP_API int acf_hip_get_ldcf_levels(const acf_hip_ctx* ctx, acf_hip_level* out, int cap);
/* Floats in one frame's fused pyramid (sum over levels of nChns*wP*hP). */
ACF_HIP_API int acf_hip_pyramid_floats(const acf_hip_ctx* ctx, int64_t* n);
/* The lambdas frame `frame` of the last acf_hip_pyramid / acf_hip_run was approximated with: the model's, or — for a
 * model without lambdas — the ones estimated from that image (Detector::Pyramid::lambdas, chnsPyramid.cpp:341-374). */
ACF_HIP_API int acf_hip_get_lambdas(acf_hip_ctx* ctx, int frame, double out[3]);

/* ---- the hot path ---------------------------------------------------- */

/* Detector::chnsPyramid for a batch (chnsPyramid.cpp:160-456).  `frames_dev`:
 * n_frames x d planes of float[w][h] already on the device.  Asynchronous on
 * the context's stream.
 * Values: the reference feeds images in [0, 1] (ACF.cpp:119).  Bit parity with it is checked for every finite input whose
 * squared gradients stay finite (|values| up to ~1e18: flat regions, denormal-sized and very large gradients included,
 * tests/test_gpu_arith.py); frames holding NaN / inf, or values whose squares overflow f32, are outside the contract (the
 * reference itself turns those into inf / NaN channels). */
ACF_HIP_API int acf_hip_pyramid(acf_hip_ctx* ctx, const float* frames_dev, int n_frames);

/* Detector::operator()(const Pyramid&) without NMS (ACF.cpp:268-367) on the
 * pyramid of the last acf_hip_pyramid call: acfDetect1 on every level
 * (acfDetect1.cpp:309-335) + box mapping.  Asynchronous. */
ACF_HIP_API int acf_hip_detect(acf_hip_ctx* ctx);

/* acf_hip_pyramid + acf_hip_detect: Detector::operator()(const MatP&) (ACF.cpp:246-265). */
ACF_HIP_API int acf_hip_run(acf_hip_ctx* ctx, const float* frames_dev, int n_frames);

/* Same with frames in host memory (H2D copy included). */
ACF_HIP_API int acf_hip_run_host(acf_hip_ctx* ctx, const float* frames_host, int n_frames);

/* Pixel layouts of packed 8-bit frames: the cv::Mat inputs of the image entry
 * Detector::operator()(const cv::Mat&) (CV_8UC3 RGB, ACF.cpp:135-141) and the
 * BGR/BGRA/grey video frames the apps convert before calling it (acf.cpp:117-148,
 * GPUDetectionPipeline.cpp:250-266).  Alpha is ignored. */
enum {
    ACF_HIP_PIX_RGB = 0,
    ACF_HIP_PIX_BGR = 1,
    ACF_HIP_PIX_RGBA = 2,
    ACF_HIP_PIX_BGRA = 3,
    ACF_HIP_PIX_GRAY = 4,
    /* YUV 4:2:0 video frames as decoders hand them out (semi-planar: a luma plane, then one plane of interleaved chroma
     * pairs, U,V for NV12 and V,U for NV21); see "YUV 4:2:0 input" below */
    ACF_HIP_PIX_NV12 = 5,
    ACF_HIP_PIX_NV21 = 6
};

/* The image entry for 8-bit input: cvt8UC3To32FC3 = convertTo(CV_32F, 1/255)
 * (ACF.cpp:114-119), I.t() (ACF.cpp:137) and the MatP plane split
 * (MatP.cpp:51-73) in one kernel, fused with the colour conversion of
 * chnsPyramid.cpp:230-263 when the model asks for one; then as acf_hip_pyramid.
 * `frames_dev`: n_frames upright images of h rows x w pixels, `row_stride_bytes`
 * between rows (0 = tightly packed), frames back to back (h * stride bytes
 * apart).  The plan's `d` must be 3 for the colour layouts and 1 for GRAY. */
ACF_HIP_API int acf_hip_pyramid_u8(acf_hip_ctx* ctx, const uint8_t* frames_dev, int n_frames, int pix, int row_stride_bytes);
ACF_HIP_API int acf_hip_run_u8(acf_hip_ctx* ctx, const uint8_t* frames_dev, int n_frames, int pix, int row_stride_bytes);

/* YUV 4:2:0 input (ACF_HIP_PIX_NV12 / _NV21) in the 8-bit entries (acf_hip_pyramid_u8 / run_u8 / stream_*).
 * Semantics: cvtColor(frame, COLOR_YUV2RGB_NV12 / _NV21) — the call a user of Detector::operator()(const cv::Mat&) makes on
 * decoded video — followed by the image entry above: BT.601 limited range in 20-bit fixed point, the chroma pair of a 2 x 2
 * block shared by its four pixels with no interpolation; all int32, >> arithmetic (floor):
 *     CY = 1220542, CVR = 1673527, CVG = -852492, CUG = -409993, CUB = 2116026
 *     y   = max(0, Y - 16) * CY
 *     ruv = (1 << 19) + CVR * (V - 128)
 *     guv = (1 << 19) + CVG * (V - 128) + CUG * (U - 128)
 *     buv = (1 << 19) + CUB * (U - 128)
 *     R = clamp((y + ruv) >> 20, 0, 255)   G = clamp((y + guv) >> 20, 0, 255)   B = clamp((y + buv) >> 20, 0, 255)
 * cvtColor is OpenCV's (not part of the reference tree): the published algorithm of its imgproc/src/color_yuv.simd.hpp is
 * restated; PARITY UNPINNED (DESIGN.md 7 says what was checked: within one code value of the rounded real BT.601 matrix on
 * every (Y, U, V)).  One kernel takes the frames to the converted planar f32 image (k_ingest_yuv420); the planes are bit for
 * bit those of the RGB layout fed with the R, G, B bytes above.
 * Frame layout: h rows of w luma bytes, `row_stride_bytes` apart (0 = w); then h / 2 rows of w / 2 chroma pairs at the same
 * row stride.  h and w must be even (of the plan, or of the unreduced frame with acf_hip_set_input_resize, where the order is
 * convert, resize, ingest as in the apps); the plan's `d` must be 3 (the luma plane is limited range, not the grey cvtColor
 * gives: a d = 1 plan is ACF_HIP_E_INVALID).
 *  acf_hip_set_yuv_layout    decoder surfaces pad the luma plane to an aligned height and the frame to an aligned size:
 *                            the chroma plane starts `chroma_offset_bytes` after a frame's first luma byte and frames are
 *                            `frame_stride_bytes` apart; 0, 0 = tight (chroma at stride * h, frames stride * h * 3 / 2
 *                            apart).  After acf_hip_plan, before acf_hip_stream_open; sticky until the next plan; the packed
 *                            layouts ignore it.  A chroma offset inside the luma plane or a frame stride that lets frames
 *                            overlap is refused by the run / open call, where the row stride is known
 *  acf_hip_op_yuv420_to_rgb  the conversion alone, host buffers: src one frame of chroma_offset_bytes (0 = tight) +
 *                            stride * rows / 2 bytes, dst rows x cols x 3 tight R, G, B
 *  acf_hip_u8_frame_bytes    host arithmetic, no context, no GPU: the bytes from one tight frame of layout `pix` to the next
 *                            (stride * rows for the packed layouts, stride * rows * 3 / 2 for NV12 / NV21; row_stride_bytes
 *                            0 = tight rows).  ACF_HIP_E_INVALID for an unknown layout, sizes < 1, a stride smaller than a
 *                            row, odd NV12 / NV21 sizes */
ACF_HIP_API int acf_hip_set_yuv_layout(acf_hip_ctx* ctx, int64_t chroma_offset_bytes, int64_t frame_stride_bytes);
ACF_HIP_API int acf_hip_op_yuv420_to_rgb(acf_hip_ctx* ctx, const uint8_t* src_host, int rows, int cols, int pix, int row_stride_bytes,
    int64_t chroma_offset_bytes, uint8_t* dst_host);
ACF_HIP_API int acf_hip_u8_frame_bytes(int pix, int rows, int cols, int row_stride_bytes, int64_t* out);

/* The image entry for upright device images of any element strides: what a tensor library holds ([n, c, H, W] in NCHW or
 * channels_last memory, packed RGB / BGR / RGBA, padded rows, a rectangular view into a larger surface) in uint8, float16,
 * bfloat16 or float32 — Detector::operator()(const cv::Mat&) for CV_32FC3 as well as CV_8UC3 (ACF.cpp:135-141: I.t(), then the
 * MatP split, MatP.cpp:51-73), with no transposed copy in front of it.
 *     plane[c][x][y] = value(frames_dev[n * stride_n + c * stride_c + y * stride_y + x * stride_x])     at the plan's h x w
 *     value: u8 float(v) * float(1 / 255.0) (as acf_hip_pyramid_u8); f16, bf16 the exact widening to f32; f32 the value itself
 * and then exactly acf_hip_pyramid / acf_hip_run on those planes: every level, hit, score bit and box is what the planar entry
 * gives for the same values (option "arith" = 1 included).  One kernel (k_ingest_image, so named under option "profile"), fused
 * with the colour conversion of chnsPyramid.cpp:230-263 when the model asks for LUV / grey; a 1-plane image is replicated as
 * chnsPyramid.cpp:234-244 says.
 * Strides are in ELEMENTS — what torch.Tensor.stride() reports for an [n, c, H, W] tensor or view.  stride_x >= 1, stride_y >= 1;
 * stride_n >= 0 (0 repeats one frame); stride_c any value: negative reads the channels backwards (packed BGR: frames_dev + 2
 * with stride_c = -1), 0 replicates one plane.  RGBA with the alpha skipped is stride_x = 4, channels = 3.  frames_dev is a
 * multiple of the element size.  Only addressed elements are read: a view may end with its allocation.
 * Asynchronous on the context's stream; nothing is allocated after the first call.  The calls always run plainly and leave a
 * captured graph of acf_hip_run (option "graph") valid; ACF_HIP_TAP_IMAGE behaves as after acf_hip_pyramid_u8.
 * ACF_HIP_E_INVALID: null pointers, n_frames outside 1 .. max_batch, an unknown dtype, channels other than the plan's d, a
 * five-plane plan, stride_x < 1, stride_y < 1, stride_n < 0, an active acf_hip_set_input_resize (8-bit packed only);
 * ACF_HIP_E_UNSUPPORTED with option "streams" > 1; ACF_HIP_E_NOPLAN without a plan.
 *  acf_hip_image_extent      host arithmetic, no context, no GPU: the lowest and the highest element offset from frames_dev that a
 *                            call with these arguments reads (first_elem <= 0 <= last_elem), to check a buffer or a view against */
enum {
    ACF_HIP_T_U8 = 0,
    ACF_HIP_T_F16 = 1,
    ACF_HIP_T_BF16 = 2,
    ACF_HIP_T_F32 = 3
};
typedef struct acf_hip_image_desc {
    int32_t dtype;    /* ACF_HIP_T_* */
    int32_t channels; /* 1 or 3: the plan's d */
    int64_t stride_n, stride_c, stride_y, stride_x; /* in elements, of an image indexed [n][c][y][x] (y = image row, x = image column) */
} acf_hip_image_desc;
ACF_HIP_API int acf_hip_pyramid_image(acf_hip_ctx* ctx, const void* frames_dev, int n_frames, const acf_hip_image_desc* desc);
ACF_HIP_API int acf_hip_run_image(acf_hip_ctx* ctx, const void* frames_dev, int n_frames, const acf_hip_image_desc* desc);
ACF_HIP_API int acf_hip_image_extent(const acf_hip_image_desc* desc, int h, int w, int n_frames, int64_t* first_elem, int64_t* last_elem);

/* The video frame entry for YUV frames of three planes, each described by its own offset and byte strides: what a software
 * decoder hands out (yuv420p = I420: three planes, often three allocations, each with its own line size), a capture device's
 * packed 4:2:2 (YUYV / UYVY / YVYU), the 4:2:2 and 4:4:4 planar surfaces of professional video, and NV12 / NV21 again.  For
 * pixel (row r, column c) of frame n at the plan's h x w, all offsets and strides in BYTES from base_dev:
 *     Y = base_dev[y.offset + n * y.stride_n + r * y.stride_row + c * y.stride_px]
 *     U = base_dev[u.offset + n * u.stride_n + (r >> sub_y) * u.stride_row + (c >> sub_x) * u.stride_px]
 *     V = base_dev[v.offset + n * v.stride_n + (r >> sub_y) * v.stride_row + (c >> sub_x) * v.stride_px]
 * (no chroma interpolation: a chroma sample is shared by the 1, 2 or 4 pixels above it), then R, G, B by the formula under
 * "YUV 4:2:0 input" above, and from there on exactly acf_hip_pyramid_u8 / run_u8(ACF_HIP_PIX_RGB) on those bytes: every plane,
 * level, hit, score bit and box is what the packed RGB entry gives for the converted frame (option "arith" = 1 included).  A
 * descriptor that describes an NV12 / NV21 frame gives what acf_hip_run_u8(ACF_HIP_PIX_NV12 / _NV21) gives, bit for bit.
 * cvtColor counterparts: COLOR_YUV2RGB_NV12 / _NV21 / _I420 / _YV12 / _YUY2 (YUYV) / _UYVY / _YVYU, which share the BT.601
 * fixed-point helpers in OpenCV's imgproc/src/color_yuv.simd.hpp; I422 and I444 have no cvtColor code with this arithmetic: they
 * are this library's extension of the same per-pixel formula.  OpenCV is not part of the reference tree: its published
 * algorithm is restated; PARITY UNPINNED.
 * h and w may be odd: a chroma plane then has ceil(h / 2^sub_y) rows of ceil(w / 2^sub_x) samples.  Offsets may be negative
 * (three separately allocated planes: base_dev is one of them, the others lie where they lie); stride_px >= 1, stride_row >= 1,
 * stride_n >= 0 (0 repeats one frame).  Only addressed bytes are ever read, so a plane may end with its allocation;
 * acf_hip_yuv_extent gives the byte range of each plane to check against.  The plan's d must be 3.
 * One kernel (k_ingest_yuv) with three load forms chosen from the descriptor and base_dev's alignment alone, all giving the same
 * bits; under option "profile" it reports as k_ingest_yuv_planar (all three stride_px = 1; every plane's first byte, stride_row
 * and stride_n multiples of 4: dword loads), k_ingest_yuv_packed422 (4:2:2 macropixels of four bytes, 4-aligned: one dword holds
 * two pixels) or k_ingest_yuv_generic (byte loads, any strides); an NV12 / NV21-shaped descriptor of even h, w runs
 * k_ingest_yuv420, the kernel of the 8-bit entry.
 * Asynchronous on the context's stream; nothing is allocated after the first call.  The calls always run plainly and leave a
 * captured graph of acf_hip_run (option "graph") valid; ACF_HIP_TAP_IMAGE behaves as after acf_hip_pyramid_u8.
 * ACF_HIP_E_INVALID: null pointers, n_frames outside 1 .. max_batch, sub_x / sub_y outside {0, 1}, stride_px < 1, stride_row < 1,
 * stride_n < 0, a plan of 1 or 5 input planes, an active acf_hip_set_input_resize; ACF_HIP_E_UNSUPPORTED with option "streams"
 * > 1; ACF_HIP_E_NOPLAN without a plan.
 *  acf_hip_yuv_to_rgb8       the conversion alone (k_yuv_to_rgb8), device buffers, no model, no plan: tight [n_frames][rows][cols][3]
 *                            R, G, B at dst_dev, asynchronously on the context's stream
 *  acf_hip_yuv_extent        host arithmetic, no context, no GPU: first[p] / last[p] = the lowest / highest byte offset from
 *                            base_dev a call with these arguments reads of plane p (0 = Y, 1 = U, 2 = V)
 *  acf_hip_yuv_layout        host arithmetic: the descriptor of a named layout (ACF_HIP_YUV_*, NOT ACF_HIP_PIX_*) of h x w with
 *                            row_stride_bytes between luma rows (0 = tight: w, or 2 * w for the packed names); *frame_bytes = the
 *                            distance to the next frame = stride_n of every plane.  NV12 / NV21: the tight rule of the 8-bit
 *                            entry.  I420 / YV12 / I422 / I444: the luma plane, then the two chroma planes tight behind one
 *                            another at row stride (row_stride_bytes >> sub_x), U then V (YV12: V then U).  YUYV / UYVY / YVYU:
 *                            macropixels of four bytes in the named order (Y0 U Y1 V / U Y0 V Y1 / Y0 V Y1 U).  The 4:2:0 names
 *                            need even h and w, the 4:2:2 names even w; the planar names an even luma stride; a stride shorter than a
 *                            row, an unknown name, sizes < 1 and null outputs are ACF_HIP_E_INVALID.  Odd sizes are for hand-built
 *                            descriptors only
 *  acf_hip_stream_open_yuv   the streaming front end (below) for host frames of frame_bytes each: every plane's one-frame extent
 *                            must lie in [0, frame_bytes) and stride_n == frame_bytes; acf_hip_stream_submit then copies
 *                            n_frames * frame_bytes and runs acf_hip_run_yuv on the slot; submit / collect / close are unchanged,
 *                            and a later acf_hip_stream_open replaces it (and the other way round) */
enum {
    ACF_HIP_YUV_NV12 = 0, /* Y plane; U, V interleaved */
    ACF_HIP_YUV_NV21 = 1, /* Y plane; V, U interleaved */
    ACF_HIP_YUV_I420 = 2, /* 4:2:0 planar Y, U, V (yuv420p) */
    ACF_HIP_YUV_YV12 = 3, /* 4:2:0 planar Y, V, U */
    ACF_HIP_YUV_I422 = 4, /* 4:2:2 planar Y, U, V */
    ACF_HIP_YUV_I444 = 5, /* 4:4:4 planar Y, U, V */
    ACF_HIP_YUV_YUYV = 6, /* 4:2:2 packed Y0 U Y1 V (YUY2) */
    ACF_HIP_YUV_UYVY = 7, /* 4:2:2 packed U Y0 V Y1 */
    ACF_HIP_YUV_YVYU = 8  /* 4:2:2 packed Y0 V Y1 U */
};
typedef struct acf_hip_yuv_plane {
    int64_t offset, stride_n, stride_row, stride_px; /* bytes */
} acf_hip_yuv_plane;
typedef struct acf_hip_yuv_desc {
    acf_hip_yuv_plane y, u, v;
    int32_t sub_x, sub_y; /* 0 or 1: log2 of the chroma subsampling along image-x / image-y */
} acf_hip_yuv_desc;
ACF_HIP_API int acf_hip_pyramid_yuv(acf_hip_ctx* ctx, const uint8_t* base_dev, int n_frames, const acf_hip_yuv_desc* desc);
ACF_HIP_API int acf_hip_run_yuv(acf_hip_ctx* ctx, const uint8_t* base_dev, int n_frames, const acf_hip_yuv_desc* desc);
ACF_HIP_API int acf_hip_yuv_to_rgb8(acf_hip_ctx* ctx, const uint8_t* base_dev, int n_frames, int rows, int cols, const acf_hip_yuv_desc* desc,
    uint8_t* dst_dev);
ACF_HIP_API int acf_hip_yuv_extent(const acf_hip_yuv_desc* desc, int h, int w, int n_frames, int64_t first[3], int64_t last[3]);
ACF_HIP_API int acf_hip_yuv_layout(int layout, int h, int w, int row_stride_bytes, acf_hip_yuv_desc* out, int64_t* frame_bytes);
ACF_HIP_API int acf_hip_stream_open_yuv(acf_hip_ctx* ctx, const acf_hip_yuv_desc* desc, int64_t frame_bytes, int cap, int depth);

/* The apps' resize to a minimum object width (src/app/acf/acf.cpp:117-148 `Resizer`,
 * GPUDetectionPipeline.cpp:250-266 computeDetectionWidth): scale = float(winSize.width) /
 * float(minWidth); cv::resize(image, reduced, {}, scale, scale, scale < 1 ? INTER_AREA :
 * INTER_LINEAR) on the packed 8-bit frame, the detector on `reduced`, the boxes back by
 * cv::Rect2f(o) * (1.f / scale).  cv::resize is OpenCV's (not part of the reference tree):
 * the CV_8U arithmetic of its imgproc/resize.cpp is restated (DESIGN.md 6b says what
 * exactly); PARITY UNPINNED.
 *  acf_hip_resize_dims       the reduced size cv::resize produces: cvRound(rows * scale) x cvRound(cols * scale)
 *  acf_hip_set_input_resize  after acf_hip_plan FOR THE REDUCED SIZE: from now on the 8-bit entries
 *                            (acf_hip_pyramid_u8 / run_u8 / stream_*) take frames of src_rows x src_cols and
 *                            reduce them on the device first (k_resize_u8); src_rows = 0 switches it off; a new
 *                            plan switches it off
 *  acf_hip_op_resize_u8      the resize alone, host buffers (dst: dst_rows x dst_cols x cpp, tight) */
ACF_HIP_API int acf_hip_resize_dims(int rows, int cols, double scale, int* out_rows, int* out_cols);
ACF_HIP_API int acf_hip_set_input_resize(acf_hip_ctx* ctx, int src_rows, int src_cols, double scale);
ACF_HIP_API int acf_hip_op_resize_u8(acf_hip_ctx* ctx, const uint8_t* src_host, int rows, int cols, int cpp, int row_stride_bytes, double scale,
    uint8_t* dst_host, int dst_rows, int dst_cols);

/* The same resize inside the tensor and YUV entries: frames of src_rows x src_cols as the descriptor describes them (acf_hip_image_desc
 * / acf_hip_yuv_desc above; acf_hip_image_extent / acf_hip_yuv_extent called with src_rows x src_cols give exactly the bytes that are
 * read), reduced by `scale` and ingested in ONE kernel (k_ingest_resized; option "profile": k_ingest_resized_image /
 * k_ingest_resized_yuv) — no converted or reduced 8-bit image goes to device memory.  The plan must be for
 * acf_hip_resize_dims(src_rows, src_cols, scale).
 * Definition: the existing entries composed, bit for bit —
 *   YUV    acf_hip_yuv_to_rgb8 on the source frames, acf_hip_op_resize_u8's arithmetic with 3 bytes a pixel, acf_hip_pyramid_u8 / run_u8
 *          (ACF_HIP_PIX_RGB)
 *   image  the addressed bytes as an upright interleaved image of `channels` bytes a pixel, the same resize with cpp = channels, run_u8
 *          with ACF_HIP_PIX_RGB or ACF_HIP_PIX_GRAY
 * every plane, level, hit, score bit and box, option "arith" = 1 included.  Detections are in the reduced frame's coordinates, as with
 * acf_hip_set_input_resize: cv::Rect2f(o) * (1.f / scale) maps them back.  cv::resize and cvtColor are OpenCV's (not part of the
 * reference tree): their published arithmetic is restated; PARITY UNPINNED.
 * The tap tables of (src_rows, src_cols, scale) are built and uploaded at the first call with a new triple (which waits for the
 * context's stream before the previous triple's tables go) and kept: nothing is allocated on later calls with the same triple; a new
 * plan drops them.  Asynchronous on the context's stream; the calls always run plainly and leave a captured graph of acf_hip_run
 * (option "graph") valid; ACF_HIP_TAP_IMAGE behaves as after acf_hip_pyramid_u8.
 * ACF_HIP_E_INVALID: what the un-resized entry refuses; src_rows / src_cols < 1; a scale that is not a positive finite number; a plan
 * of other dimensions; an active acf_hip_set_input_resize.  ACF_HIP_E_UNSUPPORTED: option "streams" > 1; an image dtype other than
 * ACF_HIP_T_U8 (cv::resize's CV_32F arithmetic is not restated).  ACF_HIP_E_NOPLAN without a plan.
 *  acf_hip_stream_open_yuv_resized   acf_hip_stream_open_yuv's rules with the one-frame extents taken at src_rows x src_cols; every
 *                                    submit runs acf_hip_run_yuv_resized on its slot; submit / collect / close are unchanged */
ACF_HIP_API int acf_hip_pyramid_yuv_resized(acf_hip_ctx* ctx, const uint8_t* base_dev, int n_frames, const acf_hip_yuv_desc* desc, int src_rows,
    int src_cols, double scale);
ACF_HIP_API int acf_hip_run_yuv_resized(acf_hip_ctx* ctx, const uint8_t* base_dev, int n_frames, const acf_hip_yuv_desc* desc, int src_rows, int src_cols,
    double scale);
ACF_HIP_API int acf_hip_pyramid_image_resized(acf_hip_ctx* ctx, const void* frames_dev, int n_frames, const acf_hip_image_desc* desc, int src_rows,
    int src_cols, double scale);
ACF_HIP_API int acf_hip_run_image_resized(acf_hip_ctx* ctx, const void* frames_dev, int n_frames, const acf_hip_image_desc* desc, int src_rows, int src_cols,
    double scale);
ACF_HIP_API int acf_hip_stream_open_yuv_resized(acf_hip_ctx* ctx, const acf_hip_yuv_desc* desc, int64_t frame_bytes, int src_rows, int src_cols,
    double scale, int cap, int depth);

/* ---- rotated and mirrored frames in the tensor and YUV entries ---------
 * Video is stored in sensor orientation with a rotation tag, and front cameras mirror; the cascade only finds upright objects.  The
 * oriented entries read the frame where it lies, as the descriptor describes it at src_rows x src_cols (Hs x Ws), and detect on the
 * upright frame — no rotated copy goes to device memory.  An orientation code is rot + 4 * mirror; the upright frame U of source S is
 *     U = np.rot90(S[:, ::-1] if mirror else S, k=-rot)     (mirror left-right first, then rot quarter turns CLOCKWISE)
 * so upright pixel (r, c) is source pixel (rs, cs):
 *     rot 0: (r, c)   rot 1: (Hs-1-c, r)   rot 2: (Hs-1-r, Ws-1-c)   rot 3: (c, Ws-1-r);   mirror: cs becomes Ws-1-cs
 * The plan must be for the upright size, acf_hip_oriented_dims(src_rows, src_cols, orient): Ws x Hs for odd rot.
 * Definition: the existing entries composed, bit for bit —
 *   image  the addressed elements of the descriptor at Hs x Ws re-arranged into U, then acf_hip_pyramid_image / run_image on a tight
 *          upright image holding U (every dtype, channels 1 or 3, stride_c of any sign)
 *   YUV    acf_hip_yuv_to_rgb8's R, G, B of the source frame (the chroma sample of source pixel (rs, cs) at (rs >> sub_y, cs >> sub_x):
 *          chosen in SOURCE coordinates) re-arranged into U, then acf_hip_pyramid_u8 / run_u8 (ACF_HIP_PIX_RGB)
 * every plane, level, hit, score bit and box, option "arith" = 1 included.  Detections are in U's coordinates; acf_hip_unorient_rect
 * maps a box back to the source frame.  ACF_HIP_ORIENT_UPRIGHT is the un-oriented entry's call: the same kernels under the same profile
 * names (every entry of a kind is one call of the library's general entry of that kind; none calls another).
 * acf_hip_image_extent / acf_hip_yuv_extent called with src_rows x src_cols give exactly the elements and bytes an oriented call
 * reads (an orientation permutes the same pixel set), and no load covers an address outside the [first, last] span of the row and
 * plane it belongs to.
 * Option "profile": k_ingest_image_oriented_rows / k_ingest_yuv_oriented_rows (rot 0 / 2) and k_ingest_image_oriented_cols /
 * k_ingest_yuv_oriented_cols (rot 1 / 3) with wide loads along the source rows — under the conditions of the un-oriented entries'
 * vector forms, and for NV12 / NV21-like descriptions whose planes, row and frame strides are 4-aligned — else
 * k_ingest_image_oriented_generic / k_ingest_yuv_oriented_generic (one element a lane, any description).
 * Asynchronous on the context's stream; nothing is allocated after the first call; the calls always run plainly and leave a captured
 * graph of acf_hip_run (option "graph") valid; ACF_HIP_TAP_IMAGE behaves as after acf_hip_pyramid_u8.
 * ACF_HIP_E_INVALID: what the un-oriented entry refuses; orient outside 0 .. 7; src_rows / src_cols < 1; a plan whose h x w is not
 * acf_hip_oriented_dims(...); an active acf_hip_set_input_resize; a five-plane plan.  ACF_HIP_E_UNSUPPORTED: option "streams" > 1.
 * ACF_HIP_E_NOPLAN without a plan.
 *  acf_hip_stream_open_yuv_oriented   acf_hip_stream_open_yuv's rules with the one-frame extents taken at src_rows x src_cols; every
 *                                     submit runs acf_hip_run_yuv_oriented on its slot; submit / collect / close are unchanged
 *  acf_hip_oriented_dims              host arithmetic: the upright h x w; ACF_HIP_E_INVALID for a bad code, size or null pointer
 *  acf_hip_unorient_rect              host arithmetic, exact: the upright box {x, y, w, h} -> the box covering the same pixels in the
 *                                     source frame: {x', y', w', h'} with, for even rot, x' = x or Ws - x - w, y' = y or Hs - y - h,
 *                                     w' = w, h' = h, and for odd rot x' = y or Ws - y - h, y' = x or Hs - x - w, w' = h, h' = w (the
 *                                     second form where that source index runs against the upright one); defined by the same
 *                                     formula for boxes that reach outside the frame, as padded detections do */
enum
{
    ACF_HIP_ORIENT_UPRIGHT = 0,        /* U = S */
    ACF_HIP_ORIENT_ROT90 = 1,          /* S turned a quarter turn clockwise */
    ACF_HIP_ORIENT_ROT180 = 2,
    ACF_HIP_ORIENT_ROT270 = 3,         /* a quarter turn anticlockwise */
    ACF_HIP_ORIENT_MIRROR = 4,         /* S[:, ::-1] */
    ACF_HIP_ORIENT_MIRROR_ROT90 = 5,   /* the anti-transpose S[::-1, ::-1].T */
    ACF_HIP_ORIENT_MIRROR_ROT180 = 6,  /* S[::-1, :] */
    ACF_HIP_ORIENT_MIRROR_ROT270 = 7   /* the transpose S.T */
};
ACF_HIP_API int acf_hip_pyramid_image_oriented(acf_hip_ctx* ctx, const void* frames_dev, int n_frames, const acf_hip_image_desc* desc, int src_rows,
    int src_cols, int orient);
ACF_HIP_API int acf_hip_run_image_oriented(acf_hip_ctx* ctx, const void* frames_dev, int n_frames, const acf_hip_image_desc* desc, int src_rows, int src_cols,
    int orient);
ACF_HIP_API int acf_hip_pyramid_yuv_oriented(acf_hip_ctx* ctx, const uint8_t* base_dev, int n_frames, const acf_hip_yuv_desc* desc, int src_rows,
    int src_cols, int orient);
ACF_HIP_API int acf_hip_run_yuv_oriented(acf_hip_ctx* ctx, const uint8_t* base_dev, int n_frames, const acf_hip_yuv_desc* desc, int src_rows, int src_cols,
    int orient);
ACF_HIP_API int acf_hip_stream_open_yuv_oriented(acf_hip_ctx* ctx, const acf_hip_yuv_desc* desc, int64_t frame_bytes, int src_rows, int src_cols,
    int orient, int cap, int depth);
ACF_HIP_API int acf_hip_oriented_dims(int src_rows, int src_cols, int orient, int* h, int* w);
ACF_HIP_API int acf_hip_unorient_rect(int orient, int src_rows, int src_cols, const int32_t in[4], int32_t out[4]);

/* ---- rotated and mirrored frames, reduced to a minimum object width ----
 * The two families above joined: the frame as stored (src_rows x src_cols = Hs x Ws, an orientation code) is turned upright and THEN
 * reduced by `scale`, in ONE kernel — the order of the reference's GL front end (GPUACF.cpp: rotate -> smooth -> reduce).  No rotated,
 * converted or reduced 8-bit image goes to device memory.
 * Definition: the existing entries composed, bit for bit —
 *   1. the bytes of S: the addressed u8 elements at the descriptor's strides (image), or acf_hip_yuv_to_rgb8's R, G, B with the chroma
 *      sample chosen in SOURCE coordinates (YUV), exactly as the oriented entries define it
 *   2. U = np.rot90(S[:, ::-1] if mirror else S, k=-rot), the upright frame of the oriented entries
 *   3. acf_hip_op_resize_u8's arithmetic on U as a tight interleaved image of `channels` bytes a pixel (3 for YUV), with the tap tables
 *      of (upright rows, upright cols, scale)
 *   4. acf_hip_pyramid_u8 / run_u8 (ACF_HIP_PIX_RGB or ACF_HIP_PIX_GRAY)
 * i.e. acf_hip_run_image_resized on a tight upright u8 image holding U: every plane, level, hit, score bit and box, option "arith" = 1
 * included.  Orient-then-resize and resize-then-orient give different bytes (cvRound of the sizes, asymmetric area taps): orient first.
 * The plan must be for acf_hip_oriented_resized_dims(src_rows, src_cols, orient, scale) = acf_hip_resize_dims(acf_hip_oriented_dims(...)).
 * Detections are in the reduced upright frame: cv::Rect2f(o) * (1.f / scale) first, then acf_hip_unorient_rect.  cv::resize and cvtColor
 * are OpenCV's (not part of the reference tree): their published arithmetic is restated; PARITY UNPINNED.
 * ACF_HIP_ORIENT_UPRIGHT is the *_resized entry's call.  acf_hip_image_extent / acf_hip_yuv_extent at src_rows x src_cols give the
 * bytes that may be read, and no load covers an address outside the [first, last] span of the row and plane it belongs to.
 * Option "profile": k_ingest_oriented_resized_image / k_ingest_oriented_resized_yuv for quarter turns (odd rot) at scales >= 1 / 4 — the
 * tile's footprint in the stored frame is read along the stored rows into LDS (dword loads for descriptions that meet the un-oriented
 * entries' row-vector / planar conditions, else bytes) and resampled from there — and the same names with _generic (each lane gathers
 * its own pixels from device memory) for rot 0 / 2, where the lanes run along the stored rows anyway, for smaller scales, and under
 * ACF_HIP_FORCE_FALLBACK=oriented_resized_generic.  Both forms give the same bits.
 * Asynchronous on the context's stream; the tap tables are those of the resized entries (built at the first call with a new upright
 * size and scale, kept; nothing is allocated on later calls); the calls always run plainly and leave a captured graph of acf_hip_run
 * (option "graph") valid; ACF_HIP_TAP_IMAGE behaves as after acf_hip_pyramid_u8.
 * ACF_HIP_E_INVALID: what either family refuses; orient outside 0 .. 7; a plan of other dimensions; an active
 * acf_hip_set_input_resize; a five-plane plan; a scale that is not a positive finite number.  ACF_HIP_E_UNSUPPORTED: option "streams"
 * > 1; an image dtype other than ACF_HIP_T_U8.  ACF_HIP_E_NOPLAN without a plan.
 *  acf_hip_stream_open_yuv_oriented_resized   acf_hip_stream_open_yuv's rules with the one-frame extents taken at src_rows x src_cols;
 *                                             every submit runs acf_hip_run_yuv_oriented_resized on its slot
 *  acf_hip_oriented_resized_dims              host arithmetic, no context: the reduced upright h x w; ACF_HIP_E_INVALID for a bad code,
 *                                             size, scale or null pointer */
ACF_HIP_API int acf_hip_pyramid_image_oriented_resized(acf_hip_ctx* ctx, const void* frames_dev, int n_frames, const acf_hip_image_desc* desc, int src_rows,
    int src_cols, int orient, double scale);
ACF_HIP_API int acf_hip_run_image_oriented_resized(acf_hip_ctx* ctx, const void* frames_dev, int n_frames, const acf_hip_image_desc* desc, int src_rows,
    int src_cols, int orient, double scale);
ACF_HIP_API int acf_hip_pyramid_yuv_oriented_resized(acf_hip_ctx* ctx, const uint8_t* base_dev, int n_frames, const acf_hip_yuv_desc* desc, int src_rows,
    int src_cols, int orient, double scale);
ACF_HIP_API int acf_hip_run_yuv_oriented_resized(acf_hip_ctx* ctx, const uint8_t* base_dev, int n_frames, const acf_hip_yuv_desc* desc, int src_rows,
    int src_cols, int orient, double scale);
ACF_HIP_API int acf_hip_stream_open_yuv_oriented_resized(acf_hip_ctx* ctx, const acf_hip_yuv_desc* desc, int64_t frame_bytes, int src_rows, int src_cols,
    int orient, double scale, int cap, int depth);
ACF_HIP_API int acf_hip_oriented_resized_dims(int src_rows, int src_cols, int orient, double scale, int* h, int* w);

/* ---- video formats: 9 .. 16-bit samples, BT.709 / BT.2020, full range ---
 * The YUV entries above convert with one arithmetic: 8-bit samples, BT.601, limited range.  The video entries take the same
 * descriptor (acf_hip_yuv_desc keeps its meaning: all offsets and strides in BYTES) together with an acf_hip_yuv_format:
 *   bits        8: one byte a sample.  9 .. 16: one little-endian 16-bit word a sample, sample = (word >> shift) & ((1 << bits) - 1);
 *               a planar 16-bit plane has stride_px 2, P010's chroma stride_px 4 with V two bytes behind U
 *   shift       P010 = 6, P012 = 4, P016 / yuv420p10le = 0; must be 0 for 8 bits; shift + bits <= 16
 *   matrix      ACF_HIP_YUV_MATRIX_BT601 / _BT709 / _BT2020 (Rec. ITU-T H.273 MatrixCoefficients 5 / 6, 1, 9)
 *   full_range  0 limited ("video"), 1 full ("pc" / JPEG)
 * A null format is the default {8, 0, BT601, 0}.
 * Arithmetic, in exact integers (N = bits; >> is floor; an implementation may use any width that gives the same integers):
 *     yoff = full_range ? 0 : 16 << (N - 8);   cmid = 1 << (N - 1);   out_max = full_range ? (1 << N) - 1 : 255 << (N - 8)
 *     y = max(0, Y - yoff) * CY
 *     R = clamp((y + (1 << 19) + CVR * (V - cmid)) >> 20, 0, out_max)
 *     G = clamp((y + (1 << 19) + CVG * (V - cmid) + CUG * (U - cmid)) >> 20, 0, out_max)
 *     B = clamp((y + (1 << 19) + CUB * (U - cmid)) >> 20, 0, out_max)
 *     plane value = float(R) * float(1.0 / out_max)          (8 bits: float(1 / 255.0), as every 8-bit entry)
 * N-bit limited-range codes are read as the 8-bit codes times 2^(N - 8), as H.273 defines them, so the constants do not depend on N.
 * Full range follows H.273 / JFIF: luma gain 1, the chroma excursion half the RGB range.  The constants are round(2^20 * q), half
 * away from zero, q the exact rational from Kr / Kb (0.299 / 0.114, 0.2126 / 0.0722, 0.2627 / 0.0593); limited range: luma gain
 * 255 / 219, chroma gain 255 / 224.  BT.601 limited is the exception: it KEEPS cvtColor's constants (from coefficients rounded to three
 * decimals), so that the default format is the arithmetic of the entries above.
 *     matrix, range     CY       CVR      CVG      CUG      CUB
 *     BT601 limited     1220542  1673527  -852492  -409993  2116026
 *     BT601 full        1048576  1470104  -748826  -360853  1858077
 *     BT709 limited     1220945  1879825  -558796  -223607  2215014
 *     BT709 full        1048576  1651297  -490864  -196424  1945738
 *     BT2020 limited    1220945  1760217  -682019  -196426  2245811
 *     BT2020 full       1048576  1546230  -599107  -172546  1972791
 * The chroma sample of pixel (r, c) is the one at (r >> sub_y, c >> sub_x) in SOURCE coordinates, no interpolation, as above.
 * Definition of the entries, composed from what exists, bit for bit (every plane, level, hit, score bit and box, option "arith" = 1
 * included):
 *   8 bits, any matrix or range   acf_hip_run_u8(ACF_HIP_PIX_RGB) on the R, G, B bytes above; with orient / scale the bytes of the
 *                                 stored frame go through the oriented, resized or oriented-then-resized definitions above, unchanged
 *   more than 8 bits              acf_hip_run_image on a tight packed float32 RGB image holding float(R) * float(1.0 / out_max)
 * OpenCV has no counterpart beyond BT.601 8-bit: PARITY UNPINNED; the matrices are H.273's.
 *  acf_hip_pyramid_video / run_video   scale 0: no resize, the plan is for acf_hip_oriented_dims(src_rows, src_cols, orient); otherwise
 *                            for acf_hip_oriented_resized_dims(...).  orient 0 with scale 0 is the plain entry (src_rows = src_cols = 0:
 *                            the plan's size).  This is the general YUV entry: acf_hip_run_yuv, _oriented, _resized and _oriented_resized
 *                            are this call with the default format and what they do not state left 0, so the default format runs
 *                            the same kernels under the same profile names as they do.
 *                            Other 8-bit formats run the same kernels with the constants as an argument (the profile names stay; an
 *                            NV12 / NV21-shaped descriptor still runs k_ingest_yuv420).  More than 8 bits: k_ingest_yuv16, one kernel with
 *                            three load forms chosen from the descriptor and base_dev's alignment alone, all giving the same bits:
 *                            k_ingest_yuv16_planar (every stride_px 2; every plane's first byte, stride_row and stride_n multiples of 4),
 *                            k_ingest_yuv16_pairs (P010-like: luma as planar; U and V interleaved 16-bit pairs, 4-aligned) and
 *                            k_ingest_yuv16_generic (16-bit loads, any even offsets and strides; Y210 runs here).  Only addressed
 *                            words are read.
 *  acf_hip_stream_open_video the streaming front end with acf_hip_stream_open_yuv's rules (extents in BYTES, acf_hip_video_extent)
 *  acf_hip_video_to_rgb      the conversion alone, device buffers, no model, no plan: dst_dev is tight [n_frames][rows][cols][3] of
 *                            uint8 (8 bits) or uint16 (more) holding R, G, B in [0, out_max]
 *  acf_hip_video_extent      host arithmetic: as acf_hip_yuv_extent, with last[p] the last BYTE read (the high byte of the last word)
 *  acf_hip_video_layout      host arithmetic: the nine ACF_HIP_YUV_* names with 1 or 2 bytes a sample (acf_hip_yuv_layout's rules with
 *                            every size in bytes doubled for bits > 8; row_stride_bytes 0 = tight).  P010 is (ACF_HIP_YUV_NV12, bits
 *                            10, shift 6), yuv420p10le (ACF_HIP_YUV_I420, bits 10), Y210 (ACF_HIP_YUV_YUYV, bits 10, shift 6)
 *  acf_hip_yuv_coeffs        host only: {yoff, cmid, out_max, CY, CVR, CVG, CUG, CUB}
 * ACF_HIP_E_INVALID: what the family's existing entry refuses; bits outside 8 .. 16; shift != 0 with bits 8; shift + bits > 16; an
 * unknown matrix; full_range outside {0, 1}; with bits > 8 an odd base, offset or stride.  ACF_HIP_E_UNSUPPORTED: option "streams"
 * > 1; bits > 8 together with orient != 0 or scale != 0 — cv::resize's 16-bit arithmetic is not restated, and a 16-bit oriented kernel
 * is deliberately left for later.  Not covered: chroma siting and interpolation, transfer functions (PQ / HLG), tone mapping,
 * big-endian words. */
enum { ACF_HIP_YUV_MATRIX_BT601 = 0, ACF_HIP_YUV_MATRIX_BT709 = 1, ACF_HIP_YUV_MATRIX_BT2020 = 2 };
typedef struct acf_hip_yuv_format {
    int32_t bits;       /* 8: one byte a sample.  9..16: one little-endian 16-bit word a sample */
    int32_t shift;      /* bits > 8: sample = (word >> shift) & ((1 << bits) - 1).  P010 = 6, P012 = 4, P016 / yuv420p10le = 0 */
    int32_t matrix;     /* ACF_HIP_YUV_MATRIX_* */
    int32_t full_range; /* 0 limited ("video"), 1 full ("pc" / JPEG) */
} acf_hip_yuv_format;   /* 16 bytes.  {8, 0, BT601, 0} is the arithmetic of the YUV entries above */
ACF_HIP_API int acf_hip_pyramid_video(acf_hip_ctx* ctx, const uint8_t* base_dev, int n_frames, const acf_hip_yuv_desc* desc, const acf_hip_yuv_format* fmt,
    int src_rows, int src_cols, int orient, double scale);
ACF_HIP_API int acf_hip_run_video(acf_hip_ctx* ctx, const uint8_t* base_dev, int n_frames, const acf_hip_yuv_desc* desc, const acf_hip_yuv_format* fmt,
    int src_rows, int src_cols, int orient, double scale);
ACF_HIP_API int acf_hip_stream_open_video(acf_hip_ctx* ctx, const acf_hip_yuv_desc* desc, const acf_hip_yuv_format* fmt, int64_t frame_bytes, int src_rows,
    int src_cols, int orient, double scale, int cap, int depth);
ACF_HIP_API int acf_hip_video_to_rgb(acf_hip_ctx* ctx, const uint8_t* base_dev, int n_frames, int rows, int cols, const acf_hip_yuv_desc* desc,
    const acf_hip_yuv_format* fmt, void* dst_dev);
ACF_HIP_API int acf_hip_video_extent(const acf_hip_yuv_desc* desc, const acf_hip_yuv_format* fmt, int h, int w, int n_frames, int64_t first[3],
    int64_t last[3]);
ACF_HIP_API int acf_hip_video_layout(int layout, const acf_hip_yuv_format* fmt, int h, int w, int row_stride_bytes, acf_hip_yuv_desc* out,
    int64_t* frame_bytes);
ACF_HIP_API int acf_hip_yuv_coeffs(const acf_hip_yuv_format* fmt, int64_t out[8]);

/* ---- crops of the stored frame: the stage behind the detections ---------
 * What nearly every caller does with a detector's boxes is crop them and hand the crops to a second model (landmarks, recognition, a
 * verifier such as acf_hip_evaluate_crops).  These entries read only the pixels under the boxes from the frame AS STORED — the
 * descriptors, formats and orientation codes of the entries above — and write upright crops of one fixed size into one device tensor,
 * in the order of the boxes; no box goes through the host, no converted or turned frame goes to device memory.  No reference
 * counterpart: the definition below is this library's own.
 *
 * The upright frame U.  Hu x Wu = acf_hip_oriented_dims(src_rows, src_cols, orient); upright pixel (r, c) is the stored pixel of the
 * orientation mapping above ("rotated and mirrored frames").  Its C values are exact floats:
 *   image source   C = channels; the addressed element: u8 as float(v), f16 / bf16 / f32 widened
 *   YUV source     C = 3; the integer R, G, B of the format's arithmetic at the stored pixel, chroma chosen in SOURCE coordinates: what
 *                  acf_hip_video_to_rgb writes
 * Sampling.  A box is (bx, by, bw, bh) = x, y, w, h in U's coordinates (pixel centres at integers + 0.5 of a unit grid: pixel c covers
 * [c, c + 1)); s = samples.  Every operation is an f32 operation rounded once, none fused:
 *     stepx = bw / float(out_w * s)            stepy = bh / float(out_h * s)
 *     v(m)  = (bx + (float(m) + 0.5f) * stepx) - 0.5f,   m = j * s + b,   clamped to [0, float(Wu - 1)]   (rows alike with by, stepy, Hu)
 *     c0 = int(floorf(v)), c1 = min(c0 + 1, Wu - 1), fx = v - float(c0)
 *     top = p00 + fx * (p01 - p00);  bot = p10 + fx * (p11 - p10);  sample = top + fy * (bot - top)
 *     acc = 0; for a < s: for b < s: acc = acc + sample(i * s + a, j * s + b);      val = acc * float(1.0 / (s * s))
 * Clamping the coordinate is border replication: a box may reach outside the frame, as padded detections do.
 * Output.  unit = float(1 / 255.0) for 8-bit codes (u8 images, 8-bit video), float(1.0 / out_max) for video of more than 8 bits, 1 for
 * floating images.  ACF_HIP_T_F32: val * unit; F16 / BF16: that value narrowed round-to-nearest-even; U8 (8-bit code sources only):
 * uint8(clamp(rint(val), 0, 255)), val unscaled.  layout 0: a crop is [C][out_h][out_w], 1: [out_h][out_w][C]; crops lie back to back,
 * acf_hip_crop_bytes apart.
 * Bad boxes.  A box with a non-finite member or bw <= 0 / bh <= 0, and a frame index outside [0, n_frames), give a crop of zeros.
 * Nothing in boxes_dev makes the kernel read outside the addressed elements: acf_hip_image_extent / acf_hip_video_extent at src_rows x
 * src_cols stay the bound.
 *  acf_hip_cut_crops        a context, no model, no plan (like acf_hip_video_to_rgb): crop i of box boxes_dev[i] in frame frame_dev[i]
 *                           into slot i of dst_dev.  n = 0 launches nothing (boxes_dev and frame_dev may then be null)
 *  acf_hip_cut_detections   on the detections of the context's last acf_hip_detect / acf_hip_run*: for frame f, n_f = the device-side
 *                           count (after the device NMS when it is on); n_f = -1 (over ACF_HIP_NMS_CAP): counts_out[f] = -1 and no crop;
 *                           else counts_out[f] = min(n_f, K, max_hits), and slot f * K + i of dst_dev (and of boxes_out_dev) is detection
 *                           i in acf_hip_get_detections' order with the box acf_hip_crop_box gives (the same f32 operations, on the
 *                           device).  Slots at and beyond the count are not written.  det_scale: the scale the frames were reduced by
 *                           (0: none); the plan's h x w must be acf_hip_oriented_resized_dims(src_rows, src_cols, orient, det_scale),
 *                           or acf_hip_oriented_dims(...) for det_scale 0, and n_frames the last batch
 *  acf_hip_crop_box         host only: a detection {x, y, w, h} of the reduced frame as a box in U — the apps' cv::Rect2f(o) * (1.f / scale)
 *                           (src/app/acf/acf.cpp:548-551): inv = det_scale == 0 ? 1.f : 1.f / float(det_scale); each of x, y, w, h is
 *                           float(int) * inv; then cx = x + w * 0.5f, w' = w * grow, x' = cx - w' * 0.5f, and y alike
 *  acf_hip_crop_bytes       host only: bytes of one crop, out_h * out_w * channels * the element size
 *  acf_hip_crop_form        host only: the form k_cut_crops takes for this box (Hu x Wu, channels and bytes of a staged code value: 1 for
 *                           8-bit codes, 2 for wider video and f16 / bf16 images, 4 for f32 images): 0 staged, 1 gather
 * One kernel, k_cut_crops (so named under option "profile"), one workgroup a crop slot, two forms chosen per crop, both giving the same
 * bits: staged — bands of output rows whose clamped footprint in U is loaded once along the stored rows into LDS as code values (YUV
 * converted once per stored pixel) and sampled from there — and gather — every sample fetches its four neighbours through the source's
 * accessor: right for strong reductions, where a footprint holds far more pixels than are sampled.  The rule (acf_hip_crop_form): gather
 * when the crop's footprint holds more than four pixels a sample, or when the footprint of one output row does not fit the stage.
 * Both entries are asynchronous on the context's stream, allocate nothing, never wait for the device, always run plainly and leave a
 * captured graph of acf_hip_run (option "graph") valid.
 * ACF_HIP_E_INVALID: null pointers; both or neither of image / yuv; what the oriented image / video entry refuses about the
 * description and the format; orient outside 0 .. 7; sizes < 1; out sizes, samples, dtype, layout, max_per_frame or reserved out of
 * range; grow not positive finite; n < 0; cut_detections without valid detections, with n_frames other than the last batch, with a
 * det_scale that is not 0 or a positive finite number, or with a plan of other dimensions.  ACF_HIP_E_UNSUPPORTED: U8 output from a
 * floating image or from video of more than 8 bits; option "streams" > 1.  Not covered: area-exact reduction (samples is the
 * anti-aliasing), rotated boxes, chroma interpolation, five-plane frames. */
typedef struct acf_hip_crop_source {          /* the frames as stored: exactly one of image / yuv is non-NULL */
    const void* base_dev; int32_t n_frames;
    const acf_hip_image_desc* image;          /* as acf_hip_run_image_oriented reads it */
    const acf_hip_yuv_desc* yuv; const acf_hip_yuv_format* fmt;   /* as acf_hip_run_video reads it; fmt NULL = default */
    int32_t src_rows, src_cols, orient;       /* stored size (Hs x Ws) and ACF_HIP_ORIENT_* */
} acf_hip_crop_source;
typedef struct acf_hip_crop_spec {
    int32_t out_h, out_w;      /* 1 .. 512 */
    int32_t samples;           /* s: s x s bilinear samples averaged per output pixel, 1 .. 4 */
    int32_t dtype;             /* ACF_HIP_T_U8 / F16 / BF16 / F32 */
    int32_t layout;            /* 0 planar [C][out_h][out_w], 1 packed [out_h][out_w][C] */
    int32_t max_per_frame;     /* K, 1 .. ACF_HIP_NMS_CAP; cut_detections only */
    float grow;                /* box grown about its centre by this factor (1 = the box); cut_detections only */
    int32_t reserved;          /* 0 */
} acf_hip_crop_spec;
ACF_HIP_API int acf_hip_cut_crops(acf_hip_ctx* ctx, const acf_hip_crop_source* src, const float* boxes_dev /* [n][4] x, y, w, h in U */,
    const int32_t* frame_dev /* [n] */, int n, const acf_hip_crop_spec* spec, void* dst_dev);
ACF_HIP_API int acf_hip_cut_detections(acf_hip_ctx* ctx, const acf_hip_crop_source* src, double det_scale, const acf_hip_crop_spec* spec, void* dst_dev,
    float* boxes_out_dev /* [n_frames][K][4], may be NULL */, int32_t* counts_out_dev /* [n_frames] */);
ACF_HIP_API int acf_hip_crop_box(const int32_t det[4], double det_scale, float grow, float out[4]);
ACF_HIP_API int acf_hip_crop_bytes(const acf_hip_crop_spec* spec, int channels, int64_t* bytes_per_crop);
ACF_HIP_API int acf_hip_crop_form(const acf_hip_crop_spec* spec, const float box[4], int Hu, int Wu, int channels, int sample_bytes, int* form);

/* ---- affine views of the stored frame: tilted, zoomed, cut out ----------
 * The cascade only finds upright objects of the plan's frame.  These entries make every frame of the batch an AFFINE VIEW of a stored
 * frame, sampled on the way in: the same frame at a few roll angles (or at the gyroscope's), a tracker's neighbourhood of the last box
 * magnified, one quadrant of a large frame at full resolution, several windows of one frame in one batch — without a turned, scaled or
 * cut copy in device memory and without a host round trip.  No reference counterpart: the definition below is this library's own.
 *
 * The stored frames are an acf_hip_crop_source, and the upright frame U (Hu x Wu = acf_hip_oriented_dims; C exact floats a pixel: an
 * image's C = channels elements, a YUV source's integer R, G, B of the format's arithmetic, chroma chosen in SOURCE coordinates) is the
 * one "crops of the stored frame" defines.
 * A view is six floats m[6]: it maps the continuous coordinates of the plan's h x w frame into U's,
 *     xu = m0 * x + m1 * y + m2,   yu = m3 * x + m4 * y + m5        (pixel c covers [c, c + 1) in both frames)
 * Sampling.  For pixel (r, c) of view i, s = samples (1 .. 4), every operation an f32 operation rounded once, none fused:
 *     inv = float(1.0 / s)
 *     py = (float(r * s + a) + 0.5f) * inv          px = (float(c * s + b) + 0.5f) * inv          a, b = 0 .. s - 1
 *     u  = (((m0 * px) + (m1 * py)) + m2) - 0.5f    v  = (((m3 * px) + (m4 * py)) + m5) - 0.5f
 *     u  = u > 0.f ? u : 0.f;  u = u < float(Wu - 1) ? u : float(Wu - 1)       (v alike with Hu; NaN becomes 0: border replication)
 *     c0 = int(floorf(u)) clamped to [0, Wu - 1], c1 = min(c0 + 1, Wu - 1), fx = u - float(c0)       (rows alike)
 *     top = p00 + fx * (p01 - p00);  bot = p10 + fx * (p11 - p10);  sample = top + fy * (bot - top)
 *     acc = 0; for a: for b: acc = acc + sample;      val = acc * float(1.0 / (s * s))
 *     plane value = val * unit
 * unit as for the crops: float(1 / 255.0) for 8-bit codes, float(1.0 / out_max) for video of more than 8 bits, 1 for floating images.
 * From there on the call IS acf_hip_pyramid_image / acf_hip_run_image on a tight planar float32 image [n_views][C][h][w] holding those
 * plane values: the colour-conversion mode the ingest picks for the plan's size, every level, hit, score bit and box, option "arith"
 * = 1 included.  The clamp makes every bit pattern of m safe: no view makes a load leave the extent acf_hip_image_extent /
 * acf_hip_video_extent give at src_rows x src_cols.  View i reads stored frame frame_dev[i] (frame_dev NULL: frame i); an index
 * outside [0, n_frames) reads nothing and yields the frame of all-zero code values.
 * Consequences: the identity view {1,0,0, 0,1,0} with s = 1 on a source whose Hu x Wu is the plan's size is the oriented image / video
 * entry bit for bit (u = c exactly, fx = 0, val = p00; on sources without negative zeros); {1,0,tx, 0,1,ty} with integers tx, ty is
 * acf_hip_run_image on the strided sub-view; video of more than 8 bits may be oriented here, which acf_hip_run_video refuses.
 *  acf_hip_pyramid_view / acf_hip_run_view   n_views = 1 .. max_batch; view i becomes frame i of the batch.  Asynchronous on the context's
 *                           stream; they allocate nothing after the first call, always run plainly and leave a captured graph of
 *                           acf_hip_run valid.  ACF_HIP_TAP_IMAGE as after acf_hip_pyramid_u8.  The detections are in VIEW coordinates:
 *                           acf_hip_cut_detections refuses after a view call (ACF_HIP_E_INVALID, "the last run was a view") until another
 *                           run; the device-only route to crops is acf_hip_merge_views + acf_hip_cut_crops (next section), the host's
 *                           acf_hip_view_box + acf_hip_cut_crops
 *  acf_hip_view_from_box    host only, in double from the float inputs, rounded to float: the view whose frame is the box (x, y, w, h in
 *                           U) turned by angle_rad about its centre: sx = bw / w, sy = bh / h, m0 = sx cos, m1 = -sy sin, m3 = sx sin,
 *                           m4 = sy cos, m2 = cx - (m0 w + m1 h) / 2, m5 = cy - (m3 w + m4 h) / 2.  Angle 0: the plain cut-and-scale
 *  acf_hip_view_quad        host only: a detection {x, y, w, h} of the view's frame as its corners TL, TR, BR, BL (x, y each) in U
 *  acf_hip_view_box         host only: the bounding box (x, y, w, h) of that quad in U: what acf_hip_cut_crops takes
 *  acf_hip_view_form        host only: the form k_ingest_view takes for tile (tile_x, tile_y) of the h x w frame (tiles of 64 x 64; channels
 *                           and sample_bytes as acf_hip_crop_form): 0 staged, 1 gather
 * One kernel, k_ingest_view (option "profile": k_ingest_view_image / k_ingest_view_yuv), grid (tiles x, tiles y, n_views), ending in the
 * store phase of every ingest kernel.  Two forms chosen per tile, both giving the same bits: staged — the clamped coordinates of the
 * tile's four corner samples, widened and clamped to U, give a rectangle that is loaded once along the stored rows into LDS as code
 * values (YUV converted once per stored pixel) and sampled from there; a sample whose 2 x 2 neighbourhood is not wholly inside it
 * fetches through the source's accessor — and gather — every sample fetches its four neighbours through the accessor: when the
 * rectangle holds more than four stored pixels a sample, or does not fit the stage (wide codes under a tilt, three f32 channels).
 * ACF_HIP_E_INVALID: null pointers; both or neither of image / yuv; what the oriented image / video entry refuses about the
 * description, the format and the orientation; channels other than the plan's d; a five-plane plan; samples outside 1 .. 4; n_views
 * outside 1 .. max_batch; frame_dev NULL with n_views > n_frames; an active acf_hip_set_input_resize.  ACF_HIP_E_UNSUPPORTED: option
 * "streams" > 1.  ACF_HIP_E_NOPLAN: no plan.  Not covered: a streaming front end for views, a fill value other than border
 * replication, perspective maps, area-exact reduction (samples is the anti-aliasing). */
ACF_HIP_API int acf_hip_pyramid_view(acf_hip_ctx* ctx, const acf_hip_crop_source* src, const float* views_dev /* [n_views][6] */,
    const int32_t* frame_dev /* [n_views], or NULL: view i reads stored frame i */, int n_views, int samples);
ACF_HIP_API int acf_hip_run_view(acf_hip_ctx* ctx, const acf_hip_crop_source* src, const float* views_dev /* [n_views][6] */,
    const int32_t* frame_dev /* [n_views], or NULL */, int n_views, int samples);
ACF_HIP_API int acf_hip_view_from_box(const float box[4] /* x, y, w, h in U */, double angle_rad, int h, int w, float m[6]);
ACF_HIP_API int acf_hip_view_quad(const float m[6], const int32_t det[4] /* x, y, w, h of the view's frame */, float quad[8] /* TL, TR, BR, BL in U */);
ACF_HIP_API int acf_hip_view_box(const float m[6], const int32_t det[4], float box[4] /* the quad's bounding box in U */);
ACF_HIP_API int acf_hip_view_form(const float m[6], int samples, int tile_x, int tile_y, int h, int w, int Hu, int Wu, int channels, int sample_bytes,
    int* form);

/* ---- merging the views' detections into the stored frame ----------------
 * After acf_hip_run_view every view of the batch holds a list of its own, in VIEW coordinates, and the device NMS (acf_hip_set_nms) has
 * worked per view.  acf_hip_merge_views maps every detection into the upright stored frame U on the device and suppresses the same
 * object found under neighbouring angles or in overlapping windows ACROSS the views of one stored frame; its boxes_out / frames_out
 * are what acf_hip_cut_crops takes, so a batch of views goes to crops of the merged detections without a device-to-host copy.
 *
 * The rule.  Every f64 operation rounded once, none fused.  For stored frame f = 0 .. n_frames - 1:
 *  1. Concatenate: the views i with frame(i) == f in ascending i (frame(i) = frame_dev[i], or i when frame_dev is NULL; a view whose
 *     index lies outside [0, n_frames) belongs to no frame), each view's list in its device order — the list acf_hip_cut_detections
 *     would read: the per-view NMS survivors when acf_hip_set_nms is on, else the raw list.  View i contributes c_i entries.  A
 *     contributing view with c_i < 0 (per-view NMS over capacity) or c_i > max_hits (an overflowed list, whose retained set is
 *     unspecified), or a total above ACF_HIP_NMS_CAP, makes the frame unknowable: counts_out[f] = -1 and no record.
 *  2. Map: box = acf_hip_view_box(views[i], det) (the four corners in f64 from the f32 view and the int box, the extremes of the
 *     unrounded corners, each member rounded to f32), quad = acf_hip_view_quad's.  An entry whose box has a non-finite member, or
 *     not (w > 0 and h > 0), is dropped: what a degenerate or NaN view gives.
 *  3. nms.type 0: the remaining entries in concatenation order; every other field of nms is ignored.
 *  4. nms.type 1 / 2: bbNms's rule (acf_hip_nms_params) on the float boxes.  Entries with double(score) < thr are dropped; the rest are
 *     ordered by descending score, equal scores keeping concatenation order (view, then index).  In f64: xs = x, xe = x + w, ys = y,
 *     ye = y + h, area = w * h.  For i in order (type 2: only a surviving i) every later j: iw = min(xe_i, xe_j) - max(xs_i, xs_j),
 *     ih alike; if iw > 0 and ih > 0: o = iw * ih, u = ovrDnmUnion ? (area_i + area_j) - o : min(area_i, area_j), and j is suppressed
 *     when o / u > overlap.  Then prune as ObjectDetector::prune (ObjectDetector.cpp:28-44).  For views that are integer
 *     translations every quantity is an integer held exactly: the rule is bbNms on the translated int boxes.
 *  5. Output, S survivors: counts_out[f] = S, the true number even when it exceeds K = max_per_frame.  Slots f * K + 0 .. min(S, K) - 1
 *     of out, quads_out and boxes_out hold the survivors in order; the box of boxes_out is grown by acf_hip_crop_box's f32 steps (cx = x
 *     + w * 0.5f, w' = w * grow, x' = cx - w' * 0.5f, y alike); frames_out there = f.  EVERY remaining slot of boxes_out and frames_out
 *     is written too, with zeros and -1 (an unknowable frame: all K of them), so that
 *         acf_hip_cut_crops(src, boxes_out, frames_out, n_frames * K, spec, dst)
 *     is legal straight away and gives crops of zeros beyond the count: nothing uninitialised is read and no count comes to the host.
 *     Record and quad slots beyond the count are not written.
 *  acf_hip_merge_views      on the detections of the context's last acf_hip_run_view (n_views that call's; views_dev and frame_dev the
 *                           ones it was given).  Asynchronous on the context's stream; allocates nothing, never waits for the device,
 *                           changes no context state (acf_hip_get_detections answers as before, acf_hip_cut_detections keeps
 *                           refusing) and leaves a captured graph of acf_hip_run valid
 *  acf_hip_op_merge_views   the same kernel on host lists dets_host [n_views][max_hits] and counts_host [n_views], results to the host;
 *                           a context, no model, no plan (like acf_hip_op_nms).  max_hits >= 1.  The caller's outputs go to the device
 *                           first: a slot the kernel does not write keeps what it held
 * One kernel, k_merge_views (so named under option "profile"): one workgroup per stored frame, everything resident in LDS — the views'
 * counts prefix-summed into n_views + 1 offsets (hence n_views <= 1024), a concatenated index finding its (view, index) by binary search
 * there, then k_nms's keys, bitonic sort, suppression, compaction and prune.
 * ACF_HIP_E_INVALID: null required pointers; n_views outside 1 .. 1024; n_frames < 1; max_per_frame outside 1 .. ACF_HIP_NMS_CAP; grow
 * not positive finite; nms.type outside 0 .. 2, nms.overlap NaN, nms.maxCount < 0 with prune; reserved not 0; merge_views without a
 * preceding acf_hip_run_view or with another n_views.  ACF_HIP_E_UNSUPPORTED: option "streams" > 1.  What needs no device is checked
 * before anything touches it.  Not covered: the overlap of the rotated quads themselves (the merged box is the quad's bounding box),
 * merging across stored frames, a host fallback for an unknowable frame (the -1 is the answer). */
typedef struct acf_hip_merged_detection {     /* 32 bytes */
    float x, y, w, h;          /* acf_hip_view_box(views[view], det): the bounding box of the quad in U */
    float score;
    int32_t view;              /* which view of the batch found it */
    int32_t index;             /* its position in that view's device list */
    int32_t scale;
} acf_hip_merged_detection;
typedef struct acf_hip_merge_spec {
    acf_hip_nms_params nms;    /* applied ACROSS the views of one stored frame */
    int32_t max_per_frame;     /* K, 1 .. ACF_HIP_NMS_CAP */
    float grow;                /* boxes_out only: acf_hip_crop_box's grow arithmetic; positive finite */
    int32_t reserved[2];       /* 0 */
} acf_hip_merge_spec;
ACF_HIP_API int acf_hip_merge_views(acf_hip_ctx* ctx, const float* views_dev /* [n_views][6] */, const int32_t* frame_dev /* [n_views], or NULL */,
    int n_views, int n_frames, const acf_hip_merge_spec* spec, acf_hip_merged_detection* out_dev /* [n_frames][K] */,
    int32_t* counts_out_dev /* [n_frames] */, float* boxes_out_dev /* [n_frames][K][4], or NULL */, int32_t* frames_out_dev /* [n_frames][K], or NULL */,
    float* quads_out_dev /* [n_frames][K][8], or NULL */);
ACF_HIP_API int acf_hip_op_merge_views(acf_hip_ctx* ctx, const acf_hip_detection* dets_host /* [n_views][max_hits] */, const int32_t* counts_host /* [n_views] */,
    int max_hits, const float* views_host /* [n_views][6] */, const int32_t* frame_host /* [n_views], or NULL */, int n_views, int n_frames,
    const acf_hip_merge_spec* spec, acf_hip_merged_detection* out /* [n_frames][K] */, int32_t* counts_out /* [n_frames] */,
    float* boxes_out /* [n_frames][K][4], or NULL */, int32_t* frames_out /* [n_frames][K], or NULL */, float* quads_out /* [n_frames][K][8], or NULL */);

/* ---- a bank of classifiers on one pyramid -------------------------------
 * A context holds one classifier (acf_hip_set_model: model 0, the primary).  A bank adds up to ACF_HIP_BANK_MAX members — frontal and
 * profile faces, a face model beside a pedestrian model, two aspect ratios of one class — that are evaluated on the pyramid the
 * primary's parameters built: one pyramid, several cascades.
 *
 * A member is a classifier with its own window and cascade fields (nTrees, nTreeNodes, treeDepth 0 .. 8, fids / thrs / hs / child,
 * modelDs, modelDsPad, stride, cascThr).  Every pyramid and channel field (nPerOct, nOctUp, nApprox, nLambdas, lambdas, pad, minDs,
 * smooth; shrink, colorEnabled, colorSmooth, colorSpace, gradMagEnabled, colorChn, normRad, normConst, full, gradHistEnabled, binSize,
 * nOrients, softBin, isLuv) must equal the primary's: the pyramid is then, bit for bit, the one a context with the member as its only
 * model would build.
 *  acf_hip_bank_check       host only, no context: ACF_HIP_OK, or the refusal with its reason in why[cap] — ACF_HIP_E_UNSUPPORTED for
 *                           ldcfK > 0 on either side; ACF_HIP_E_INVALID for a deviating pyramid / channel field and for whatever
 *                           acf_hip_check_model(member, nChns, ..) refuses, nChns derived from the channel fields (so: a feature id
 *                           beyond nChns x the member's window cells, a bad child[])
 *  acf_hip_set_bank         needs a model; checks every member, copies its arrays, and drops the plan (as acf_hip_set_model does).
 *                           n = 0 or members = NULL clears the bank.  acf_hip_set_model clears it too: the members were checked against
 *                           the previous primary.  acf_hip_plan then builds for every member what it builds for the primary's cascade
 *                           — the window grid over the plan's levels from the member's modelDsPad and stride (a level smaller than
 *                           the window has none), the cascade tables with a rank set, the run buffers for max_hits hits per frame, the
 *                           box table from the member's modelDs.  Nothing is allocated after the plan.  acf_hip_set_option reaches the
 *                           members; under option "profile" their launches are part of acf_hip_profile_get
 *  acf_hip_get_bank_levels  the plan's levels with model `model`'s window grid (nWinR, nWinC); model 0: acf_hip_get_levels'
 *  acf_hip_detect_bank      every member's cascade on the pyramid of the last batch, asynchronously on the context's stream, after any
 *                           acf_hip_pyramid* / acf_hip_run* entry.  Member m's list is, bit for bit — hits, score bits, boxes, order —,
 *                           what a context holding member m as its only model gives from acf_hip_run on the same frames.  The
 *                           existing cascade kernels run, on a state of the member's own: its rank cells come from its own k_rank
 *                           launch over the float pyramid wherever the member and the options admit them, else the float forms run;
 *                           all forms give identical results and acf_hip_get_bank_forms reports the one taken.  It changes nothing
 *                           the primary left (acf_hip_get_detections, acf_hip_cut_detections, acf_hip_merge_views answer as before; a
 *                           captured graph of acf_hip_run stays valid).  Members get no device NMS of their own: their lists are raw.
 *                           ACF_HIP_E_INVALID without a bank, a plan or a valid pyramid, and when the float pyramid of the batch was
 *                           not written (option "keep_pyramid" = 0 with a primary on rank cells); ACF_HIP_E_UNSUPPORTED with option
 *                           "streams" > 1
 *  acf_hip_get_bank_detections / _hits   model `model`'s list of one frame after acf_hip_detect_bank, as acf_hip_get_raw_detections /
 *                           acf_hip_get_hits return a list (model 0: exactly those two entries)
 *  acf_hip_get_bank_forms   model `model`'s ACF_HIP_CF_* record of its last cascade (model 0: acf_hip_get_cascade_forms')
 *
 * Joining the lists.  For frame f = 0 .. n_frames - 1:
 *  1. Concatenate: model 0's raw list (what acf_hip_get_raw_detections returns, whether or not the device NMS is on), then members
 *     1 .. n in order, each list in its device order (scale, column, row).  A list with a count above max_hits (an overflowed list,
 *     whose retained set is unspecified) or below 0, or a total above ACF_HIP_NMS_CAP, makes the frame unknowable: counts_out[f] = -1
 *     and no record.
 *  2. nms.type 0: the entries in concatenation order; every other field of nms, and separate, is ignored.
 *  3. nms.type 1 / 2: k_nms's rule (acf_hip_nms_params, acf_hip_op_nms) on the int boxes.  Entries with double(score) < thr are dropped;
 *     the rest are ordered by descending score, equal scores keeping concatenation order (model, then index); the suppression loop
 *     (type 2: only a surviving i suppresses) with the overlap from int products, the quotient in f64; then prune.  separate = 0: every
 *     pair is tested, so the same object found by two models is reported once.  separate = 1: only detections of the same model
 *     suppress each other — the survivors are the union of the per-model acf_hip_op_nms survivors; the output order is still the
 *     joint score order and prune is joint.
 *  4. Output, S survivors: counts_out[f] = S, the true number even when it exceeds K = max_per_frame.  Slots f * K + 0 .. min(S, K) - 1
 *     of out and boxes_out hold the survivors in order; boxes_out = acf_hip_crop_box(det, det_scale, grow) with the same f32
 *     operations; frames_out there = f.  EVERY remaining slot of boxes_out and frames_out is written too, with zeros and -1 (an
 *     unknowable frame: all K of them), so that acf_hip_cut_crops(src, boxes_out, frames_out, n_frames * K, spec, dst) is legal
 *     straight away.  Record slots beyond the count are not written.
 *  acf_hip_join_bank        on the lists of the last acf_hip_run* + acf_hip_detect_bank (n_frames that batch's).  Asynchronous on the
 *                           context's stream; allocates nothing, never waits for the device, changes no context state
 *  acf_hip_op_join_bank     the same kernel on host lists dets_host [n_models][n_frames][max_hits] and counts_host
 *                           [n_models][n_frames], results to the host; a context, no model, no plan.  n_models 1 .. ACF_HIP_BANK_MAX + 1,
 *                           max_hits >= 1.  The caller's outputs go to the device first: a slot the kernel does not write keeps what
 *                           it held
 * One kernel, k_join_bank (so named under option "profile"): one workgroup per frame, everything resident in LDS, k_nms's keys, sort,
 * compaction and prune.
 * ACF_HIP_E_INVALID: null required pointers; max_per_frame outside 1 .. ACF_HIP_NMS_CAP; grow not positive finite; nms.type outside
 * 0 .. 2, nms.overlap NaN, nms.maxCount < 0 with prune; reserved not 0; separate outside {0, 1}; det_scale not 0 or positive finite;
 * join_bank without detections of the primary and an acf_hip_detect_bank since the last pyramid.  ACF_HIP_E_UNSUPPORTED: option
 * "streams" > 1.  What needs no device is checked before anything touches it.  Not covered: members with pyramid fields of their own,
 * LDCF members, a per-model device NMS, bank records in the streaming front end. */
#define ACF_HIP_BANK_MAX 8   /* members; model indices 0 (the context's model) .. 8 */
typedef struct acf_hip_bank_detection {      /* 32 bytes */
    int32_t x, y, w, h;
    float score;
    int32_t scale;
    int32_t model;             /* 0: the context's model; m >= 1: member m - 1 of acf_hip_set_bank */
    int32_t index;             /* its position in that model's device list */
} acf_hip_bank_detection;
typedef struct acf_hip_bank_spec {
    acf_hip_nms_params nms;    /* applied ACROSS the models of one frame (separate = 1: within each model) */
    int32_t separate;          /* 0 / 1 */
    int32_t max_per_frame;     /* K, 1 .. ACF_HIP_NMS_CAP */
    float grow;                /* boxes_out only: acf_hip_crop_box's grow; positive finite */
    double det_scale;          /* boxes_out only: acf_hip_crop_box's det_scale; 0 (no resize) or positive finite */
    int32_t reserved[2];       /* 0 */
} acf_hip_bank_spec;
ACF_HIP_API int acf_hip_bank_check(const acf_hip_params* primary, const acf_hip_params* member, char* why, int cap);
ACF_HIP_API int acf_hip_set_bank(acf_hip_ctx* ctx, const acf_hip_params* members, int n);
ACF_HIP_API int acf_hip_get_bank_levels(const acf_hip_ctx* ctx, int model, acf_hip_level* out, int cap);
ACF_HIP_API int acf_hip_detect_bank(acf_hip_ctx* ctx);
ACF_HIP_API int acf_hip_get_bank_detections(acf_hip_ctx* ctx, int model, int frame, acf_hip_detection* out, int cap, int* count);
ACF_HIP_API int acf_hip_get_bank_hits(acf_hip_ctx* ctx, int model, int frame, acf_hip_hit* out, int cap, int* count);
ACF_HIP_API int acf_hip_get_bank_forms(const acf_hip_ctx* ctx, int model, int32_t* out, int cap, int* n);
ACF_HIP_API int acf_hip_join_bank(acf_hip_ctx* ctx, const acf_hip_bank_spec* spec, acf_hip_bank_detection* out_dev /* [n_frames][K] */,
    int32_t* counts_out_dev /* [n_frames] */, float* boxes_out_dev /* [n_frames][K][4], or NULL */, int32_t* frames_out_dev /* [n_frames][K], or NULL */);
ACF_HIP_API int acf_hip_op_join_bank(acf_hip_ctx* ctx, const acf_hip_detection* dets_host /* [n_models][n_frames][max_hits] */,
    const int32_t* counts_host /* [n_models][n_frames] */, int n_models, int n_frames, int max_hits, const acf_hip_bank_spec* spec,
    acf_hip_bank_detection* out /* [n_frames][K] */, int32_t* counts_out /* [n_frames] */, float* boxes_out /* [n_frames][K][4], or NULL */,
    int32_t* frames_out /* [n_frames][K], or NULL */);

/* ---- streaming front end ---------------------------------------------
 * The overlap of transfer and compute that GPUDetectionPipeline::runFast gets
 * from its two-frame texture FIFO (GPUDetectionPipeline.cpp:357-437), expressed
 * with HIP streams and events: batch k+1 is copied host->device on a copy
 * stream while batch k runs on the context's stream; results come back as the
 * fixed-capacity records of acf_hip_export_detections in pinned host memory.
 *
 *   acf_hip_stream_open(ctx, pix, stride, cap, depth)   depth = batches in flight (2..8)
 *   acf_hip_stream_submit(ctx, frames_host, n, &ticket)  returns at once (frames_host pinned: see acf_hip_host_alloc)
 *   acf_hip_stream_collect(ctx, ticket, &records, &n)    waits for that batch only
 *
 * Tickets must be collected in order; `records` stays valid until `depth` more
 * batches have been submitted.  `frames_host` must stay untouched until its
 * ticket is collected. */
ACF_HIP_API int acf_hip_stream_open(acf_hip_ctx* ctx, int pix, int row_stride_bytes, int cap, int depth);
ACF_HIP_API int acf_hip_stream_submit(acf_hip_ctx* ctx, const uint8_t* frames_host, int n_frames, int* ticket);
ACF_HIP_API int acf_hip_stream_collect(acf_hip_ctx* ctx, int ticket, const int32_t** records, int* n_frames);
ACF_HIP_API int acf_hip_stream_close(acf_hip_ctx* ctx);
/* Page-locked host memory for acf_hip_stream_submit / acf_hip_run_host callers that do not link HIP. */
ACF_HIP_API int acf_hip_host_alloc(size_t bytes, void** out);
ACF_HIP_API int acf_hip_host_free(void* p);

/* Wait for the stream, then return frame `frame`'s detections in the
 * reference's order (level ascending, then c, then r; ACF.cpp:326-329,
 * acfDetect1.cpp:86-96).  `*count` is the true number even if > cap. */
/* params != NULL: from the next acf_hip_detect / acf_hip_run* on, every frame's detections go through bbNms (+ prune)
 * on the device, and acf_hip_get_detections / acf_hip_export_detections / the stream records return the survivors, in
 * score order (Detector::operator(), ACF.cpp:332-353).  NULL: back to the raw list (scale, column, row order). */
ACF_HIP_API int acf_hip_set_nms(acf_hip_ctx* ctx, const acf_hip_nms_params* params);
/* bbNms + prune of one host list: boxes [n][4] = {x, y, w, h}, f64 scores; keep_idx receives the indices of the survivors
 * in output order (capacity n), *count their number.  n <= ACF_HIP_NMS_CAP. */
ACF_HIP_API int acf_hip_op_nms(acf_hip_ctx* ctx, const int32_t* boxes, const double* scores, int n, const acf_hip_nms_params* params,
    int32_t* keep_idx, int* count);
ACF_HIP_API int acf_hip_get_detections(acf_hip_ctx* ctx, int frame, acf_hip_detection* out, int cap, int* count);
/* The cascade's hits behind the detections: hit i is the window that produced detection i of acf_hip_get_detections (with
 * the device NMS on: the survivors' windows, in the survivors' order; *count = their number). */
ACF_HIP_API int acf_hip_get_hits(acf_hip_ctx* ctx, int frame, acf_hip_hit* out, int cap, int* count);
/* The list acfDetect1 produced (ACF.cpp:302-329: scale, column, row order) whether or not the device NMS is on.  The device
 * NMS takes at most ACF_HIP_NMS_CAP detections per frame; beyond that acf_hip_get_detections returns ACF_HIP_E_CAPACITY for the
 * frame (record count -1) and the caller suppresses this list on the host (acf::HipDetector does; bbNms.cpp has no limit). */
ACF_HIP_API int acf_hip_get_raw_detections(acf_hip_ctx* ctx, int frame, acf_hip_detection* out, int cap, int* count);

/* Device-side export for the multi-GPU gather: writes, for every frame of the
 * last batch, a fixed-capacity record [count, then cap x {x,y,w,h,score bits,scale}]
 * of int32 into `dst_dev` (n_frames * (1 + 6*cap) int32), sorted as above. */
ACF_HIP_API int acf_hip_export_detections(acf_hip_ctx* ctx, int32_t* dst_dev, int cap);

ACF_HIP_API int acf_hip_synchronize(acf_hip_ctx* ctx);
/* With option "count_repairs" = 1 (measurements: it synchronises after every verification): out = {image planes whose
 * smoothing segments were checked, of those recomputed as one chain, level planes checked, recomputed} since the context
 * was created — how often the speculative column segments (options smooth_segments / smooth_warm / level_warm) miss. */
ACF_HIP_API int acf_hip_get_repairs(acf_hip_ctx* ctx, int64_t out[4]);
/* Read-only: the form convTri(M, normRad) took at every real scale in the last acf_hip_pyramid / acf_hip_run* call (0 before the
 * first).  out[i] for real scale i (at most `cap`; *n = their number): bit 0 = the x pass left checkpoints which the y kernel
 * replayed (no plane U travels through memory), bit 1 = the context holds a plane U for that scale (it is allocated only when a
 * call first takes a form that reads it).  Additive: ACF_HIP_ABI_VERSION stays. */
ACF_HIP_API int acf_hip_get_tri_forms(const acf_hip_ctx* ctx, int32_t* out, int cap, int* n);
/* Read-only: what the level stage (approximated levels, final smoothing, placement, rank cells) decided, written down where the plan
 * and the last acf_hip_pyramid / acf_hip_run* call decided it.  *n = ACF_HIP_LF_HEAD + number of levels; at most `cap` words are
 * written.  Call-wide, of the last call (zeros before the first): out[0] = path (ACF_HIP_LV_*), out[1] = the level kernels wrote the
 * rank cells, out[2] = they wrote floats, out[3] = column segments of k_level_all's first launch (0: it did not run), out[4] =
 * k_resample(approx) ran first, out[5] = number of levels.  out[ACF_HIP_LF_HEAD + i], level i, of the job list that path reads (the
 * plan's fused list before the first call and on the paths that run no level kernel): bits 0-7 rows per lane R, bits 8-10 the mode
 * (0 real, 1 x and y down, 2 x down y up, 3 x up y down, 4 x and y up), bits 12-13 who takes the level (ACF_HIP_LF_BY_*), and from bit
 * 16 the reasons this level gives the plan not to fuse (ACF_HIP_LF_WHY_*; all clear on every level: the plan can).  With a batch
 * that the call cut into launches of their own (image-specific lambdas) the words are those of the launches: they all share one
 * plan.  Additive: ACF_HIP_ABI_VERSION stays. */
#define ACF_HIP_LF_HEAD 6
#define ACF_HIP_LV_FUSED 0       /* k_level_all + k_level groups resample, smooth and place every level */
#define ACF_HIP_LV_WAVE_SMOOTH 1 /* the same kernels smooth and place what a separate k_resample approximated */
#define ACF_HIP_LV_SMOOTH_JOBS 2 /* the tiled smoothing kernels over every level */
#define ACF_HIP_LV_COPY 3        /* no smoothing: plane copies */
#define ACF_HIP_LF_BY_NONE 0     /* no level kernel (paths 2 and 3) */
#define ACF_HIP_LF_BY_ALL 1      /* k_level_all */
#define ACF_HIP_LF_BY_GROUP 2    /* a k_level<R, mode> group launch */
#define ACF_HIP_LF_WHY_TAPS (1 << 16)   /* more than three taps on an axis */
#define ACF_HIP_LF_WHY_EXACT (1 << 17)  /* an exact 1/k ratio on an axis */
#define ACF_HIP_LF_WHY_ROWS (1 << 18)   /* an approximated level of more than 8 rows per lane */
#define ACF_HIP_LF_WHY_WINDOW (1 << 19) /* more source rows than the level kernel's window holds */
#define ACF_HIP_LF_WHY_TALL (1 << 20)   /* taller than the tallest level kernel */
#define ACF_HIP_LF_WHY_MIXED (1 << 21)  /* one axis up, the other down */
ACF_HIP_API int acf_hip_get_level_forms(const acf_hip_ctx* ctx, int32_t* out, int cap, int* n);
/* Read-only: how every real scale's image was resampled, written down where it is decided: the route and the launch by the last
 * acf_hip_pyramid / acf_hip_run* call (zero before the first), the plan's side by acf_hip_plan.  out[i] for real scale i (at most
 * `cap`; *n = their number):
 *   bits 0-3   the route (ACF_HIP_SF_ROUTE_*)
 *   bit 4      the launch was a SLOW instantiation of k_resample_strip (an output with more than four y taps)
 *   bit 5      the generic k_resample ran with 2 columns per wave (else RS_XT)
 *   bit 6, 7   the plan holds a strip plan of this scale alone / of this scale together with the next one
 *   bits 8-15  nty, bits 16-23 nSplit: the row tiles and column segments of the k_resample_strip launch this scale made (routes
 *              STRIP and STRIP_PAIR_A; 0 otherwise — PAIR_B made no launch of its own)
 *   bits 24-27 why the plan of this scale alone was refused, bits 28-31 why the plan of the pair was (ACF_HIP_SF_WHY_*; 0: not
 *              refused, or no plan was asked for)
 * Additive: ACF_HIP_ABI_VERSION stays. */
#define ACF_HIP_SF_ROUTE_NONE 0         /* not resampled: the frame itself */
#define ACF_HIP_SF_ROUTE_HALF_FUSED 1   /* written by the previous scale's k_smooth_vec (its exact half) */
#define ACF_HIP_SF_ROUTE_PAIR_B 2       /* output B of the previous scale's k_resample_strip<true, .> */
#define ACF_HIP_SF_ROUTE_STRIP 3        /* k_resample_strip<false, .> */
#define ACF_HIP_SF_ROUTE_STRIP_PAIR_A 4 /* k_resample_strip<true, .>, which wrote the next scale as well */
#define ACF_HIP_SF_ROUTE_HALF 5         /* k_resample_half */
#define ACF_HIP_SF_ROUTE_UP 6           /* k_resample_up */
#define ACF_HIP_SF_ROUTE_GENERIC 7      /* k_resample */
#define ACF_HIP_SF_SLOW (1 << 4)
#define ACF_HIP_SF_XT2 (1 << 5)
#define ACF_HIP_SF_PLAN_STRIP (1 << 6)
#define ACF_HIP_SF_PLAN_PAIR (1 << 7)
#define ACF_HIP_SF_WHY_NOT_DOWN 1       /* an axis up-sampled */
#define ACF_HIP_SF_WHY_ROWS 2           /* source rows not a multiple of 4, or fewer than 8 */
#define ACF_HIP_SF_WHY_ALIGN 3          /* the source planes are not 16-byte aligned */
#define ACF_HIP_SF_WHY_PAIR_MISMATCH 4  /* the two outputs do not share their source */
#define ACF_HIP_SF_WHY_SLOW_TAPS 5      /* more than 8 y taps, or taps further than 15 rows apart */
#define ACF_HIP_SF_WHY_X_TAPS 6         /* more than 4 x taps */
#define ACF_HIP_SF_WHY_B_STEPS 7        /* output B needs more column steps than output A */
#define ACF_HIP_SF_WHY_NO_TILING 8      /* no row tiling fits the kernel's LDS, item and chunk bounds */
ACF_HIP_API int acf_hip_get_scale_forms(const acf_hip_ctx* ctx, int32_t* out, int cap, int* n);
/* Read-only: what the last cascade call of this context decided (planCascadeCall's record, copied where runCascade made it): the
 * cascade of acf_hip_detect / acf_hip_run*, or of acf_hip_op_acf_detect1* — whichever ran last; all zero before the first and
 * again after acf_hip_plan.  Needs no plan.  *n = ACF_HIP_CF_WORDS; at most `cap` words are written:
 *   [0] path (ACF_HIP_CF_PATH_*)            [1] rank cells stood for the floats      [2] the tile kernel (ACF_HIP_CF_TILE_*)
 *   [3] NW  [4] TR  [5] TC  [6] passW  [7] pooled  [8..12] b[0..4]  [13] nTiles: the geometry of the tile set that kernel ran on
 *                                            (zero without a tile kernel)
 *   [14] workgroups of the tile launch       [15] they were persistent                [16] its dynamic LDS in bytes
 *   [17] nStages  [18..21] bounds  [22] firstStage  [23] mode: the staged path's stages (zero on the other paths)
 *   [24] codeScan (leaf codes + ordered scan)  [25] pooledTail (k_cascade_tile3D wrote the codes)  [26] waveTail (a wave per entry)
 *   [27] codes.cap  [28] qcap                [29] frames of the call
 * Additive: ACF_HIP_ABI_VERSION stays. */
#define ACF_HIP_CF_WORDS 30
#define ACF_HIP_CF_PATH_NONE 0   /* no windows */
#define ACF_HIP_CF_PATH_TILED2 1 /* depth 2: k_cascade_tile3 + its tails */
#define ACF_HIP_CF_PATH_STAGED 2 /* k_cascade_first / _queue / _tail, for depths 1, 3, 4 with a tile kernel in front */
#define ACF_HIP_CF_TILE_NONE 0
#define ACF_HIP_CF_TILE_3 1      /* k_cascade_tile3 */
#define ACF_HIP_CF_TILE_3D 2     /* k_cascade_tile3D */
#define ACF_HIP_CF_TILE_D 3      /* k_cascade_tileD */
ACF_HIP_API int acf_hip_get_cascade_forms(const acf_hip_ctx* ctx, int32_t* out, int cap, int* n);
/* Host only (tests): the checkpoint buffer of an h x w plane — out[0] = float index of the (T, U) pair that row y's replay of the
 * 16-column segment holding column x starts from, out[1] = floats per frame.  Per frame
 * [x >> 6][(y + 8) >> 4][(x >> 4) & 3][(y + 8) & 15][2]: the 16 rows x 4 segments a wave of the y kernel takes per step are 512
 * contiguous bytes; the state is the one after column (x & ~15) - 1, for segment 0 the one after column 0. */
ACF_HIP_API int acf_hip_tri_ck_layout(int h, int w, int x, int y, int64_t out[2]);

/* Per-kernel timing with HIP events recorded on the context's stream (option
 * "profile" = 1): the counterpart of the reference's ScopeTimeLogger stage
 * timers (GPUDetectionPipeline.cpp:366,415,485).  Synchronises, then returns
 * up to `cap` kernel names (static strings), their accumulated milliseconds and
 * launch counts since the last call, and resets the accumulation. */
ACF_HIP_API int acf_hip_profile_get(acf_hip_ctx* ctx, int* n, const char** names, float* ms, int* launches, int cap);

/* ---- parity taps (tests only; not on the timed path) ------------------ */

/* Copy level `level` of frame `frame`'s fused pyramid ([nChns][wP][hP]) to host. */
ACF_HIP_API int acf_hip_read_level(acf_hip_ctx* ctx, int frame, int level, float* host_out);
/* The same level as the 16-bit threshold-rank cells the cascade read ([nChns][wP][hP], after acf_hip_detect / acf_hip_run
 * with "rank_cells" on and a model that admits them; ACF_HIP_E_UNSUPPORTED otherwise). */
ACF_HIP_API int acf_hip_read_rank_level(acf_hip_ctx* ctx, int frame, int level, uint16_t* host_out);
/* Host only, no context: the rank cells of `n` values of channel `chn` and the rank indices of every node threshold, as
 * acf_hip_plan builds them for this model (`nChns` channels).  rank(v) = number of distinct node thresholds t of the
 * channel with t <= v; node q's index is k + 1 where t_k is its threshold, so that v < thrs[q]  <=>  rank(v) < index[q].
 * cells_out[n]; thr_index_out[nTrees * nTreeNodes] (0 for leaves); either may be NULL.  info[4] = {usable, shift, buckets,
 * distinct thresholds} of the channel.  ACF_HIP_E_UNSUPPORTED when the model's thresholds do not admit the table. */
ACF_HIP_API int acf_hip_rank_cells_host(const acf_hip_params* params, int nChns, int chn, const float* v, int n, uint16_t* cells_out,
    uint32_t* thr_index_out, int32_t* info);

enum {
    ACF_HIP_TAP_IMAGE = 0,    /* resampled image at a real scale, before smoothing: d planes */
    ACF_HIP_TAP_SMOOTHED = 1, /* after convTri (logger tags L,U,V chnsCompute.cpp:241-250) */
    ACF_HIP_TAP_M = 2,        /* gradMag before normalisation (tag M, gradientMag.cpp:112-117) */
    ACF_HIP_TAP_O = 3,        /* orientation (tag O) */
    ACF_HIP_TAP_S = 4,        /* convTri(M, normRad) */
    ACF_HIP_TAP_MNORM = 5,    /* tag Mnorm */
    ACF_HIP_TAP_CHNS = 6,     /* unsmoothed, unpadded channels of a level: nChns planes [wC][hC] */
    ACF_HIP_TAP_LDCF = 7      /* LDCF level the cascade reads: nChns*k planes [round(wP/2)][round(hP/2)] (after acf_hip_detect) */
};
/* `index`: real-scale ordinal for taps 0-5, level for ACF_HIP_TAP_CHNS.  With five input planes, M, O, S and MNORM do not exist
 * at ordinal 0 (the frame brought M and O; nothing is computed and the reference logs none of them, chnsCompute.cpp:265-269):
 * ACF_HIP_E_INVALID. */
ACF_HIP_API int acf_hip_read_tap(acf_hip_ctx* ctx, int frame, int tap, int index, float* host_out, int64_t cap_floats);

/* ---- single operators on host planes ---------------------------------
 * The reference exposes these as static members of acf::Detector
 * (ACF.h:441-493) and as free functions; each runs the same HIP kernel the
 * pyramid uses, on one plane set, synchronously. */

/* Detector::rgbConvert (rgbConvert.cpp:101-170) flag = ACF_HIP_CS_LUV or GRAY. */
ACF_HIP_API int acf_hip_op_rgb_convert(acf_hip_ctx* ctx, const float* in, float* out, int h, int w, int flag);
/* Detector::convTri (convTri.cpp:204-253): r in (0,1] -> convTri1 with the
 * reference's in-place aliasing semantics when `aliased` != 0; r > 1 -> convTri. */
ACF_HIP_API int acf_hip_op_conv_tri(acf_hip_ctx* ctx, const float* in, float* out, int h, int w, int d, double r, int aliased);
/* Detector::gradientMag (gradientMag.cpp:102-135). S_out may be NULL. */
ACF_HIP_API int acf_hip_op_gradient_mag(acf_hip_ctx* ctx, const float* in, float* M, float* O, float* S_out,
    int h, int w, int normRad, double normConst, int full);
/* Self-check of the gradMag kernels' fast form of m = min(1/sqrt(m2), 1e10), M = 1/m (one v_rsq_f32 + FMA refinements)
 * against the IEEE sqrt and divisions it stands for (gradientMex.cpp:209-219 with exact arithmetic), on the device, for
 * every float bit pattern first_bits .. last_bits taken as m2: *mismatches = how many differ in either result,
 * *first_bad_bits = the smallest such pattern.  0 .. 0x7f7fffff (every finite m2 >= 0) must give 0. */
ACF_HIP_API int acf_hip_selftest_gradmag(acf_hip_ctx* ctx, uint32_t first_bits, uint32_t last_bits, uint64_t* mismatches, uint32_t* first_bad_bits);
/* Detector::chnsCompute (ACF.h:342-349, chnsCompute.cpp:146-338; addChn :340-370): the channels of ONE image at its own scale,
 * without a pyramid plan — crop to a multiple of shrink (:203-217), rgbConvert (:235; skipped for colorSpace orig / rgb, for
 * isLuv and for a 1-plane image), convTri(I, I, pColor.smooth, 1) in place (:239), gradientMag with its normalisation (:263-283),
 * gradientHist (:310-331), every enabled type reduced by `shrink` (addChn's imResample) and concatenated: colour, magnitude,
 * histogram.
 *   p     the Options::Pyramid::Chns fields of acf_hip_params are read (shrink .. isLuv; classifier and pyramid fields ignored);
 *         NULL: the context's model (acf_hip_set_model)
 *   in    HOST planes [d][w][h], d = 1 or 3 — or 5: three image planes followed by the gradient magnitude and orientation that came
 *         with the image (chnsCompute.cpp:219-226: they replace gradientMag and its normalisation, verbatim whatever colorSpace and
 *         normRad say) —, the transposed planar layout.  d = 1 (colorSpace gray or orig, colorChn 0) is its own single colour plane
 *         (rgbConvert.cpp:129-148): nChns = 1 + 1 + nOrients with every type on; unlike acf_hip_plan, which replicates it to three
 *         planes first (chnsPyramid.cpp:234-244).  d = 4 is refused on purpose (the reference would drop the lone extra plane)
 *   out   HOST buffer of `cap` floats receiving [nChns][w / shrink][h / shrink] (cropped sizes); NULL: only the sizes are reported
 * *nChns, *hC, *wC (each may be NULL) receive the channel count and the cell-plane size.  Honours option "arith". */
ACF_HIP_API int acf_hip_chns_compute(acf_hip_ctx* ctx, const acf_hip_params* p, const float* in, int h, int w, int d, float* out, int64_t cap,
    int* nChns, int* hC, int* wC);
/* Detector::gradientHist (gradientHist.cpp:92-115) -> gradHist (gradientMex.cpp:375-509): soft_bin even — >= 0 the magnitude
 * is shared between the two nearest orientation bins, < 0 the nearest bin takes it; no spatial interpolation.  Odd soft_bin
 * (trilinear: HOG / FHOG features) is ACF_HIP_E_UNSUPPORTED. */
ACF_HIP_API int acf_hip_op_gradient_hist(acf_hip_ctx* ctx, const float* M, const float* O, float* H,
    int h, int w, int bin, int nOrients, int soft_bin, int full);
/* imResample (imResampleMex.cpp:385-420). */
ACF_HIP_API int acf_hip_op_im_resample(acf_hip_ctx* ctx, const float* in, float* out, int ha, int wa, int hb, int wb, int d, double nrm);
/* Tests only: two imResample outputs of one source ([d][wa][ha] -> outA [d][wbA][hbA] and outB [d][wbB][hbB], B no larger than A
 * on either axis), planned and launched as the pyramid plans two real scales of one source: k_resample_strip's two-output form
 * where its plan holds, else each output as acf_hip_op_im_resample runs it.  *word says which: bits 0-3 = why the pair plan was
 * refused (ACF_HIP_SF_WHY_*); 0 and bits 8-15 non-zero = the pair was launched, with bit 4 = a SLOW instantiation, bits 8-15 nty,
 * 16-23 ntyB, 24-31 nSplit, 32-47 nSteps, 48-63 nStepsB.  Additive: ACF_HIP_ABI_VERSION stays. */
ACF_HIP_API int acf_hip_op_im_resample_pair(acf_hip_ctx* ctx, const float* in, float* outA, float* outB, int ha, int wa, int hbA, int wbA, int hbB, int wbB,
    int d, double nrm, uint64_t* word);
/* Detector::acfDetect1 on one host channel buffer [nChns][wP][hP] (acfDetect1.cpp:309-335). */
ACF_HIP_API int acf_hip_op_acf_detect1(acf_hip_ctx* ctx, const float* chns, int hP, int wP, int nChns,
    acf_hip_hit* out, int cap, int* count);
/* Tests only: the same call on 16-bit threshold-rank cells, as acf_hip_detect runs it on a plan's pyramid: the rank tables and the
 * rank tile set of the model are built for the buffer, k_rank makes the rank cells from the caller's floats, and the tile kernel
 * (and, depth 2, the tail) read only those.  ACF_HIP_E_UNSUPPORTED where no rank set can be built or the call would not read it
 * (option "rank_cells" or "cascade_tiles" off, a depth without a tile kernel, thresholds the rank tables do not admit): floats are
 * never run in its place.  Additive: ACF_HIP_ABI_VERSION stays. */
ACF_HIP_API int acf_hip_op_acf_detect1_rank(acf_hip_ctx* ctx, const float* chns, int hP, int wP, int nChns,
    acf_hip_hit* out, int cap, int* count);

/* The uint8_t body of acfDetect1 (ParallelDetectionBody<uint8_t,...>, acfDetect1.cpp:157-166,187-192) on one host
 * channel buffer of bytes [nChns][wP][hP], the format the reference's GL backend feeds the cascade (GPUACF.cpp:790).
 * `thrsU8`: Classifier::thrsU8 ([nTrees][nTreeNodes] bytes), or NULL to derive it from the model's thrs as the
 * loader does (ACFIOArchive.h:96-99, acf_hip_thrs_u8). */
ACF_HIP_API int acf_hip_op_acf_detect1_u8(acf_hip_ctx* ctx, const uint8_t* chns, int hP, int wP, int nChns, const uint8_t* thrsU8,
    acf_hip_hit* out, int cap, int* count);
/* Detector::evaluate(const MatP&, shrink, modelDsPad, stride) (ACF.h:543-544, acfDetect1.cpp:337-342): score of the single
 * window at (0,0) of one host channel buffer [nChns][wP][hP]; trees are added until the score is <= cascThr (the reference
 * passes 0 here) and the score reached is returned, whether or not the window would be a detection. */
ACF_HIP_API int acf_hip_op_evaluate(acf_hip_ctx* ctx, const float* chns, int hP, int wP, int nChns, double cascThr, float* score);
/* Detector::evaluate(const cv::Mat&) for a BATCH of crops (ACF.h:543, ACF.cpp:123-133 = computeChannels + evaluate(MatP),
 * acfDetect1.cpp:337-342) — how the reference's CLI classifies images of exactly the window's size (acf.cpp:350-355).  Hot path:
 * DEVICE pointers, on the context's stream, a model but no plan.  scores_dev[i] receives exactly the bits acf_hip_chns_compute(ctx,
 * chns, crop i, ..) followed by acf_hip_op_evaluate(ctx, channels, hC, wC, nChns, cascThr, ..) returns: the crop cut to a multiple
 * of shrink, rgbConvert with the same pass-through rules, the in-place convTri1 colour smoothing, gradientMag with its
 * normalisation, gradientHist, addChn's shrink, then the window at (0, 0), trees in order until the score is <= cascThr (the
 * reference passes 0).  Every tree depth 0..8; option "arith" is honoured.
 *   chns       the Options::Pyramid::Chns fields are read, as in acf_hip_chns_compute; NULL: the context's model.  (The reference's
 *              overload always computes the toolbox-default channels of computeChannels, ACF.cpp:183-236: pass those to mirror it.)
 *   crops_dev  n crops back to back, each [d][w][h] transposed planar f32, d = 1 or 3
 *   _u8        n upright packed images of h rows x w pixels in layout pix (ACF_HIP_PIX_RGB / BGR / RGBA / BGRA / GRAY; NV12 / NV21 are
 *              refused), row_stride_bytes apart (0 = tight), crops stride * h bytes apart; the bytes become planes by the 8-bit entries'
 *              arithmetic, float(v) * float(1 / 255.0)
 * Two forms, chosen by the crop's size alone, identical in every bit: crops whose planes fit one workgroup's LDS (80 x 80 x 3 and
 * 128 x 64 x 3 do) are scored by ONE kernel, k_crop_score, asynchronously and without allocating; bigger crops go as a batch of
 * frames through the kernels acf_hip_chns_compute launches and k_evaluate_windows — that form allocates its planes per call and
 * SYNCHRONISES the stream before it returns.  With option "profile" the form that ran reports under those two names.
 * ACF_HIP_E_NOMODEL without a model; ACF_HIP_E_INVALID for null pointers, n < 1, d not 1 or 3, a cropped image smaller than
 * modelDsPad on either axis, a model whose feature ids reach beyond nChns(chns) x the window's cells, NV12 / NV21 or unknown pix;
 * what acf_hip_chns_compute refuses with its code (odd softBin, pColor.smooth > 1, ...); ACF_HIP_E_UNSUPPORTED for an LDCF model. */
ACF_HIP_API int acf_hip_evaluate_crops(acf_hip_ctx* ctx, const acf_hip_params* chns, const float* crops_dev, int n, int h, int w, int d,
    double cascThr, float* scores_dev);
ACF_HIP_API int acf_hip_evaluate_crops_u8(acf_hip_ctx* ctx, const acf_hip_params* chns, const uint8_t* crops_dev, int n, int h, int w, int pix,
    int row_stride_bytes, double cascThr, float* scores_dev);
/* thrs.convertTo(thrsU8, CV_8UC1, 255.0f) (ACFIOArchive.h:96-99): host only, no context. */
ACF_HIP_API int acf_hip_thrs_u8(const float* thrs, int n, uint8_t* out);

#ifdef __cplusplus
}
#endif
#endif /* ACF_HIP_H */
