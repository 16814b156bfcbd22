// acf_hip.hip — implementation of the C ABI in include/acf_hip.h: context,
// planning, buffer ownership and kernel launches.  All device work is
// enqueued on the context's stream; nothing here falls back to the CPU.
// This file holds the context, the guards and helpers every entry shares, and the plan / run / stream entries; the stages'
// logic, the input entries (input_run.hip.h), the read-back entries and the single-operator entries are textual parts (*.hip.h), included
// in the order of their use.
#include "kernels.hip.h"

#include <algorithm>
#include <atomic>
#include <cmath>
#include <cstdio>
#include <cstring>
#include <mutex>
#include <string>
#include <type_traits>
#include <vector>

using namespace acfhip;

namespace
{

struct DevBuf
{
    void* p = nullptr;
    size_t bytes = 0;
};

// LDS-tile plan of a down-sampling descriptor (resampleTilePlan; k_ldcf_tile)
struct ResampleTiling
{
    int rows = 0, cols = 0, xo = 0, tile_y = 0, tile_x = 0;
};

// k_resample_strip plan of a down-sampling image resample, alone or together with the next real scale's (same source)
struct StripPlan
{
    bool ok = false;
    int yt = 0, nty = 0, nSteps = 0, ntyB = 0, nStepsB = 0, tileY = 0, tileX = 0, rowsP = 0, maxCols = 0, slowRows = 0, fillRounds = 0, tileFloats = 0;
    uint32_t magic = 0;
    size_t lds = 0;
    int why = 0; // !ok: the reason stripPlan refused (ACF_HIP_SF_WHY_*; 0: no plan was asked for)
};

struct RealScale
{
    int level = 0, h = 0, w = 0;
    bool resampled = false; // image produced by imResample (else it is the current I itself)
    bool adoptAsI = false;  // after this scale, I := smoothed image of this scale
    int src_h = 0, src_w = 0;
    int descIndex = -1;
    StripPlan strip, stripPair;     // k_resample_strip: this scale's image alone / together with the next real scale's (stripPair.ok)
    float *img = nullptr, *sm = nullptr, *M = nullptr, *O = nullptr, *U = nullptr, *S = nullptr, *Mn = nullptr;
    int64_t uFloats = 0, moFloats = 0; // floats per frame of U and of M, O (room for the blocked layouts' padding)
    // convTri's x pass as checkpoints (host_plan.h triCkIndex): where that form runs U is not needed, so U is allocated only when a
    // call first takes a form that reads it (PyramidRun::realScale).  triForm: what the last pyramid call ran (acf_hip_get_tri_forms)
    float* Ck = nullptr;
    int64_t ckFloats = 0;
    int triForm = 0;
    int32_t scaleForm = 0; // acf_hip_get_scale_forms' run side (route, SLOW, xt, nty, nSplit), written by PyramidRun::imageResample
};

// Where the frames of a call come from: what every entry that takes frames hands to pyramidBody (input_run.hip.h holds the rest of
// the input path; the type stands here because the context keeps the one its stream was opened with)
enum SourceKind
{
    SRC_F32,   // planar float planes, the pyramid's own layout
    SRC_U8,    // packed 8-bit frames: pix (ACF_HIP_PIX_*, NV12 / NV21 included), rowStride
    SRC_IMAGE, // an upright image of any element strides: img
    SRC_YUV,   // three planes described by offsets and byte strides: yuv
    SRC_VIEW   // affine views of stored frames (acf_hip_pyramid_view): img or yuv (viewYuv) + fmt at srcRows x srcCols, orient; views, viewFrames
};
struct FrameSource
{
    SourceKind kind = SRC_F32;
    const void* base = nullptr;
    const char* who = "pyramid";  // the entry's name in messages
    int pix = 0, rowStride = 0;
    acf_hip_image_desc img{};
    acf_hip_yuv_desc yuv{};
    bool resized = false;         // the resized entries: frames of srcRows x srcCols, reduced by `scale` to the plan's size
    int srcRows = 0, srcCols = 0;
    double scale = 1;
    int orient = 0;               // the oriented entries (ACF_HIP_ORIENT_*, image and YUV kinds): frames of srcRows x srcCols, turned to the plan's size
    acf_hip_yuv_format fmt{ 8, 0, ACF_HIP_YUV_MATRIX_BT601, 0 }; // the video entries (SRC_YUV): sample width, matrix and range; this is the default
    // the view entries (SRC_VIEW): frame i of the batch is view views[i] of stored frame viewFrames[i] (null: i) of nStored, samples x samples a pixel
    bool viewYuv = false;
    const float* views = nullptr;
    const int32_t* viewFrames = nullptr;
    int nStored = 0, samples = 1;
};

} // namespace

// One set of tile tables of the LDS-tiled cascade (buildTileSet): geometry, tile list, node records with tile-layout offsets, on
// float cells or on 16-bit threshold-rank cells (thresholds then as rank indices).
struct TileSet
{
    bool ok = false;
    TileGeom g{};
    int nTiles = 0, aTB = 4;
    CascTile* d_tiles = nullptr;
    TreeNode* d_tileNodes = nullptr;  // depth 2: every tree
    uint32_t* d_tileNodesS = nullptr; // depth 2, stage A of k_cascade_tile3: 10 * aTB dwords per batch of aTB trees
    // depths other than 2 (k_cascade_tileD): records of trees [0, t1D) in batches of tbD
    uint32_t* d_nodesD = nullptr;
    int tbD = 0, t1D = 0;
    uint32_t* d_tileOffD = nullptr; // k_cascade_tile3D: tile offsets of every node, [tree][nTreeNodes]
    uint32_t* d_thrsRankD = nullptr; // ... and, on rank cells, the thresholds' rank indices in the same layout
};

// A leaf-code buffer: [frame][cap][pitch] bytes, 4 * leaf index of every tail tree of the first cap queue entries of a frame.
struct LeafCodes
{
    uint8_t* d = nullptr;
    int cap = 0, pitch = 0;
};

// The cascade's counters in d_qcounts, int32 each, for a state of B frames: the ONE statement of their layout.
//   staged path:        the count of stage s's queue [frame] at s * B (at most 4 stages); the tile counters of the tile kernel in front
//                       (depths 1, 3, 4) at 8 * B
//   depth-2 tiled path: the tail queue's count [frame] at 0, its head [frame] at B, k_cascade_tile3's tile counters at 2 * B
struct QueueCounters
{
    static constexpr size_t TILE_COUNTERS = 8; // the persistent tile kernels' next tile, one per XCD
    int32_t* d;
    size_t B;
    static size_t allocCount(size_t B) { return 8 * B + TILE_COUNTERS; }
    int32_t* stage(int s) const { return d + size_t(s) * B; }
    size_t stagedCount(int nStages) const { return size_t(nStages) * B; } // what the staged path clears from d on
    int32_t* tileNextD() const { return d + 8 * B; }                      // (cleared on its own, when the workgroups are persistent)
    int32_t* queueCount() const { return d; }
    int32_t* queueHead() const { return d + B; }
    int32_t* tileNext2() const { return d + 2 * B; }
    size_t tiled2Count() const { return 2 * B + TILE_COUNTERS; }          // what the depth-2 tiled path clears from d on
};

// Everything the cascade launch needs on the device, and what it was built for.
struct CascState
{
    int cell = 0;    // pixels per cell: shrink, or 2 * shrink on the LDCF pyramid
    int nLevels = 0; // levels of a frame
    int batch = 0;   // frames the per-frame buffers hold
    int maxHits = 0; // hits per frame d_hits, d_hitsX, d_sorted and d_dets hold (allocCascadeRun)
    CascLevel* d_cascLevels = nullptr;
    int32_t* d_blockLevel = nullptr;
    int blocksPerFrame = 0;
    uint32_t* d_cidAll = nullptr;
    float *d_thrs = nullptr, *d_hs = nullptr;
    uint32_t* d_child = nullptr;
    uint32_t* d_fids = nullptr;
    CascNode2* d_nodes2 = nullptr;
    acf_hip_hit *d_hits = nullptr, *d_sorted = nullptr;
    // stride < shrink: the cascade runs on the grid of distinct window offsets (kernels.hip.h, k_expand_hits)
    int dedupQ = 1;                  // shrink / stride when that is an integer > 1, else 1
    int2* d_realWin = nullptr;       // [level] {nWinR, nWinC} of the real window grid
    acf_hip_hit* d_hitsX = nullptr;  // the expanded hits (k_sort_map's input)
    acf_hip_detection* d_dets = nullptr;
    int32_t* d_counts = nullptr;
    uint2* d_queue[2] = { nullptr, nullptr }; // survivor queues between cascade stages
    int32_t* d_qcounts = nullptr;             // see QueueCounters
    QueueCounters counters() const { return { d_qcounts, size_t(batch) }; }
    int qcap = 0;
    // LDS-tiled path (stride a multiple of shrink): the tile sets over float cells and over threshold-rank cells (host_plan.h).
    // Depth 2: k_cascade_tile3 + the tail; depths 1, 3, 4: the staged path's first stages (k_cascade_tile3D if g.pooled, else
    // k_cascade_tileD).  A set that is not in use has ok == false; tilesR.ok implies tiles.ok.
    TileSet tiles, tilesR;
    // depth 2: the tail beyond tiles.g.b[4] (k_cascade_tail3, k_cascade_tail_rank)
    TreeNode* d_tailNodes = nullptr; // offsets = feature ids (window-local layout), all trees
    TreeNode* d_tailNodesR = nullptr; // k_cascade_tail_rank: packed (z, c, r) feature positions, thresholds as rank indices
    int tailWaves = 0;
    float* d_tailScratch = nullptr; // k_cascade_tail3 leaf matrices: [blocks][tailWaves][TAIL_G][tailPad]
    int tailPad = 0, tailSlab = 0, tailBlocks = 0, tailNodesLds = 0;
    // the tail's leaf codes of the first codes.cap queue entries per frame (depth 2: stage E of k_cascade_tile3 + k_tail_scan;
    // depths 1..4: stage E of k_cascade_tile3D or k_tail_codesD, + k_tail_scanD)
    LeafCodes codes;
    // the rank pyramid (threshold-rank cells, 16 bits each) and the tables that make it from the float pyramid (k_rank)
    RankChan* d_rankChan = nullptr;
    RankRec* d_rankRec = nullptr;
    int rankMaxRec = 0;
    bool rankHasZero = false; // RankTables::hasZero: the rank kernels' forms with the select for negative cells
    RankJob* d_rankJobs = nullptr;
    uint16_t* d_pyrR = nullptr;
    int64_t pyrRCells = 0; // cells per frame
    int rankMaxWP = 0;
};

// The LDCF post-stage (acf_hip_params::ldcfK > 0; PlanBuild::ldcf, runLdcf): every level of the pyramid filtered (k 5x5 filters per
// channel) and halved into the LDCF pyramid, on which the cascade then runs.
struct LdcfStage
{
    std::vector<acf_hip_level> levels; // level table of the LDCF pyramid
    int descBase = 0;                  // the levels' resample descriptors in h_descs / d_descs
    int64_t floats = 0, tmpFloats = 0; // floats per frame of the LDCF pyramid and of the filtered scratch
    float* d_filt = nullptr;
    LdcfJob* d_jobs = nullptr;
    // k_ldcf_tile (filters + half resample fused): flat list of output tiles over all levels, LDS geometry
    LdcfTileJob* d_tileJobs = nullptr;
    int tiles = 0, tileRows = 0, tileCols = 0;
    int maxCells = 0, maxBlocks = 0; // k_ldcf_conv + k_resample (no tile list): grid sizes
    float* d_tmp = nullptr;
    float* d_pyr = nullptr;
};

// acf_hip_set_option's keys, one field each (OPTION_KEYS), except "graph" and "streams": those stay the parent's, and
// sub-batch children hold a copy of everything here.  Every field is an int so that the key table can point at it.
struct Options
{
    int taps = 0;
    int arith = 0;   // 1 = the reference's rcpps / rsqrtps bits from d_x86 (acf_hip_set_x86_tables)
    int profile = 0;
    int fusedSmooth = 1; // 0: separate smoothing / half resample / colour-channel kernels
    // 0 = gradMag as its own kernel (k_grad_mag_vec), 1 = inside the gradient plane's smoothing chain (k_smooth_grad) where that
    // pays (big planes, many frames), 2 = wherever k_smooth_grad applies
    int fusedGrad = 1;
    // convTri's x pass over M inside that chain as well (k_smooth_grad_tri; the gradient plane is then ONE segment): 0 = never
    // (k_tri_x5v), 1 = where k_smooth_grad runs in batches of >= 64 frames of a context that shares its device, 2 = wherever
    // k_smooth_grad runs
    int fusedTri = 1;
    // this context runs beside other contexts on the same device (the pools set it).  Kernel forms are then chosen for the least
    // WORK instead of the shortest time alone: a lone context cuts the smoothing chains into segments to fill the machine (20 % more
    // columns, a verify and a repair launch per scale) and keeps the x pass a kernel of its own; beside other contexts a thin
    // chain's latency is covered by their kernels and only its work counts (3 x 96 frames at 1080p: +4.3 % frames/s; alone, 96
    // frames: -7 %)
    int sharedDevice = 0;
    // the pooled tile kernel runs as persistent workgroups that draw tiles from a counter (best alone on the device: -8 % on that
    // kernel) or one short-lived workgroup per tile (best beside other contexts' kernels, which then find free LDS)
    int tilePersist = 1;
    int cascadeTiles = 1; // 0: force the global-memory staged cascade (A/B and parity of both paths)
    // 1: the tile kernel of depth-2 models reads 16-bit threshold-rank cells (host_plan.h) — identical decisions, half the tile;
    // 0: it reads the float pyramid (A/B and parity of both forms)
    int rankCells = 1;
    // 1: the real scales of a batch run on their own streams (best for ONE context: +8 % frames/s, batch-1 latency 2.1 -> 1.5 ms);
    // 0: on the context's stream in order — what an application that runs several contexts side by side wants (three contexts:
    // 12.1k instead of 11.6k frames/s; they already fill each other's gaps, more streams only multiplex the hardware queues)
    int scaleStreams = 1;
    // the tile kernels of the contexts of one device take turns (each waits for the tile kernel submitted before it on that
    // device, whichever context's): contexts that run in phase otherwise run their cascades — bound by LDS and VALU, not by
    // memory — beside each other instead of beside the other contexts' memory-bound pyramid kernels
    int cascadeTurns = 0;
    int fusedLevels = 1; // 1 fused resample+smooth, 2 separate resample + wave-per-plane smooth, 0 separate launches
    // k_smooth_vec's speculative column segments (kernels.hip.h): the image smoothing's recursion along image-x cut into column
    // segments that start smoothWarm columns early and are checked against each other: 0 = as many as fill the GPU for the batch,
    // 1 = one chain per plane, n = n segments; smoothForceRedo = 1 marks every plane for the repair launch (tests)
    int smoothSegments = 0;
    // 96 warm-up columns: a value decays fourfold per column, so 12-25 columns settle the last bit of ordinary values — but where
    // the image turns exactly 0 (a black bar) the true chain carries a tail that only reaches 0 by underflow, after ~75 columns,
    // while a warm-up started inside the bar is 0 at once (profiles/r03_repair_rates.json: 3 % of planes repaired at 48, none
    // at 64+ on frames with black and flat bands); at 96 frames per launch 48 / 64 / 96 columns cost the same (0.36-0.38 ms)
    int smoothWarm = 64, smoothForceRedo = 0; // (profiles/r03_repair_rates.json: no repair from 64 columns on)
    // The level chains' segments: 0 (default) = AUTO — batches of at most levelSegFrames (8) frames run the speculative segmented
    // k_level_all + k_level_verify + the repair launch, bigger batches one chain per plane; 1 = off; n > 1 = n segments whatever
    // the batch.  A level is at most 480 columns, so segments only pay with warm-ups of ~32 columns (levelWarm; one frame:
    // 372 -> 124 us), and channel planes have exactly-zero regions wherever the image is flat (no gradient): a plane whose
    // hand-over differs costs its whole chain again in the repair launch (tests/test_gpu_segments.py counts the repairs of a
    // frame with flat bands so that this cost stays visible).
    int levelSegments = 0;
    int levelWarm = 32;
    // planes the repair launches had to recompute (synchronises after every verify: measurements only)
    int countRepairs = 0;
    // 0: the caller only wants detections (acf_hip_run / acf_hip_detect): when the levels leave as rank cells the float pyramid is
    // not written at all (acf_hip_read_level and the Pyramid-returning entries then fail with ACF_HIP_E_INVALID); 1 (default): both
    int keepPyramid = 1;
};

// The context's state is grouped by lifetime.  Each group is a base of acf_hip_ctx, so its fields are reached as c->field, and a
// lifetime's reset is the assignment of a default-constructed group: no function keeps a list of fields to clear.

// ---- acf_hip_set_model's: the classifier and the channel parameters (they survive acf_hip_plan)
struct ModelState
{
    bool hasModel = false;
    acf_hip_params p{};
    std::vector<uint32_t> fids, child;
    std::vector<float> thrs, hs;
    std::vector<float> ldcfFilters; // where p.ldcfFilters points: the filters outlive a plan, the LDCF stage built from them does not
    // acf_hip_evaluate_crops: the classifier on the device without a plan (not one of the plan's buffers: uploaded at the first call
    // after acf_hip_set_model, freed by the next one and by acf_hip_destroy); fidMax: the largest feature id a tree walk can read
    struct CropModel
    {
        uint32_t *fids = nullptr, *child = nullptr;
        float *thrs = nullptr, *hs = nullptr;
        uint32_t fidMax = 0;
        bool valid = false;
    } crop;
    // acf_hip_set_bank: the members' parameters and arrays (p's pointers name the vectors beside it).  They were checked against this
    // model, so acf_hip_set_model clears them
    struct BankMember
    {
        acf_hip_params p{};
        std::vector<uint32_t> fids, child;
        std::vector<float> thrs, hs;
    };
    std::vector<BankMember> bank;
};

// ---- what the last pyramid / detect call left (part of the plan's state: a new plan starts without a batch; a replayed graph
// restores what its captured host code left, GraphSlot::after)
struct LastRun
{
    int lastBatch = 0;
    bool pyramidValid = false, detectValid = false;
    bool ranksValid = false;   // the rank pyramid of the last batch has been written (by the level kernels or by k_rank)
    bool floatPyramid = true;  // the float pyramid of the last batch exists (option keep_pyramid = 0: it may not)
    bool countsFetched = false; // h_counts holds the last batch's counts
    const float* lastFrames = nullptr;
    bool viewRun = false;      // the last batch's frames were views (acf_hip_pyramid_view): its boxes are in view coordinates
    bool bankValid = false;    // acf_hip_detect_bank has run on the last batch's pyramid
};

// ---- acf_hip_plan's: everything the plan builds, and what runs allocate lazily under it.  dropPlan frees `allocs` and assigns a
// fresh PlanState, so a pointer declared here never outlives the memory it names.
struct PlanState : LastRun
{
    bool hasPlan = false;
    Plan plan;
    int maxBatch = 0, maxHits = 0;
    std::vector<void*> allocs; // every device buffer of this struct (devAlloc / devUpload)
    // image-specific lambdas (model without lambdas, chnsPyramid.cpp:341-374): per-frame plane sums of two real levels on
    // the device, the lambdas of every frame of the last batch on the host
    bool autoLambdas = false;
    double* d_planeSums = nullptr;     // [maxBatch][2][nChns]
    std::vector<double> h_lambdas;     // [maxBatch][3]
    // constant tables (ensureConstTables: also built without a plan, for the single-operator entries)
    float* d_lTable = nullptr;
    float* d_acos = nullptr;
    // planning tables
    std::vector<RealScale> real;
    std::vector<ResampleDesc> h_descs; // [real-image resamples..., approx levels...]
    int nImgDescs = 0, nApproxDescs = 0;
    ResampleDesc* d_descs = nullptr;
    int32_t* d_it = nullptr;
    float* d_ft = nullptr;
    SmoothJob* d_realJobs = nullptr; // one per real scale
    SmoothJob* d_finalJobs = nullptr;
    LevelJob* d_levelJobs = nullptr;
    float* d_dump = nullptr; // 64 floats nobody reads: target of stores from lanes past the end of a plane (keeps kernels branch-free)
    LevelJob* d_levelJobsRaw = nullptr; // same levels, every one read from its raw channels (after a separate resample launch)
    struct LevelGroup
    {
        int R, mode, first, count;
        double cost; // ~ column steps x work per step of the group's longest plane chain and of all its planes (see pack)
        int lane;    // side stream the launch goes to (longest-processing-time-first over the hardware queues)
    };
    std::vector<LevelGroup> levelGroups, levelGroupsRaw; // jobs sorted into runs of equal (R, mode)
    int nAllJobs = 0, nAllJobsRaw = 0; // leading jobs of d_levelJobs(/Raw) that go to the single k_level_all launch
    bool fusedOk = false;      // the fused resample+smooth level kernel covers this plan
    PadJob* d_padJobs = nullptr;
    PadJob* d_padJobsR = nullptr; // the same borders in the rank pyramid's layout
    bool levelsEmitRank = false;  // every level goes through k_level_all: the level kernels can write the rank cells themselves
    // acf_hip_get_level_forms: per level the word levelJobs wrote while it decided (ACF_HIP_LF_*; the job in the fused list and in the
    // raw list), and the call-wide words the last pyramid call's planLevels left
    std::vector<int32_t> levelFormFused, levelFormRaw;
    int32_t levelCallForm[ACF_HIP_LF_HEAD] = { 0, 0, 0, 0, 0, 0 };
    // acf_hip_get_cascade_forms: the record of the last runCascade on this context (noteCascadeForms), and its place in the order
    // of the process's cascade calls (0: none yet) — a parent's operator call against its sub-batch children's pipeline calls
    int32_t cascadeForm[ACF_HIP_CF_WORDS] = {};
    uint64_t cascadeFormSeq = 0;
    // k_smooth_vec's speculative column segments (kernels.hip.h): state of the segments' hand-overs, planes to repair
    float *d_specState = nullptr, *d_trueState = nullptr;
    int32_t* d_redo = nullptr;
    size_t redoInts = 0, lvRedoInts = 0; // their sizes (clearRepairFlags)
    // the same for the level chains (k_level_all<OUT, 1>), for batches of at most levelSegFrames frames
    float *d_lvSpec = nullptr, *d_lvTrue = nullptr;
    int32_t* d_lvRedo = nullptr;
    int levelSegFrames = 0, levelSegCap = 0, levelHMax = 0;
    int segCap = 0;               // segments the state buffers hold per plane
    int finalMaxH = 0;
    int approxMaxBlocks = 0;
    int64_t padMaxElems = 0;
    LdcfStage ldcf;
    // frame buffers
    float* d_color = nullptr; // colour-converted full-resolution image (if a conversion is needed)
    float* d_chns = nullptr;
    float* d_pyr = nullptr;
    // the plan's cascade (tables, model arrays, work queues, outputs); acf_hip_op_acf_detect1 builds and runs a state of its own
    CascState cs;
    BoxLevel* d_boxLevels = nullptr;
    // -- allocated by the first run that needs them --
    float* d_stage = nullptr; // H2D staging for run_host; planar f32 target of the 8-bit ingest when no colour conversion follows
    // device bbNms + prune: survivors of every frame, what get_detections / export then return (the settings are the context's: nmsOn, nms)
    int32_t *d_nmsKeep = nullptr, *d_nmsN = nullptr, *d_nmsCounts = nullptr;
    acf_hip_detection* d_nmsDets = nullptr;
    std::vector<int32_t> h_counts;
    // acf_hip_set_input_resize: the apps' resize to a minimum object width in front of the 8-bit entries (k_resize_u8)
    struct InputResize
    {
        bool on = false;
        int rows = 0, cols = 0;
        double scale = 1;
        ResizeTables t;
        int32_t *d_xlin = nullptr, *d_ylin = nullptr, *d_xrun = nullptr, *d_yrun = nullptr, *d_xtap = nullptr, *d_ytap = nullptr;
        uint8_t* d_out = nullptr; // [maxBatch][plan.H][plan.W][4]
        int osBand[2] = { -1, -1 }; // the oriented resized entries: reduced rows a band for rot 0 / 2 and rot 1 / 3 (orientedResizedBand; -1: not yet)
    } rz;
    // the resized tensor / YUV entries (acf_hip_pyramid_image_resized / _yuv_resized): the tap tables of the last (rows, cols, scale),
    // uploaded at the first call with a new key and kept until another key or acf_hip_plan (d_out is not used: k_ingest_resized
    // leaves no reduced 8-bit image)
    InputResize rzIn;
    // acf_hip_set_yuv_layout: where an NV12 / NV21 frame's chroma plane starts and how far frames are apart (0 = tight)
    struct YuvLayout
    {
        int64_t chromaOff = 0, frameStride = 0;
    } yuv;
    uint8_t* d_yuvRgb = nullptr; // k_yuv420_to_rgb8's tight RGB frames (in front of the input resize; fallback yuv_unfused)
    size_t yuvRgbBytes = 0;
};

// ---- an open stream's (acf_hip_stream_open* .. acf_hip_stream_close; acf_hip_plan closes it: its slots are sized by the plan)
struct StreamFront
{
    struct StreamSlot
    {
        uint8_t* d_in = nullptr;   // device copy of the packed 8-bit batch
        int32_t* d_rec = nullptr;  // device records (acf_hip_export_detections layout)
        int32_t* h_rec = nullptr;  // pinned host records
        hipEvent_t evH2D = nullptr, evDone = nullptr;
        int ticket = -1, nFrames = 0;
    };
    std::vector<StreamSlot> slots;
    hipStream_t copyStream = nullptr;
    int stCap = 0, nextTicket = 0, nextCollect = 0;
    int64_t stFrameBytes = 0; // bytes between the frames of a submitted batch
    FrameSource stSrc;        // what the stream was opened for: a batch runs as this source at its slot's device buffer
};

// ---- create .. destroy, and the settings that survive acf_hip_plan (options, NMS, the x86 tables, the counted repairs)
struct acf_hip_ctx : ModelState, PlanState, StreamFront
{
    int device = 0;
    hipStream_t stream = nullptr; // the caller's stream: assigned in acf_hip_create and nowhere else (a stage that enqueues elsewhere is told its stream)
    bool ownStream = false;
    // side streams: independent launches of one stage (the level groups) run concurrently, forked from and
    // joined back into `stream` with events, so the stage costs its longest launch instead of their sum
    std::vector<hipStream_t> side;
    hipEvent_t evFork = nullptr;
    std::vector<hipEvent_t> evJoin;
    std::vector<hipEvent_t> evScale;   // pyramid: "real scale k has been smoothed" (the next real scale starts from it on its own stream)
    hipEvent_t evTurn[2] = { nullptr, nullptr }; // [0] tile kernel, [1] level kernel (bit 1 of the option: own turns; bit 2: the tile kernels' turns)
    // the device as hipGetDeviceProperties describes it (acf_hip_create): the persistent grids are sized from these.  The
    // counters the persistent workgroups draw tiles from are eight (blockIdx.x & 7: one per XCD of an MI355X, whose
    // dispatcher deals consecutive workgroups to consecutive XCDs); on a part with another XCD count the ranges still
    // cover every tile, only their locality is lost.
    int numCus = 256;
    size_t ldsPerCu = size_t(160) * 1024;
    mutable std::string err;
    Options opt; // acf_hip_set_option's settings (sub-batch children hold the parent's)
    bool x86Owned = false;
    uint32_t* d_x86 = nullptr; // [X86_BUF_N]: rcp over [1, 2) by m >> 11 (4096), rsqrt over [1, 4) by parity and m >> 11 (2 x 4096), then gradMag's composed pairs
    // acf_hip_set_nms: device bbNms + prune after the cascade (its buffers are the plan's)
    bool nmsOn = false;
    acf_hip_nms_params nms{};
    int64_t repairs[4] = { 0, 0, 0, 0 }; // {smoothing planes checked, redone, level planes checked, redone}
    bool countersZeroed = false; // for the length of one acf_hip_run: it has cleared the tiled cascade's counters in front of the pyramid's launches
    // Sub-batch contexts (option "streams" = K > 1): the batch is cut into K contiguous chunks, each run by a child
    // context with its own buffers and stream, forked from / joined into `stream` by events.  The path is a chain of
    // kernels several of which are latency-bound inside a frame (column recursions, per-tile dependency chains):
    // chunks at different stages of the chain fill each other's idle issue slots and memory time.  They hold the plan's buffers
    // in this context's place, so they go with the plan (dropPlan).
    std::vector<acf_hip_ctx*> kids;
    int nStreams = 1, kidChunk = 0;
    // The bank's members under a plan (bank_run.hip.h): a context each, with the member as its model, its own cascade state, box table
    // and result buffers — and this context's device, stream and options; no pyramid of its own.  They go with the plan.
    // What is meaningful on a member, and all that runCascade, readRecords and acf_hip_profile_get read of it: device, stream, numCus,
    // ldsPerCu, opt, err, evPool / evUsed, evTurn; ModelState (p and the arrays); of PlanState hasPlan, plan (the owner's geometry, the
    // level table with the member's window grid), maxBatch, maxHits, allocs, cs, d_boxLevels, h_counts, cascadeForm; of LastRun
    // lastBatch, pyramidValid, detectValid, countsFetched (set by acf_hip_detect_bank).  Everything else keeps its default: d_pyr, d_chns,
    // d_x86, the real scales, the job lists and the NMS buffers are null on a member — code that needs the cells takes them from the
    // CascInput it is handed, never from a member's PlanState.
    std::vector<acf_hip_ctx*> bankCtx;
    // option "graph": acf_hip_run replays a HIP graph captured from its own launches (same frames pointer, same batch size):
    // one host call instead of ~45 launches per frame — what a single frame's latency is made of when the kernels take 20 us
    int useGraph = 0;
    // option "graph": captured runs keyed by (input pointer, batch size); a caller that alternates between a few input buffers
    // (double / triple buffering) replays one graph per buffer instead of re-capturing on every call
    struct GraphSlot
    {
        hipGraphExec_t exec = nullptr;
        const float* frames = nullptr;
        LastRun after; // what the captured host code left behind (after.lastBatch: the batch size)
    };
    static constexpr int GRAPH_SLOTS = 4;
    GraphSlot graphs[GRAPH_SLOTS];
    int graphNext = 0; // slot the next capture replaces (round robin)
    int plainRuns = 0, graphBroken = 0;
    // option "profile": a pool of markers, the first evUsed of them recorded since the last acf_hip_profile_get
    struct ProfMark
    {
        hipEvent_t ev;
        const char* name;
        hipStream_t stream; // the stream it was recorded on (a kernel ends at the next marker of ITS stream)
    };
    std::vector<ProfMark> evPool;
    size_t evUsed = 0;
};

// the ONE statement of "the cascade state has rank cells and option rank_cells is on"; each reader adds its own terms
static inline bool rankCellsOn(const acf_hip_ctx* c, const CascState& cs)
{
    return cs.tilesR.ok && c->opt.rankCells;
}

#define HIPCHK(ctx, call)                                                                                  \
    do                                                                                                     \
    {                                                                                                      \
        hipError_t e_ = (call);                                                                            \
        if (e_ != hipSuccess)                                                                              \
        {                                                                                                  \
            (ctx)->err = std::string(#call) + ": " + hipGetErrorString(e_);                               \
            return ACF_HIP_E_HIP;                                                                          \
        }                                                                                                  \
    } while (0)

#define LAUNCHCHK(ctx, what)                                                                               \
    do                                                                                                     \
    {                                                                                                      \
        hipError_t e_ = hipGetLastError();                                                                 \
        if (e_ != hipSuccess)                                                                              \
        {                                                                                                  \
            (ctx)->err = std::string("launch ") + what + ": " + hipGetErrorString(e_);                    \
            return ACF_HIP_E_HIP;                                                                          \
        }                                                                                                  \
    } while (0)

namespace
{

// ACF_HIP_FORCE_FALLBACK: the library's ONE form-selecting environment switch (read once per process).  Every stage keeps one
// fallback form for the shapes its default form does not cover; a comma-separated list of the names below makes those fallbacks
// run where the default would, so that tests/test_gpu_variants.py can hold each of them against the oracle on ordinary frames.
// All forms give identical results.  (The other two variables, ACF_HIP_CASC_BOUNDS and ACF_HIP_TILE_TR / _NW, are the tile
// kernels' tuning knobs: stage boundaries and tile geometry.)
enum : uint32_t
{
    FB_TRIY_UNFUSED = 1u << 0,      // convTri's y pass writes S, k_chns forms the cells (instead of k_triy_chns)
    FB_MOU_PLAIN = 1u << 1,         // M, O, U as plain planes (instead of 64 x 16 blocks)
    FB_RESAMPLE_NO_STRIP = 1u << 2, // image resamples without k_resample_strip
    FB_RESAMPLE_NO_PAIR = 1u << 3,  // ... without the two small scales in one pass
    FB_RESAMPLE_NO_UP = 1u << 4,    // up-sampling (nOctUp > 0) through the generic k_resample
    FB_RESAMPLE_GENERIC = 1u << 5,  // every resample through the generic k_resample
    FB_LEVEL_GROUPS = 1u << 6,      // the levels as one k_level launch per (rows per lane, mode) run instead of k_level_all
    FB_LDCF_UNFUSED = 1u << 7,      // LDCF as k_ldcf_conv + k_resample instead of k_ldcf_tile
    FB_NO_DEDUP = 1u << 8,          // stride < shrink: one cascade evaluation per window instead of one per distinct offset
    FB_NO_TAIL_CODES = 1u << 9,     // the tail without leaf codes (k_cascade_tail3 / _tail_rank on every tail window)
    FB_TAIL3 = 1u << 10,            // every tail window through k_cascade_tail3
    FB_TILED_STAGED = 1u << 11,     // depths 1, 3, 4: the staged queue instead of the pooled tile kernel
    FB_TILED_POOLED1 = 1u << 12,    // depth 1 on float cells: the pooled tile kernel instead of the staged queue
    FB_YUV_UNFUSED = 1u << 13,      // NV12 / NV21 as k_yuv420_to_rgb8 + k_ingest_u8 instead of k_ingest_yuv420
    FB_TRIY_STORED_U = 1u << 14,    // convTri's x pass writes the blocked plane U (instead of checkpoints replayed by k_triy_chns)
    FB_ORIENTED_RESIZED_GENERIC = 1u << 15, // the oriented resized entries gather from global memory (instead of staging the footprint in LDS)
};
uint32_t fallbackMask()
{
    static const uint32_t mask = [] {
        static const struct { const char* name; uint32_t bit; } kNames[] = {
            { "triy_unfused", FB_TRIY_UNFUSED }, { "mou_plain", FB_MOU_PLAIN }, { "resample_no_strip", FB_RESAMPLE_NO_STRIP },
            { "resample_no_pair", FB_RESAMPLE_NO_PAIR }, { "resample_no_up", FB_RESAMPLE_NO_UP }, { "resample_generic", FB_RESAMPLE_GENERIC },
            { "level_groups", FB_LEVEL_GROUPS }, { "ldcf_unfused", FB_LDCF_UNFUSED }, { "no_dedup", FB_NO_DEDUP }, { "no_tail_codes", FB_NO_TAIL_CODES },
            { "tail3", FB_TAIL3 }, { "tiled_staged", FB_TILED_STAGED }, { "tiled_pooled1", FB_TILED_POOLED1 },
            { "yuv_unfused", FB_YUV_UNFUSED }, { "triy_stored_u", FB_TRIY_STORED_U },
            { "oriented_resized_generic", FB_ORIENTED_RESIZED_GENERIC } };
        uint32_t m = 0;
        const char* e = getenv("ACF_HIP_FORCE_FALLBACK");
        std::string s = e ? e : "";
        size_t i = 0;
        while (i < s.size())
        {
            size_t j = s.find(',', i);
            j = j == std::string::npos ? s.size() : j;
            const std::string tok = s.substr(i, j - i);
            bool known = tok.empty();
            for (const auto& n : kNames)
            {
                if (tok == n.name)
                {
                    m |= n.bit;
                    known = true;
                }
            }
            if (!known)
            {
                fprintf(stderr, "acf_hip: ACF_HIP_FORCE_FALLBACK: unknown name '%s'\n", tok.c_str());
                abort(); // (a test that names a form that does not exist must not pass on the default form)
            }
            i = j + 1;
        }
        return m;
    }();
    return mask;
}
inline bool fallbackForced(uint32_t which)
{
    return (fallbackMask() & which) != 0;
}

int fail(const acf_hip_ctx* c, int code, const std::string& msg)
{
    c->err = msg;
    return code;
}

// The entry guards: 0, or the code the entry returns at once (a null context has nowhere to leave a text).  An entry calls one
// through `if (int rc = needPlan(c, "detect")) return rc;`.
int needCtx(const acf_hip_ctx* c)
{
    return c ? ACF_HIP_OK : ACF_HIP_E_INVALID;
}
int needPlan(const acf_hip_ctx* c, const char* who, const char* hint = "")
{
    return !c ? ACF_HIP_E_INVALID : c->hasPlan ? ACF_HIP_OK : fail(c, ACF_HIP_E_NOPLAN, std::string(who) + ": plan first" + hint);
}
// (the read-back entries have always answered a null context with E_NOPLAN)
int needPlanRead(const acf_hip_ctx* c, const char* who)
{
    return c ? needPlan(c, who) : ACF_HIP_E_NOPLAN;
}
int needModel(const acf_hip_ctx* c, const char* who)
{
    return !c ? ACF_HIP_E_INVALID : c->hasModel ? ACF_HIP_OK : fail(c, ACF_HIP_E_NOMODEL, std::string(who) + ": set_model first");
}
int needStream(const acf_hip_ctx* c, const char* who)
{
    return !c ? ACF_HIP_E_INVALID : !c->slots.empty() ? ACF_HIP_OK : fail(c, ACF_HIP_E_INVALID, std::string(who) + ": stream_open first");
}

// the CPU tables the three approximate sites evaluate (option "arith" = 1), or null: exact arithmetic
inline const uint32_t* x86T(const acf_hip_ctx* c)
{
    return c->opt.arith ? c->d_x86 : nullptr;
}

// Profile marker: an event recorded on the stream before the launch named
// `name`; a kernel's time is the span to the next marker.
void prof(acf_hip_ctx* c, hipStream_t st, const char* name)
{
    if (!c->opt.profile)
    {
        return;
    }
    if (c->evUsed == c->evPool.size())
    {
        hipEvent_t e;
        if (hipEventCreate(&e) != hipSuccess)
        {
            return;
        }
        c->evPool.push_back({ e, name, st });
    }
    acf_hip_ctx::ProfMark& m = c->evPool[c->evUsed++];
    m.name = name;
    m.stream = st;
    (void)hipEventRecord(m.ev, st);
}

template <class T>
int devAlloc(acf_hip_ctx* c, T** out, size_t count)
{
    void* p = nullptr;
    HIPCHK(c, hipMalloc(&p, std::max<size_t>(count, 1) * sizeof(T)));
    c->allocs.push_back(p);
    *out = reinterpret_cast<T*>(p);
    return ACF_HIP_OK;
}

// convTri's plane U of a real scale, for `batch` frames (at plan time, or when a call first takes a form that reads it)
int allocU(acf_hip_ctx* c, RealScale& rs, int batch)
{
    return devAlloc(c, &rs.U, size_t(batch) * size_t(rs.uFloats));
}

template <class T>
int devUpload(acf_hip_ctx* c, T** out, const std::vector<T>& v)
{
    int rc = devAlloc(c, out, v.size());
    if (rc)
    {
        return rc;
    }
    if (!v.empty())
    {
        HIPCHK(c, hipMemcpy(*out, v.data(), v.size() * sizeof(T), hipMemcpyHostToDevice));
    }
    return ACF_HIP_OK;
}

// one buffer of devAlloc / devUpload given back before the context's teardown (the caller has made sure nothing in flight reads it)
template <class T>
void devRelease(acf_hip_ctx* c, T*& p)
{
    if (!p)
    {
        return;
    }
    auto it = std::find(c->allocs.begin(), c->allocs.end(), static_cast<void*>(p));
    if (it != c->allocs.end())
    {
        c->allocs.erase(it);
        (void)hipFree(p);
    }
    p = nullptr;
}

// Whatever devAlloc / devUpload add to the context's list while the mark lives is freed when it goes.  For acf_hip_op_acf_detect1:
// its buffers come from buildCascadeTables / allocCascadeRun, which allocate into the context — so they cannot be a Scratch's.
struct AllocMark
{
    acf_hip_ctx* c;
    size_t mark;
    ~AllocMark()
    {
        for (size_t i = mark; i < c->allocs.size(); i++)
        {
            (void)hipFree(c->allocs[i]);
        }
        c->allocs.resize(mark);
    }
};

// The one-off device buffers of an operator entry (not the hot path): freed when the entry returns, whichever way.
struct Scratch
{
    std::vector<void*> ptrs;
    ~Scratch()
    {
        for (void* p : ptrs)
        {
            (void)hipFree(p);
        }
    }
    template <class T>
    T* alloc(size_t n)
    {
        void* p = nullptr;
        if (hipMalloc(&p, std::max<size_t>(n, 1) * sizeof(T)) != hipSuccess)
        {
            return nullptr;
        }
        ptrs.push_back(p);
        return reinterpret_cast<T*>(p);
    }
    template <class T>
    T* upload(const T* h, size_t n)
    {
        T* d = alloc<T>(n);
        if (d && n && hipMemcpy(d, h, n * sizeof(T), hipMemcpyHostToDevice) != hipSuccess)
        {
            return nullptr;
        }
        return d;
    }
    // an operator's tail: n elements of what the context's stream computed, on the host
    template <class T>
    static int download(acf_hip_ctx* c, const char* who, T* host, const T* dev, size_t n)
    {
        hipError_t e = hipStreamSynchronize(c->stream);
        e = e ? e : hipMemcpy(host, dev, n * sizeof(T), hipMemcpyDeviceToHost);
        return e ? fail(c, ACF_HIP_E_HIP, std::string(who) + ": " + hipGetErrorString(e)) : ACF_HIP_OK;
    }
};

// The plan goes: its buffers, every pointer to them and everything computed for it — and the sub-batch children, which hold a
// plan's buffers in their parent's place.  (The caller has made sure nothing in flight reads the buffers.)
void dropPlan(acf_hip_ctx* c)
{
    for (acf_hip_ctx* k : c->kids)
    {
        (void)acf_hip_destroy(k);
    }
    c->kids.clear();
    for (acf_hip_ctx* m : c->bankCtx)
    {
        (void)acf_hip_destroy(m);
    }
    c->bankCtx.clear();
    for (void* p : c->allocs)
    {
        (void)hipFree(p);
    }
    static_cast<PlanState&>(*c) = PlanState{};
}

// rgb2luv_setup's table (toolbox/rgbConvertMex.cpp:39-58)
std::vector<float> makeLTable()
{
    std::vector<float> t(1064);
    const float y0 = (float)((6.0 / 29) * (6.0 / 29) * (6.0 / 29));
    const float a = (float)((29.0 / 3) * (29.0 / 3) * (29.0 / 3));
    const float maxi = (float)1.0 / 270;
    for (int i = 0; i < 1025; i++)
    {
        float y = (float)(i / 1024.0);
        float l = y > y0 ? 116 * (float)pow((double)y, 1.0 / 3.0) - 16 : y * a;
        t[i] = l * maxi;
    }
    for (int i = 1025; i < 1064; i++)
    {
        t[i] = t[i - 1];
    }
    return t;
}

LuvConsts makeLuvConsts()
{
    LuvConsts k;
    const float z = 1.0f;
    k.un = (float)0.197833;
    k.vn = (float)0.468331;
    k.mr[0] = (float)0.430574 * z;
    k.mr[1] = (float)0.222015 * z;
    k.mr[2] = (float)0.020183 * z;
    k.mg[0] = (float)0.341550 * z;
    k.mg[1] = (float)0.706655 * z;
    k.mg[2] = (float)0.129553 * z;
    k.mb[0] = (float)0.178325 * z;
    k.mb[1] = (float)0.071330 * z;
    k.mb[2] = (float)0.939180 * z;
    const float maxi = (float)1.0 / 270;
    k.minu = -88 * maxi;
    k.minv = -134 * maxi;
    k.cun = 13 * k.un;
    k.cvn = 13 * k.vn;
    return k;
}

// ACosTable (toolbox/gradientMex.cpp:103-165): 2*(n+b) entries, centre at n+b.
std::vector<float> makeAcosTable()
{
    const int n = 10000, b = 10;
    const float PI = 3.14159265f;
    std::vector<float> a(2 * n + 2 * b);
    float* a1 = a.data() + n + b;
    for (int i = -n - b; i < -n; i++)
    {
        a1[i] = PI;
    }
    for (int i = -n; i < n; i++)
    {
        a1[i] = float(std::acos(i / float(n)));
    }
    for (int i = n; i < n + b; i++)
    {
        a1[i] = 0;
    }
    for (int i = -n - b; i < n / 10; i++)
    {
        if (a1[i] > PI - 1e-6f)
        {
            a1[i] = PI - 1e-6f;
        }
    }
    return a;
}

int ensureConstTables(acf_hip_ctx* c)
{
    if (c->d_lTable)
    {
        return ACF_HIP_OK;
    }
    int rc = devUpload(c, &c->d_lTable, makeLTable());
    if (rc)
    {
        return rc;
    }
    if ((rc = devUpload(c, &c->d_acos, makeAcosTable())))
    {
        return rc;
    }
    return devAlloc(c, &c->d_dump, 1024);
}

// what every single-operator entry starts with: a context, its device current, the constant tables
int opBegin(acf_hip_ctx* c)
{
    if (int rc = needCtx(c)) return rc;
    HIPCHK(c, hipSetDevice(c->device));
    return ensureConstTables(c);
}

// rank pyramid: cells between the columns of a level (every column starts on 16 bytes)
inline int rankPitch(int hP)
{
    return (hP + 7) / 8 * 8;
}

inline int cdiv(int64_t a, int64_t b)
{
    return int((a + b - 1) / b);
}

// ---- kernel launch helpers (shared by the pyramid and the op_* entry points) ----
// (A picker returns the instantiation a launch takes; each names its instantiations in the order the code object lists them.)

// a kernel that takes more than 64 KiB of dynamic LDS asks for it first
int allowLds(acf_hip_ctx* c, const void* kernel, size_t bytes)
{
    if (bytes > 64 * 1024)
    {
        HIPCHK(c, hipFuncSetAttribute(kernel, hipFuncAttributeMaxDynamicSharedMemorySize, int(bytes)));
    }
    return ACF_HIP_OK;
}

using SmoothTri1Kernel = void (*)(const float*, float*, const SmoothJob*, int64_t, int64_t, float, int, float*);

static SmoothTri1Kernel smoothTri1Kernel(int R, bool aliased)
{
    switch (R)
    {
        case 1: return aliased ? k_smooth_tri1<1, true> : k_smooth_tri1<1, false>;
        case 2: return aliased ? k_smooth_tri1<2, true> : k_smooth_tri1<2, false>;
        case 3: return aliased ? k_smooth_tri1<3, true> : k_smooth_tri1<3, false>;
        default: return aliased ? k_smooth_tri1<4, true> : k_smooth_tri1<4, false>;
    }
}

int launchSmooth(acf_hip_ctx* c, hipStream_t st, const float* in, float* out, const SmoothJob* d_jobs, int nJobs, int maxPlanes, int maxH,
    int64_t in_fs, int64_t out_fs, int nFrames, float p, bool aliased)
{
    // threads along y, R interleaved rows per thread: the (nt, R) with the fewest idle row slots (every slot
    // is computed: the kernel clamps instead of branching), fewer rows per thread on a tie
    int nt = 64, R = 0;
    int64_t best = -1;
    for (int r = 1; r <= 4; r++)
    {
        const int t = ((maxH + 64 * r - 1) / (64 * r)) * 64;
        if (t <= 1024 && (best < 0 || int64_t(t) * r < best))
        {
            best = int64_t(t) * r;
            nt = t;
            R = r;
        }
    }
    if (!R)
    {
        return fail(c, ACF_HIP_E_UNSUPPORTED, "smooth: plane taller than 4096 rows");
    }
    const int ldsStride = maxH + 1;
    prof(c, st, nJobs > 1 ? "k_smooth_tri1(levels)" : "k_smooth_tri1(image)");
    const size_t lds = 2 * size_t(ldsStride) * sizeof(float);
    hipLaunchKernelGGL(smoothTri1Kernel(R, aliased), dim3(maxPlanes, nJobs, nFrames), dim3(nt), lds, st, in, out, d_jobs, in_fs, out_fs, p, ldsStride,
        c->d_dump);
    LAUNCHCHK(c, "k_smooth_tri1");
    return ACF_HIP_OK;
}

// fuse: the ChnsArgs of the level when convTriY may be followed at once by the channel cells (k_triy_chns); *fused reports it
// floats per frame of U in the blocked layout: [ceil(w / 64)][ceil((h + 8) / 16)] blocks of 64 columns x 16 rows
static int64_t uBlockedFloats(int h, int w)
{
    return int64_t(cdiv(w, 64)) * ((h + 8 + 15) / 16) * 1024;
}

// ... and of M / O: [ceil(w / 64)][ceil(h / 16)] blocks
static int64_t moBlockedFloats(int h, int w)
{
    return int64_t(cdiv(w, 64)) * ((h + 15) / 16) * 1024;
}

struct TriPlan
{
    bool vecX, doFuse, blocked, ck;
};

// Which forms convTri(M) + the channel cells of a level take: the vector x pass, the fused y pass + cells, and the blocked
// layout of M, O and U (kernels.hip.h, k_tri_x5v) — possible when gradMag, the x pass and the fused y pass are all the vector
// forms and the buffers have room for the blocks' padding (A/B: ACF_HIP_MOU_PLAIN).  gradVec: k_grad_mag_vec writes M and O.
// ck: the x pass leaves checkpoints and k_triy_chns replays it (M and O blocked as before, no U) — wherever the blocked forms apply
// and the checkpoint buffer has room; otherwise blocked needs a U buffer that holds the blocks (a null U holds nothing).
static TriPlan triPlan(const float* in, const float* U, int h, int w, int rad, int64_t fs, const ChnsArgs* fuse, int64_t uCapacity, int64_t moCapacity,
    bool gradVec, const float* Ck = nullptr, int64_t ckCapacity = 0)
{
    const bool noFuse = fallbackForced(FB_TRIY_UNFUSED), plain = fallbackForced(FB_MOU_PLAIN), storedU = fallbackForced(FB_TRIY_STORED_U);
    TriPlan t;
    t.vecX = rad == 5 && h % 4 == 0 && w >= 48 && fs % 4 == 0 && ((uintptr_t(in) | uintptr_t(U)) & 15) == 0;
    t.doFuse = fuse && !noFuse && rad == 5 && h % 4 == 0 && h >= 48 && w % 4 == 0 && fs % 4 == 0 && (uintptr_t(U) & 15) == 0 && fuse->doNorm &&
        !fuse->Mn && (fuse->colorDone || !fuse->colorEnabled) && (fuse->magEnabled || fuse->histEnabled) && fuse->nOrients <= 12 &&
        ((uintptr_t(fuse->M) | uintptr_t(fuse->O)) & 15) == 0;
    const bool blockedMO = t.vecX && t.doFuse && gradVec && !plain && moCapacity >= moBlockedFloats(h, w);
    t.ck = blockedMO && !storedU && Ck && (uintptr_t(Ck) & 15) == 0 && ckCapacity >= triCkFloats(h, w);
    t.blocked = t.ck || (blockedMO && U && uCapacity >= uBlockedFloats(h, w));
    return t;
}

using TriX5Kernel = void (*)(const float*, float*, int, int, int64_t, int64_t, int, int);
using TriyChnsKernel = void (*)(const float*, ChnsArgs, int64_t, int);

static TriX5Kernel triX5Kernel(bool ut, bool ck)
{
    if (ck)
    {
        return k_tri_x5v<true, true>;
    }
    return ut ? k_tri_x5v<true> : k_tri_x5v<false>;
}

static TriyChnsKernel triyChnsKernel(bool maxO6, bool ut, bool x86, bool ck)
{
    if (ck)
    {
        if (maxO6)
        {
            return x86 ? k_triy_chns<6, true, true, true> : k_triy_chns<6, true, false, true>;
        }
        return x86 ? k_triy_chns<12, true, true, true> : k_triy_chns<12, true, false, true>;
    }
    if (maxO6)
    {
        if (ut)
        {
            return x86 ? k_triy_chns<6, true, true> : k_triy_chns<6, true, false>;
        }
        return x86 ? k_triy_chns<6, false, true> : k_triy_chns<6, false, false>;
    }
    if (ut)
    {
        return x86 ? k_triy_chns<12, true, true> : k_triy_chns<12, true, false>;
    }
    return x86 ? k_triy_chns<12, false, true> : k_triy_chns<12, false, false>;
}

// uCapacity / moCapacity: floats per frame the U and the M, O buffers hold (>= fs); blocked: M and O ARE in the blocked layout
// (the caller ran k_grad_mag_vec<true> after asking triPlan)
// xDone: U is there already (k_smooth_grad_tri wrote it, blocked)
// ck: the checkpoint form (Ck, ckCapacity: its buffer); the caller asked triPlan with the same arguments
int launchTri(acf_hip_ctx* c, hipStream_t st, const float* in, float* U, float* S, int h, int w, int rad, int64_t fs, int nFrames, ChnsArgs* fuse = nullptr,
    bool* fused = nullptr, int64_t uCapacity = 0, int64_t moCapacity = 0, bool blocked = false, bool xDone = false, float* Ck = nullptr,
    int64_t ckCapacity = 0, bool ck = false)
{
    if (rad > 15)
    {
        return fail(c, ACF_HIP_E_UNSUPPORTED, "convTri: radius > 15");
    }
    const TriPlan tp = triPlan(in, U, h, w, rad, fs, fuse, uCapacity, moCapacity, blocked, Ck, ckCapacity);
    if ((blocked && !tp.blocked) || ck != (blocked && tp.ck))
    {
        return fail(c, ACF_HIP_E_INVALID, "convTri: blocked M/O without the kernels that read them");
    }
    if (!ck && !U)
    {
        return fail(c, ACF_HIP_E_INVALID, "convTri: no U buffer for the stored form");
    }
    const bool vecX = tp.vecX, doFuse = tp.doFuse, ut = blocked;
    const int nyb = triCkBlockRows(h), nybM = (h + 15) / 16; // (U's blocks and the checkpoints' have the same rows)
    const int64_t ufs = ck ? triCkFloats(h, w) : uBlockedFloats(h, w), mfs = moBlockedFloats(h, w);
    float* const xOut = ck ? Ck : U; // what the x pass leaves and the y pass takes
    if (xDone)
    {
        if (!ut || !doFuse)
        {
            return fail(c, ACF_HIP_E_INVALID, "convTri: the x pass rode on the smoothing chain, but the y pass does not read its blocks");
        }
    }
    else
    {
        prof(c, st, "k_tri_x");
        if (vecX)
        {
            hipLaunchKernelGGL(triX5Kernel(ut, ck), dim3(cdiv(h / 4, 64), 1, nFrames), dim3(64), 0, st, in, xOut, h, w,
                ut ? mfs : fs, ut ? ufs : fs, ut ? nyb : 0, ut ? nybM : 0);
        }
        else
        {
            hipLaunchKernelGGL(k_tri_x, dim3(cdiv(h, 256), 1, nFrames), dim3(256), 0, st, in, U, h, w, rad, fs);
        }
        LAUNCHCHK(c, "k_tri_x");
    }
    if (fused)
    {
        *fused = false;
    }
    if (doFuse)
    {
        prof(c, st, "k_triy_chns");
        if (ut)
        {
            fuse->m_fs = mfs;
            fuse->nybM = nybM;
        }
        hipLaunchKernelGGL(triyChnsKernel(fuse->nOrients <= 6, ut, fuse->x86 != nullptr, ck), dim3(cdiv(w, 256), 1, nFrames), dim3(256), 0, st,
            (const float*)xOut, *fuse, ut ? ufs : fs, ut ? nyb : 0);
        LAUNCHCHK(c, "k_triy_chns");
        *fused = true;
        return ACF_HIP_OK;
    }
    prof(c, st, "k_tri_y");
    if (rad == 5 && h % 4 == 0 && h >= 48 && fs % 4 == 0 && ((uintptr_t(U) | uintptr_t(S)) & 15) == 0)
    {
        hipLaunchKernelGGL(k_tri_y5s, dim3(cdiv(w, 256), 1, nFrames), dim3(256), 0, st, (const float*)U, S, h, w, fs);
    }
    else
    {
        hipLaunchKernelGGL(k_tri_y, dim3(cdiv(w, 64), 1, nFrames), dim3(64), 0, st, (const float*)U, S, h, w, rad, fs);
    }
    LAUNCHCHK(c, "k_tri_y");
    return ACF_HIP_OK;
}

float shrinkGainY(int S)
{
    // imResampleMex.cpp:145-157 with r = 1 and wa == S*wb, then :286/:316 r/S
    float r = 1.0f;
    r /= (float)S;
    r /= float(1 + 1e-6);
    return r / (float)S;
}

using ChnsKernel = void (*)(ChnsArgs);

static ChnsKernel chnsKernel(int shrink, bool maxO6)
{
    if (shrink == 4)
    {
        return maxO6 ? k_chns<4, 6> : k_chns<4, 12>;
    }
    return maxO6 ? k_chns<2, 6> : k_chns<2, 12>;
}

int launchChns(acf_hip_ctx* c, hipStream_t st, const ChnsArgs& a, int shrink, int nFrames)
{
    const int hc = a.h / shrink, wc = a.w / shrink;
    prof(c, st, "k_chns");
    hipLaunchKernelGGL(chnsKernel(shrink, a.nOrients <= 6), dim3(cdiv(int64_t(hc) * wc, 256), 1, nFrames), dim3(256), 0, st, a);
    LAUNCHCHK(c, "k_chns");
    return ACF_HIP_OK;
}

// rgbConvert's gray weights (rgbConvertMex.cpp)
struct GrayWeights
{
    float r, g, b;
};
constexpr GrayWeights kGray = { (float).2989360213 * 1.0f, (float).5870430745 * 1.0f, (float).1140209043 * 1.0f };

// the input planes are the colour planes as they are: no conversion (chnsPyramid.cpp:230-263, rgbConvert.cpp:101-170)
static bool colourPassthrough(const acf_hip_params& p, int nIn)
{
    return nIn >= 3 && (p.colorSpace == ACF_HIP_CS_ORIG || p.colorSpace == ACF_HIP_CS_RGB || (p.isLuv && p.colorSpace == ACF_HIP_CS_LUV));
}

} // namespace

// gradMagNorm as a stand-alone kernel (only the op_gradient_mag entry point
// needs it; the pyramid fuses it into k_chns).  toolbox/gradientMex.cpp:254-275.
__global__ void __launch_bounds__(256) k_norm(float* __restrict__ M, const float* __restrict__ S, int n, float norm, const uint32_t* __restrict__ x86)
{
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n)
    {
        return;
    }
    const int n4 = (n / 4) * 4;
    if (i < n4)
    {
        M[i] = x86 ? M[i] * x86_rcp(S[i] + norm, x86) : M[i] * (1.0f / (S[i] + norm));
    }
    else
    {
        M[i] = M[i] / (S[i] + norm);
    }
}

// Strided plane copy for smooth == 0 (convTri.cpp:206-210: J = I).
__global__ void __launch_bounds__(256) k_copy_planes(const float* __restrict__ in, float* __restrict__ out, const SmoothJob* __restrict__ jobs,
    int64_t in_fs, int64_t out_fs)
{
    const SmoothJob j = jobs[blockIdx.y];
    const int64_t per = int64_t(j.h) * j.w;
    const int64_t e = int64_t(blockIdx.x) * blockDim.x + threadIdx.x;
    if (e >= per * j.nplanes)
    {
        return;
    }
    const int z = int(e / per);
    const int rem = int(e - int64_t(z) * per);
    const int x = rem / j.h, y = rem - x * j.h;
    out[int64_t(blockIdx.z) * out_fs + j.out_off + int64_t(z) * j.out_ps + int64_t(x) * j.out_cs + y] =
        in[int64_t(blockIdx.z) * in_fs + j.in_off + int64_t(z) * j.in_ps + rem];
}


namespace
{
// Fork: `ev` recorded on `from`, then each of the n streams streamAt(0 .. n - 1) waits for it.
template <class StreamAt>
int forkStreams(acf_hip_ctx* c, hipStream_t from, hipEvent_t ev, size_t n, StreamAt streamAt)
{
    HIPCHK(c, hipEventRecord(ev, from));
    for (size_t i = 0; i < n; i++)
    {
        HIPCHK(c, hipStreamWaitEvent(streamAt(i), ev, 0));
    }
    return ACF_HIP_OK;
}
// Join: c->evJoin[i] recorded on streamAt(i) and `to` waiting for it, stream by stream.
template <class StreamAt>
int joinStreams(acf_hip_ctx* c, size_t n, StreamAt streamAt, hipStream_t to)
{
    for (size_t i = 0; i < n; i++)
    {
        HIPCHK(c, hipEventRecord(c->evJoin[i], streamAt(i)));
        HIPCHK(c, hipStreamWaitEvent(to, c->evJoin[i], 0));
    }
    return ACF_HIP_OK;
}
int kidsFork(acf_hip_ctx* c)
{
    return forkStreams(c, c->stream, c->evFork, c->kids.size(), [c](size_t i) { return c->kids[i]->stream; });
}
int kidsJoin(acf_hip_ctx* c)
{
    return joinStreams(c, c->kids.size(), [c](size_t i) { return c->kids[i]->stream; }, c->stream);
}
// fn(kid, first, n) for every child that owns frames of a batch of nF (child i: [i * chunk, min(nF, (i+1) * chunk))), forked from
// and joined into c's stream; the first failure returns its code with the child's text on c
template <class Fn>
int forEachKid(acf_hip_ctx* c, int nF, Fn fn)
{
    int rc = kidsFork(c);
    for (size_t i = 0; i < c->kids.size() && !rc; i++)
    {
        const int first = int(i) * c->kidChunk, n = std::min(nF - first, c->kidChunk);
        if (n > 0 && (rc = fn(c->kids[i], first, n)))
        {
            return fail(c, rc, c->kids[i]->err);
        }
    }
    return rc ? rc : kidsJoin(c);
}
// fn(ctx, frame) for one frame of the last batch: on a context with children, on the child that owns the frame with the frame's
// index within it (outOfRange: the reader's own text for a frame outside the batch); a child's failure leaves its text on c
template <class Fn>
int onFrameOwner(acf_hip_ctx* c, int frame, const char* outOfRange, Fn fn)
{
    if (!c || c->kids.empty())
    {
        return fn(c, frame);
    }
    if (frame < 0 || frame >= c->lastBatch)
    {
        return fail(c, ACF_HIP_E_INVALID, outOfRange);
    }
    acf_hip_ctx* k = c->kids[size_t(frame / c->kidChunk)];
    const int rc = fn(k, frame % c->kidChunk);
    return rc == ACF_HIP_OK ? rc : fail(c, rc, k->err);
}
// A whole run of nF frames on a context with children: run(kid, the kid's first frame, its count) on every child's share; then the
// parent holds the batch (`who` names the entry in the text for a bad nF)
template <class Run>
int runOnKids(acf_hip_ctx* c, const char* who, const float* frames, int nF, Run run)
{
    if (!frames || nF <= 0 || nF > c->maxBatch)
    {
        return fail(c, ACF_HIP_E_INVALID, std::string(who) + ": n_frames out of range");
    }
    const size_t per = size_t(c->plan.d_in) * c->plan.H * c->plan.W;
    const int rc = forEachKid(c, nF, [&](acf_hip_ctx* k, int first, int n) { return run(k, frames + first * per, n); });
    if (!rc)
    {
        c->lastBatch = nF;
        c->pyramidValid = c->detectValid = true;
        c->viewRun = false;
    }
    return rc;
}
} // namespace

// option cascade_turns: the last submission of every device per kernel class (an event owned by the submitting context)
namespace
{
std::mutex g_turnMu;
hipEvent_t g_turnLast[2][64] = {};
// which: 0 = the tile kernel, 1 = the level kernel; chain: whose turns it takes (0 / 1)
// (on c->stream: the levels and the cascade always run on the context's own stream)
int turnBegin(acf_hip_ctx* c, int which, int chain)
{
    if (c->device < 0 || c->device >= 64)
    {
        return ACF_HIP_OK;
    }
    if (!c->evTurn[which])
    {
        HIPCHK(c, hipEventCreateWithFlags(&c->evTurn[which], hipEventDisableTiming));
    }
    std::lock_guard<std::mutex> lk(g_turnMu);
    hipEvent_t last = g_turnLast[chain][c->device];
    if (last && last != c->evTurn[0] && last != c->evTurn[1])
    {
        HIPCHK(c, hipStreamWaitEvent(c->stream, last, 0));
    }
    return ACF_HIP_OK;
}
int turnEnd(acf_hip_ctx* c, int which, int chain)
{
    if (!c->evTurn[which] || c->device < 0 || c->device >= 64)
    {
        return ACF_HIP_OK;
    }
    std::lock_guard<std::mutex> lk(g_turnMu);
    HIPCHK(c, hipEventRecord(c->evTurn[which], c->stream));
    g_turnLast[chain][c->device] = c->evTurn[which];
    return ACF_HIP_OK;
}
void cascTurnForget(acf_hip_ctx* c)
{
    std::lock_guard<std::mutex> lk(g_turnMu);
    for (int w = 0; w < 2; w++)
    {
        if (c->evTurn[w])
        {
            for (int ch = 0; ch < 2; ch++)
            {
                if (c->device >= 0 && c->device < 64 && g_turnLast[ch][c->device] == c->evTurn[w])
                {
                    g_turnLast[ch][c->device] = nullptr;
                }
            }
            (void)hipEventDestroy(c->evTurn[w]);
            c->evTurn[w] = nullptr;
        }
    }
}
} // namespace

extern "C" {


int acf_hip_abi_version(void)
{
    return ACF_HIP_ABI_VERSION;
}

// The side streams of a context (real scales beside each other, level groups): created when something first forks.
// The HIP runtime multiplexes all streams of a process onto GPU_MAX_HW_QUEUES (default 4) hardware queues, and kernels of
// two streams that share a queue never overlap: with seven streams per context the main streams of three contexts
// shared queues (rocprofv3 timeline: never more than two kernels at once; profiles/timeline.py).
constexpr int ACF_SIDE_STREAMS = 6;
constexpr int LEVEL_MAX_R_REAL = 9; // k_level<R, LM_REAL> is instantiated up to nine rows per lane (a 4K frame's 540-cell level), resampling forms up to eight
static void ensureSide(acf_hip_ctx* c)
{
    while (int(c->side.size()) < std::min<int>(ACF_SIDE_STREAMS, int(c->evJoin.size())))
    {
        hipStream_t st;
        if (hipStreamCreateWithFlags(&st, hipStreamNonBlocking) != hipSuccess)
        {
            (void)hipGetLastError();
            break;
        }
        c->side.push_back(st);
    }
}

int acf_hip_create(int device, void* stream, acf_hip_ctx** out)
{
    if (!out)
    {
        return ACF_HIP_E_INVALID;
    }
    *out = nullptr;
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess || n <= 0 || device < 0 || device >= n)
    {
        return ACF_HIP_E_NODEVICE;
    }
    if (hipSetDevice(device) != hipSuccess)
    {
        return ACF_HIP_E_NODEVICE;
    }
    acf_hip_ctx* c = new (std::nothrow) acf_hip_ctx();
    if (!c)
    {
        return ACF_HIP_E_HIP;
    }
    c->device = device;
    {
        hipDeviceProp_t prop;
        if (hipGetDeviceProperties(&prop, device) == hipSuccess)
        {
            c->numCus = prop.multiProcessorCount > 0 ? prop.multiProcessorCount : c->numCus;
            c->ldsPerCu = prop.maxSharedMemoryPerMultiProcessor > 0 ? size_t(prop.maxSharedMemoryPerMultiProcessor) : c->ldsPerCu;
        }
    }
    if (stream)
    {
        c->stream = reinterpret_cast<hipStream_t>(stream);
    }
    else
    {
        if (hipStreamCreateWithFlags(&c->stream, hipStreamNonBlocking) != hipSuccess)
        {
            delete c;
            return ACF_HIP_E_HIP;
        }
        c->ownStream = true;
    }
    // (the side streams themselves are created at their first use, ensureSide: every HIP stream takes a share of the
    // runtime's few hardware queues, and contexts that never fork must not push each other's main streams onto one queue)
    for (int i = 0; i < ACF_SIDE_STREAMS; i++)
    {
        hipEvent_t ev;
        if (hipEventCreateWithFlags(&ev, hipEventDisableTiming) == hipSuccess)
        {
            c->evJoin.push_back(ev);
        }
    }
    (void)hipEventCreateWithFlags(&c->evFork, hipEventDisableTiming);
    *out = c;
    return ACF_HIP_OK;
}

int acf_hip_device_count(int* count)
{
    if (!count)
    {
        return ACF_HIP_E_INVALID;
    }
    *count = 0;
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess || n <= 0)
    {
        (void)hipGetLastError();
        return ACF_HIP_E_NODEVICE;
    }
    for (int i = 0; i < n; i++)
    {
        hipDeviceProp_t pr;
        if (hipGetDeviceProperties(&pr, i) == hipSuccess && std::string(pr.gcnArchName).rfind("gfx950", 0) == 0)
        {
            (*count)++;
        }
    }
    return *count > 0 ? ACF_HIP_OK : ACF_HIP_E_NODEVICE;
}

static void dropGraph(acf_hip_ctx* c)
{
    if (!c)
    {
        return;
    }
    bool synced = false;
    for (auto& g : c->graphs)
    {
        if (g.exec)
        {
            if (!synced)
            {
                // (the last replay may still be running: an executable graph is not released under it)
                (void)hipSetDevice(c->device);
                (void)hipStreamSynchronize(c->stream);
                synced = true;
            }
            (void)hipGraphExecDestroy(g.exec);
        }
        g = acf_hip_ctx::GraphSlot();
    }
    c->graphNext = 0;
    c->plainRuns = 0; // the next run is a plain one again (it may allocate: NMS buffers, side streams)
}

// acf_hip_evaluate_crops' copy of the classifier (crops_run.hip.h: ensureCropModel) goes with the model it was made from
static void dropCropModel(acf_hip_ctx* c)
{
    if (!c)
    {
        return;
    }
    auto& m = c->crop;
    if (m.fids || m.thrs || m.hs || m.child)
    {
        (void)hipSetDevice(c->device);
        (void)hipStreamSynchronize(c->stream); // (a call in flight may be reading it)
        (void)hipFree(m.fids);
        (void)hipFree(m.thrs);
        (void)hipFree(m.hs);
        (void)hipFree(m.child);
    }
    m = acf_hip_ctx::CropModel();
}

int acf_hip_destroy(acf_hip_ctx* c)
{
    dropGraph(c);
    dropCropModel(c);
    if (!c)
    {
        return ACF_HIP_E_INVALID;
    }
    (void)hipSetDevice(c->device);
    (void)hipStreamSynchronize(c->stream);
    (void)acf_hip_stream_close(c);
    cascTurnForget(c);
    dropPlan(c);
    if (c->d_x86 && c->x86Owned)
    {
        (void)hipFree(c->d_x86);
    }
    for (const auto& m : c->evPool)
    {
        (void)hipEventDestroy(m.ev);
    }
    for (hipStream_t st : c->side)
    {
        (void)hipStreamDestroy(st);
    }
    for (hipEvent_t e : c->evJoin)
    {
        (void)hipEventDestroy(e);
    }
    if (c->evFork)
    {
        (void)hipEventDestroy(c->evFork);
    }
    for (hipEvent_t e : c->evScale)
    {
        (void)hipEventDestroy(e);
    }
    if (c->ownStream)
    {
        (void)hipStreamDestroy(c->stream);
    }
    delete c;
    return ACF_HIP_OK;
}

const char* acf_hip_last_error(const acf_hip_ctx* c)
{
    return c ? c->err.c_str() : "null context";
}

// acf_hip_set_option's keys (each described in include/acf_hip.h).  `field` is the Options member the value goes to, in the
// context and in each of its sub-batch children; "graph" and "streams" have none: `after` sets them on the parent alone
// (children never capture graphs; "streams" takes effect at the next acf_hip_plan).
struct OptionKey
{
    const char* key;
    int Options::*field;
    bool nonzero;                               // stores value != 0 (else the value as given)
    bool (*refuse)(const acf_hip_ctx*, int);    // null: any value
    const char* why;                            // acf_hip_last_error of a refused value
    void (*after)(acf_hip_ctx*, int);           // side effect, on every context the value is set on
};

static bool negative(const acf_hip_ctx*, int v)
{
    return v < 0;
}

static const char* const LEVEL_RANGE = "option: level_warm a positive multiple of 4, level_segments >= 0";
static const char* const SMOOTH_RANGE = "option: smooth_segments >= 0, smooth_warm a multiple of 16";

static const OptionKey OPTION_KEYS[] = {
    { "graph", nullptr, false, nullptr, nullptr, [](acf_hip_ctx* c, int v) { c->useGraph = v; c->graphBroken = 0; } },
    { "streams", nullptr, false, [](const acf_hip_ctx*, int v) { return v < 1 || v > 6; }, "streams: 1..6",
        [](acf_hip_ctx* c, int v) { c->nStreams = v; } },
    { "taps", &Options::taps, true },
    { "arith", &Options::arith, true, [](const acf_hip_ctx* c, int v) { return v != 0 && !c->d_x86; },
        "arith: install a CPU's tables first (acf_hip_set_x86_tables)" },
    { "profile", &Options::profile, true, nullptr, nullptr, [](acf_hip_ctx* c, int) { c->evUsed = 0; } },
    { "fused_levels", &Options::fusedLevels, false },
    { "fused_smooth", &Options::fusedSmooth, true },
    { "fused_grad", &Options::fusedGrad, false },
    { "fused_tri", &Options::fusedTri, false },
    { "shared_device", &Options::sharedDevice, true },
    { "cascade_tiles", &Options::cascadeTiles, true },
    { "rank_cells", &Options::rankCells, true, nullptr, nullptr, [](acf_hip_ctx* c, int) { c->detectValid = false; } },
    { "tile_persist", &Options::tilePersist, false },
    { "cascade_turns", &Options::cascadeTurns, false },
    { "scale_streams", &Options::scaleStreams, true },
    { "keep_pyramid", &Options::keepPyramid, true },
    { "count_repairs", &Options::countRepairs, false, negative, LEVEL_RANGE },
    { "level_segments", &Options::levelSegments, false, negative, LEVEL_RANGE },
    { "level_warm", &Options::levelWarm, false, [](const acf_hip_ctx*, int v) { return v < 4 || v % 4 != 0; }, LEVEL_RANGE },
    { "smooth_segments", &Options::smoothSegments, false, negative, SMOOTH_RANGE },
    { "smooth_force_redo", &Options::smoothForceRedo, false, negative, SMOOTH_RANGE },
    { "smooth_warm", &Options::smoothWarm, false, [](const acf_hip_ctx*, int v) { return v < 0 || v % 16 != 0; }, SMOOTH_RANGE },
};

int acf_hip_set_option(acf_hip_ctx* c, const char* key, int value)
{
    if (!c || !key)
    {
        return ACF_HIP_E_INVALID;
    }
    dropGraph(c); // (whatever changes, a captured graph no longer describes the next run)
    const OptionKey* o =
        std::find_if(std::begin(OPTION_KEYS), std::end(OPTION_KEYS), [&](const OptionKey& r) { return !strcmp(key, r.key); });
    if (o == std::end(OPTION_KEYS))
    {
        return fail(c, ACF_HIP_E_INVALID, std::string("unknown option ") + key);
    }
    if (o->refuse && o->refuse(c, value))
    {
        return fail(c, ACF_HIP_E_INVALID, o->why); // (a child holds the parent's d_x86: it would refuse the same values)
    }
    if (!o->field)
    {
        o->after(c, value);
        return ACF_HIP_OK;
    }
    auto set = [&](acf_hip_ctx* t) {
        t->opt.*o->field = o->nonzero ? value != 0 : value;
        if (o->after)
        {
            o->after(t, value);
        }
    };
    set(c);
    for (acf_hip_ctx* k : c->kids)
    {
        set(k);
    }
    for (acf_hip_ctx* m : c->bankCtx)
    {
        set(m);
    }
    return ACF_HIP_OK;
}

int acf_hip_get_scales(int nPerOct, int nOctUp, int minDs_h, int minDs_w, int shrink, int h, int w,
    double* scales, double* shw_h, double* shw_w, int cap, int* n)
{
    if (!n || nPerOct <= 0 || minDs_h <= 0 || minDs_w <= 0 || shrink <= 0)
    {
        return ACF_HIP_E_INVALID;
    }
    ScaleList sl = getScales(nPerOct, nOctUp, minDs_h, minDs_w, shrink, h, w);
    *n = int(sl.scales.size());
    for (int i = 0; i < *n && i < cap; i++)
    {
        if (scales)
        {
            scales[i] = sl.scales[i];
        }
        if (shw_h)
        {
            shw_h[i] = sl.shw_h[i];
        }
        if (shw_w)
        {
            shw_w[i] = sl.shw_w[i];
        }
    }
    return ACF_HIP_OK;
}

int acf_hip_plan_levels(const acf_hip_params* p, int h, int w, int d, acf_hip_level* out, int cap, int* nScales, int* nChns)
{
    if (!p || !nScales)
    {
        return ACF_HIP_E_INVALID;
    }
    Plan plan;
    std::string err;
    int rc = buildPlan(*p, h, w, d, plan, err);
    if (rc)
    {
        return rc;
    }
    *nScales = int(plan.levels.size());
    if (nChns)
    {
        *nChns = plan.nChns;
    }
    for (int i = 0; i < *nScales && i < cap && out; i++)
    {
        out[i] = plan.levels[i];
    }
    return ACF_HIP_OK;
}

// What a classifier must satisfy before a walk is launched on it (include/acf_hip.h, acf_hip_params::child).  Only the nodes that carry a
// feature test are looked at: the first 2^depth - 1 of a fixed-depth tree, the nodes with child != 0 of a variable-depth one; leaves
// and unused slots may hold anything.  nChns > 0: every test's feature id against nChns planes of the model window in cells of `cell`
// pixels (cids[], acfDetect1.cpp:390-406).
static int checkModel(const acf_hip_params& p, int nChns, int cell, std::string& why)
{
    if (p.nTrees <= 0 || p.nTreeNodes <= 0 || !p.fids || !p.thrs || !p.hs)
    {
        why = "empty classifier";
        return ACF_HIP_E_INVALID;
    }
    if (p.treeDepth < 0 || p.treeDepth > 8)
    {
        why = "treeDepth must be 0..8 (acfDetect1.cpp:204-226)";
        return ACF_HIP_E_INVALID;
    }
    if (p.treeDepth == 0 && !p.child)
    {
        why = "treeDepth 0 needs child[]";
        return ACF_HIP_E_INVALID;
    }
    if (p.treeDepth > 0 && p.nTreeNodes < (1 << (p.treeDepth + 1)) - 1)
    {
        why = "nTreeNodes too small for treeDepth";
        return ACF_HIP_E_INVALID;
    }
    if (p.stride <= 0 || p.shrink <= 0 || cell <= 0 || p.modelDsPad_h % p.shrink || p.modelDsPad_w % p.shrink)
    {
        why = "stride/shrink/modelDsPad";
        return ACF_HIP_E_INVALID;
    }
    const uint64_t nF = nChns > 0 ? uint64_t(nChns) * uint64_t(p.modelDsPad_h / cell) * uint64_t(p.modelDsPad_w / cell) : 0;
    const int nInternal = p.treeDepth > 0 ? (1 << p.treeDepth) - 1 : 0;
    for (int t = 0; t < p.nTrees; t++)
    {
        for (int k = 0; k < p.nTreeNodes; k++)
        {
            const size_t q = size_t(t) * p.nTreeNodes + k;
            const bool test = p.treeDepth > 0 ? k < nInternal : p.child[q] != 0;
            // next node = child[k] - (ftr < thr), in 0-based terms child[k] - 1 or child[k] (acfDetect1.cpp:146-155): both must stay
            // inside the tree AND lie after k — trees are stored parent-first, and a backward or self reference in an untrusted
            // model file would make the walk `while (child[k])` spin forever on the GPU
            if (p.treeDepth == 0 && test && (p.child[q] >= uint32_t(p.nTreeNodes) || p.child[q] - 1 <= uint32_t(k)))
            {
                why = "child[] of tree " + std::to_string(t) + ", node " + std::to_string(k) + " is " + std::to_string(p.child[q]) +
                    ": the pair child - 1, child must lie after its parent and inside the tree's " + std::to_string(p.nTreeNodes) + " nodes";
                return ACF_HIP_E_INVALID;
            }
            if (nChns > 0 && test && p.fids[q] >= nF)
            {
                why = "feature id out of range for modelDsPad/shrink/channels (tree " + std::to_string(t) + ", node " + std::to_string(k) + ": " +
                    std::to_string(p.fids[q]) + " of " + std::to_string(nF) + ")";
                return ACF_HIP_E_INVALID;
            }
        }
    }
    return ACF_HIP_OK;
}

int acf_hip_check_model(const acf_hip_params* p, int nChns, char* why, int cap)
{
    std::string err;
    int rc = ACF_HIP_E_INVALID;
    if (!p || nChns < 0)
    {
        err = "check_model: arguments";
    }
    else
    {
        rc = checkModel(*p, nChns, p->shrink, err);
    }
    if (why && cap > 0)
    {
        std::snprintf(why, size_t(cap), "%s", err.c_str());
    }
    return rc;
}

int acf_hip_set_model(acf_hip_ctx* c, const acf_hip_params* p)
{
    dropGraph(c);
    dropCropModel(c);
    if (!c || !p)
    {
        return ACF_HIP_E_INVALID;
    }
    {
        // the structure alone (nChns = 0: the channels a call scores on are not known yet): no entry launches a walk on a model
        // that did not pass here
        std::string why;
        if (const int rc = checkModel(*p, 0, p->shrink, why))
        {
            return fail(c, rc, "set_model: " + why);
        }
    }
    if (p->nOrients < 1 || p->nOrients > 12)
    {
        return fail(c, ACF_HIP_E_UNSUPPORTED, "set_model: nOrients must be 1..12");
    }
    const bool ldcf = p->ldcfK > 0 && p->ldcfFilters;
    if (ldcf && (p->ldcfK > 16 || p->modelDsPad_h % (2 * p->shrink) || p->modelDsPad_w % (2 * p->shrink)))
    {
        return fail(c, ACF_HIP_E_INVALID, "set_model: LDCF needs 1..16 filters per channel and modelDsPad divisible by 2*shrink");
    }
    const size_t n = size_t(p->nTrees) * p->nTreeNodes;
    c->p = *p;
    c->ldcfFilters.clear();
    c->p.ldcfK = ldcf ? p->ldcfK : 0;
    c->p.ldcfFilters = nullptr;
    if (ldcf)
    {
        const int dcol = p->colorSpace == ACF_HIP_CS_GRAY ? 1 : 3;
        const int nC = (p->colorEnabled ? dcol : 0) + (p->gradMagEnabled ? 1 : 0) + (p->gradHistEnabled ? p->nOrients : 0);
        c->ldcfFilters.assign(p->ldcfFilters, p->ldcfFilters + size_t(p->ldcfK) * nC * 25);
        c->p.ldcfFilters = c->ldcfFilters.data();
    }
    c->fids.assign(p->fids, p->fids + n);
    c->thrs.assign(p->thrs, p->thrs + n);
    c->hs.assign(p->hs, p->hs + n);
    if (p->child)
    {
        c->child.assign(p->child, p->child + n);
    }
    else
    {
        c->child.assign(n, 0u);
    }
    c->p.fids = c->fids.data();
    c->p.thrs = c->thrs.data();
    c->p.hs = c->hs.data();
    c->p.child = c->child.data();
    c->hasModel = true;
    c->bank.clear(); // (the members were checked against the previous model)
    if (c->hasPlan)
    {
        (void)hipStreamSynchronize(c->stream);
        dropPlan(c); // (built for the previous model; a refused model, above, leaves it and the children as they were)
    }
    return ACF_HIP_OK;
}

#include "cascade_plan.hip.h"  // splitFid, pooledTileLds, buildTileSet, buildCascadeTables, allocCascadeRun

#include "resample_plan.hip.h" // stripPlan, launchStrip, resampleTilePlan

#include "plan_build.hip.h" // acf_hip_plan's stages (PlanBuild), after the helpers they call

static int planBank(acf_hip_ctx* c, int max_batch, int max_hits); // (bank_run.hip.h)

// acf_hip_plan's work on a context that dropPlan has just left without a plan
static int planFresh(acf_hip_ctx* c, int H, int W, int d_in, int max_batch, int max_hits)
{
    const acf_hip_params& p = c->p;
    int rc = buildPlan(p, H, W, d_in, c->plan, c->err);
    if (rc)
    {
        return rc;
    }
    c->maxBatch = max_batch;
    c->maxHits = max_hits;
    if (c->nStreams > 1 && max_batch >= 2 * c->nStreams && c->evFork && int(c->evJoin.size()) >= c->nStreams)
    {
        // sub-batch contexts: this context keeps only the plan's geometry; every device buffer lives in a child
        c->kidChunk = (max_batch + c->nStreams - 1) / c->nStreams;
        for (int i = 0; i < c->nStreams; i++)
        {
            acf_hip_ctx* k = nullptr;
            if ((rc = acf_hip_create(c->device, nullptr, &k)))
            {
                return fail(c, rc, "plan: cannot create a sub-batch context");
            }
            c->kids.push_back(k);
            k->opt = c->opt;
            k->d_x86 = c->d_x86; // (the parent's tables; the parent frees them)
            k->nmsOn = c->nmsOn; // (acf_hip_set_nms before the plan, or a re-plan: the new children run what the parent reports)
            k->nms = c->nms;
            if ((rc = acf_hip_set_model(k, &c->p)) || (rc = acf_hip_plan(k, H, W, d_in, c->kidChunk, max_hits)))
            {
                return fail(c, rc, k->err);
            }
        }
        return ACF_HIP_OK;
    }
    // smoothing radii the recursion kernel implements (convTri.cpp:215-218)
    for (double r : { p.colorSmooth, p.smooth })
    {
        if (!(r == 0.0 || (r > 0 && r <= 1.0)))
        {
            return fail(c, ACF_HIP_E_UNSUPPORTED, "plan: smoothing radius must be 0 or in (0,1]");
        }
    }
    if (p.normRad < 0 || p.normRad == 1 || p.normRad > 15)
    {
        return fail(c, ACF_HIP_E_UNSUPPORTED, "plan: normRad must be 0 or 2..15");
    }
    if ((rc = ensureConstTables(c)))
    {
        return rc;
    }
    PlanBuild b(c, H, W, d_in, max_batch, max_hits);
    if ((rc = b.colourBuffer()) || (rc = b.realScales()) || (rc = b.imageStrips()) || (rc = b.approxLevels()) || (rc = b.finalJobs()) || (rc = b.levelJobs()) ||
        (rc = b.ldcf()) || (rc = b.uploadAndScratch()) || (rc = b.cascade()) || (rc = planBank(c, max_batch, max_hits)))
    {
        return rc;
    }
    c->h_counts.assign(size_t(max_batch), 0);
    return ACF_HIP_OK;
}

int acf_hip_plan(acf_hip_ctx* c, int H, int W, int d_in, int max_batch, int max_hits)
{
    dropGraph(c);
    if (int rc = needModel(c, "plan")) return rc;
    if (max_batch <= 0 || max_hits <= 0)
    {
        return fail(c, ACF_HIP_E_INVALID, "plan: max_batch/max_hits");
    }
    HIPCHK(c, hipSetDevice(c->device));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    (void)acf_hip_stream_close(c); // its slots are sized by the plan
    dropPlan(c);
    // (a plan refused from here on leaves none: what it had built goes at once)
    if (const int rc = planFresh(c, H, W, d_in, max_batch, max_hits))
    {
        dropPlan(c);
        return rc;
    }
    c->hasPlan = true;
    return ACF_HIP_OK;
}

int acf_hip_num_levels(const acf_hip_ctx* c, int* nScales, int* nChns)
{
    if (int rc = needPlanRead(c, "num_levels")) return rc;
    if (nScales)
    {
        *nScales = int(c->plan.levels.size());
    }
    if (nChns)
    {
        *nChns = c->plan.nChns;
    }
    return ACF_HIP_OK;
}

int acf_hip_get_levels(const acf_hip_ctx* c, acf_hip_level* out, int cap)
{
    if (int rc = needPlanRead(c, "get_levels")) return rc;
    if (!out || cap < int(c->plan.levels.size()))
    {
        return fail(c, ACF_HIP_E_INVALID, "get_levels: capacity");
    }
    std::copy(c->plan.levels.begin(), c->plan.levels.end(), out);
    return ACF_HIP_OK;
}

int acf_hip_get_ldcf_levels(const acf_hip_ctx* c, acf_hip_level* out, int cap)
{
    if (!c || !c->hasPlan || !out)
    {
        return ACF_HIP_E_INVALID;
    }
    const acf_hip_ctx* src = c->kids.empty() ? c : c->kids[0];
    if (src->p.ldcfK <= 0 || src->ldcf.levels.empty())
    {
        return ACF_HIP_E_INVALID;
    }
    const int n = std::min(cap, int(src->ldcf.levels.size()));
    std::copy(src->ldcf.levels.begin(), src->ldcf.levels.begin() + n, out);
    return ACF_HIP_OK;
}

int acf_hip_pyramid_floats(const acf_hip_ctx* c, int64_t* n)
{
    if (int rc = needPlanRead(c, "pyramid_floats")) return rc;
    *n = c->plan.pyr_floats;
    return ACF_HIP_OK;
}

int acf_hip_get_repairs(acf_hip_ctx* c, int64_t out[4])
{
    if (!c || !out)
    {
        return ACF_HIP_E_INVALID;
    }
    for (int i = 0; i < 4; i++)
    {
        out[i] = c->repairs[i];
        for (const acf_hip_ctx* k : c->kids)
        {
            out[i] += k->repairs[i];
        }
    }
    return ACF_HIP_OK;
}

int acf_hip_get_tri_forms(const acf_hip_ctx* c, int32_t* out, int cap, int* n)
{
    if (int rc = needPlanRead(c, "get_tri_forms")) return rc;
    if (!n || (cap > 0 && !out))
    {
        return ACF_HIP_E_INVALID;
    }
    const acf_hip_ctx* s = c->kids.empty() ? c : c->kids[0]; // (sub-batch children hold the buffers; they all run the same forms)
    *n = int(s->real.size());
    for (int i = 0; i < *n && i < cap; i++)
    {
        out[i] = s->real[size_t(i)].triForm;
    }
    return ACF_HIP_OK;
}

int acf_hip_get_level_forms(const acf_hip_ctx* c, int32_t* out, int cap, int* n)
{
    if (int rc = needPlanRead(c, "get_level_forms")) return rc;
    if (!n || (cap > 0 && !out))
    {
        return ACF_HIP_E_INVALID;
    }
    const acf_hip_ctx* s = c->kids.empty() ? c : c->kids[0]; // (sub-batch children hold the plan's job lists; they all run the same forms)
    const int nL = int(s->levelFormFused.size());
    *n = ACF_HIP_LF_HEAD + nL;
    for (int i = 0; i < ACF_HIP_LF_HEAD && i < cap; i++)
    {
        out[i] = s->levelCallForm[i];
    }
    const int path = s->levelCallForm[0];
    const int32_t form = 0xffff, why = ~form, taker = 3 << 12;
    for (int i = 0; i < nL && ACF_HIP_LF_HEAD + i < cap; i++)
    {
        const int32_t f = s->levelFormFused[size_t(i)], r = s->levelFormRaw[size_t(i)];
        out[ACF_HIP_LF_HEAD + i] = (f & why) | (path == ACF_HIP_LV_WAVE_SMOOTH ? r & form : path == ACF_HIP_LV_FUSED ? f & form : f & form & ~taker);
    }
    return ACF_HIP_OK;
}

int acf_hip_get_scale_forms(const acf_hip_ctx* c, int32_t* out, int cap, int* n)
{
    if (int rc = needPlanRead(c, "get_scale_forms")) return rc;
    if (!n || (cap > 0 && !out))
    {
        return ACF_HIP_E_INVALID;
    }
    const acf_hip_ctx* s = c->kids.empty() ? c : c->kids[0]; // (sub-batch children hold the real scales; they all take the same routes)
    *n = int(s->real.size());
    for (int i = 0; i < *n && i < cap; i++)
    {
        // the run's side as imageResample wrote it, the plan's side as imageStrips / stripPlan left it
        const RealScale& rs = s->real[size_t(i)];
        out[i] = int32_t(uint32_t(rs.scaleForm) | (rs.strip.ok ? ACF_HIP_SF_PLAN_STRIP : 0) | (rs.stripPair.ok ? ACF_HIP_SF_PLAN_PAIR : 0) |
            uint32_t(rs.strip.why) << 24 | uint32_t(rs.stripPair.why) << 28);
    }
    return ACF_HIP_OK;
}

int acf_hip_get_cascade_forms(const acf_hip_ctx* c, int32_t* out, int cap, int* n)
{
    if (int rc = needCtx(c)) return rc;
    if (!n || (cap > 0 && !out))
    {
        return ACF_HIP_E_INVALID;
    }
    // (sub-batch children run the pipeline's cascades, all in the same forms; the operator's runs on the context itself)
    const acf_hip_ctx* s = !c->kids.empty() && c->kids[0]->cascadeFormSeq > c->cascadeFormSeq ? c->kids[0] : c;
    *n = ACF_HIP_CF_WORDS;
    std::copy(s->cascadeForm, s->cascadeForm + std::max(0, std::min(cap, ACF_HIP_CF_WORDS)), out);
    return ACF_HIP_OK;
}

int acf_hip_tri_ck_layout(int h, int w, int x, int y, int64_t out[2])
{
    if (!out || h <= 0 || w <= 0 || x < 0 || x >= w || y < 0 || y >= h)
    {
        return ACF_HIP_E_INVALID;
    }
    out[0] = triCkIndex(x, y, triCkBlockRows(h));
    out[1] = triCkFloats(h, w);
    return ACF_HIP_OK;
}

int acf_hip_get_lambdas(acf_hip_ctx* c, int frame, double out[3])
{
    if (!c || !out)
    {
        return ACF_HIP_E_INVALID;
    }
    return onFrameOwner(c, frame, "get_lambdas: frame out of range", [&](acf_hip_ctx* c, int frame) -> int {
        if (!c->hasPlan || !c->pyramidValid)
        {
            return fail(c, ACF_HIP_E_NOPLAN, "get_lambdas: no pyramid");
        }
        if (frame < 0 || frame >= c->lastBatch)
        {
            return fail(c, ACF_HIP_E_INVALID, "get_lambdas: frame out of range");
        }
        for (int j = 0; j < 3; j++)
        {
            out[j] = c->h_lambdas[size_t(frame) * 3 + j];
        }
        return ACF_HIP_OK;
    });
}

// A/B knob: ACF_HIP_RESAMPLE_GENERIC forces the gather kernel for the image resamples (read once)
static bool resampleGenericOnly()
{
    const bool v = fallbackForced(FB_RESAMPLE_GENERIC);
    return v;
}

// k_resample_up applies: both axes up-sampled, whole quads of output rows, 16-byte aligned planes
static bool resampleUpOk(const ResampleDesc& d)
{
    const bool off = fallbackForced(FB_RESAMPLE_NO_UP);
    return !off && d.xmode == RS_UP && d.ymode == RS_UP && d.hb % 4 == 0 && d.ha >= 4 && d.dst_off % 4 == 0 && d.dst_frame_stride % 4 == 0;
}

namespace
{
// A call that fails between a verify launch and its repair launch (a launch error, the count_repairs read-back) would leave
// repair flags set for the next call — harmless for results (a flagged plane is recomputed as one chain), but counted by
// count_repairs and paid for.  Every failing pyramid call therefore takes the flags down again.
static void clearRepairFlags(acf_hip_ctx* c)
{
    if (c->d_redo && c->redoInts)
    {
        (void)hipMemsetAsync(c->d_redo, 0, sizeof(int32_t) * c->redoInts, c->stream);
    }
    if (c->d_lvRedo && c->lvRedoInts)
    {
        (void)hipMemsetAsync(c->d_lvRedo, 0, sizeof(int32_t) * c->lvRedoInts, c->stream);
    }
}

} // namespace

#include "input_run.hip.h"   // u8Geom and the description checks, planIngest (IngestPlan), launchColour, the resize tables, the input entries

#include "pyramid_run.hip.h" // PyramidRun (acf_hip_pyramid's stages), pyramidBody

namespace
{
int pyramidImpl(acf_hip_ctx* c, const FrameSource& src, int nF)
{
    const int rc = pyramidBody(c, src, nF);
    if (rc && c && c->hasPlan && c->kids.empty())
    {
        clearRepairFlags(c);
    }
    return rc;
}
} // namespace

int acf_hip_pyramid(acf_hip_ctx* c, const float* frames, int nF)
{
    return pyramidImpl(c, FrameSource{ SRC_F32, frames }, nF);
}

#include "cascade_run.hip.h"    // wholeCascadeTiled, planCascadeCall, clearCounters, runCascade, launchNms, runLdcf

int acf_hip_detect(acf_hip_ctx* c)
{
    if (c && !c->kids.empty())
    {
        if (!c->pyramidValid)
        {
            return fail(c, ACF_HIP_E_INVALID, "detect: no pyramid (call acf_hip_pyramid)");
        }
        const int rc = forEachKid(c, c->lastBatch, [](acf_hip_ctx* k, int, int) { return acf_hip_detect(k); });
        if (!rc)
        {
            c->detectValid = true;
        }
        return rc;
    }
    if (int rc = needPlan(c, "detect")) return rc;
    if (!c->pyramidValid)
    {
        return fail(c, ACF_HIP_E_INVALID, "detect: no pyramid (call acf_hip_pyramid)");
    }
    HIPCHK(c, hipSetDevice(c->device));
    const bool ldcf = c->p.ldcfK > 0;
    const int nF = c->lastBatch;
    const CascInput in = { ldcf ? c->ldcf.d_pyr : c->d_pyr, ldcf ? c->ldcf.floats : c->plan.pyr_floats, nF, c->plan.nChns * std::max(c->p.ldcfK, 1) };
    if (!ldcf && !c->floatPyramid && planCascadeCall(c, c->cs, in, true).readsFloats(c->ranksValid))
    {
        // (options changed between acf_hip_pyramid and acf_hip_detect: the float cells this path reads were never written)
        return fail(c, ACF_HIP_E_INVALID, "detect: the float pyramid of this batch was not written (keep_pyramid = 0) and the selected cascade reads floats");
    }
    int rc;
    if ((ldcf && (rc = runLdcf(c, nF))) || (rc = runCascade(c, c->cs, in, c->d_boxLevels, &c->ranksValid)) || (nmsRequested(c) && (rc = launchNms(c, nF))))
    {
        return rc;
    }
    prof(c, c->stream, "(end)");
    c->countsFetched = false;
    c->detectValid = true;
    return ACF_HIP_OK;
}

// A captured run replayed: the launches, then the host-side state that pyramidBody / acf_hip_detect's host code left at the capture
// (the batch and both results valid, which pyramids were written, the counts on the host not this run's)
static int graphReplay(acf_hip_ctx* c, const acf_hip_ctx::GraphSlot& gs)
{
    HIPCHK(c, hipGraphLaunch(gs.exec, c->stream));
    static_cast<LastRun&>(*c) = gs.after;
    return ACF_HIP_OK;
}

// acf_hip_run knows that the cascade follows the pyramid: the tiled cascade's counters (hit counts; its queue's count and head and the
// tile counters) are cleared in front of the pyramid's launches instead of between the level kernel and the cascade, where a single
// frame waits for every node of the chain (runCascade then skips clearCounters: CascadeCall::countersCleared)
static int preZeroCounters(acf_hip_ctx* c, int nF)
{
    if (!c || !c->hasPlan || !c->kids.empty() || !wholeCascadeTiled(c, c->cs) || c->p.ldcfK > 0 || !c->cs.d_counts || !c->cs.d_qcounts || nF <= 0 ||
        nF > c->maxBatch)
    {
        return ACF_HIP_OK;
    }
    HIPCHK(c, hipSetDevice(c->device));
    const int rc = clearCounters(c, c->cs, planCascadeCall(c, c->cs, { c->d_pyr, c->plan.pyr_floats, nF, c->plan.nChns }, true));
    c->countersZeroed = !rc;
    return rc;
}

// acf_hip_run's work: the pyramid, then the cascade with its counters cleared early
static int pyramidThenDetect(acf_hip_ctx* c, const float* frames, int nF)
{
    int rc = preZeroCounters(c, nF);
    if (!rc)
    {
        rc = acf_hip_pyramid(c, frames, nF);
    }
    if (!rc)
    {
        rc = acf_hip_detect(c);
    }
    if (c)
    {
        c->countersZeroed = false;
    }
    return rc;
}

int acf_hip_run(acf_hip_ctx* c, const float* frames, int nF)
{
    if (c && !c->kids.empty())
    {
        return runOnKids(c, "run", frames, nF, acf_hip_run);
    }
    // option "graph": the launches of this call — same frames pointer, same batch size, nothing in the path that reads back or
    // records events of its own — as one captured graph.  The first calls run plainly (they may allocate); a capture that the
    // runtime refuses switches the option off for this context and the call runs plainly.
    const bool graphable = c && c->useGraph && !c->graphBroken && c->hasPlan && !c->opt.profile && !c->opt.taps && !c->opt.countRepairs && !c->autoLambdas &&
        c->opt.cascadeTurns == 0 && frames && nF > 0 && nF <= c->maxBatch;
    if (graphable)
    {
        for (auto& gs : c->graphs)
        {
            if (gs.exec && gs.frames == frames && gs.after.lastBatch == nF)
            {
                HIPCHK(c, hipSetDevice(c->device));
                return graphReplay(c, gs);
            }
        }
    }
    if (graphable && c->plainRuns >= 1)
    {
        HIPCHK(c, hipSetDevice(c->device));
        acf_hip_ctx::GraphSlot& gs = c->graphs[c->graphNext];
        if (gs.exec)
        {
            (void)hipStreamSynchronize(c->stream); // (a replay of the slot being replaced may still be running)
            (void)hipGraphExecDestroy(gs.exec);
            gs = acf_hip_ctx::GraphSlot();
        }
        hipGraph_t g = nullptr;
        bool ok = hipStreamBeginCapture(c->stream, hipStreamCaptureModeRelaxed) == hipSuccess;
        int rcc = ACF_HIP_OK;
        if (ok)
        {
            rcc = pyramidThenDetect(c, frames, nF);
            ok = hipStreamEndCapture(c->stream, &g) == hipSuccess && g != nullptr && !rcc;
        }
        if (ok)
        {
            ok = hipGraphInstantiate(&gs.exec, g, nullptr, nullptr, 0) == hipSuccess && gs.exec != nullptr;
        }
        if (g)
        {
            (void)hipGraphDestroy(g);
        }
        if (ok)
        {
            gs.frames = frames;
            gs.after = static_cast<const LastRun&>(*c);
            c->graphNext = (c->graphNext + 1) % acf_hip_ctx::GRAPH_SLOTS;
            return graphReplay(c, gs);
        }
        (void)hipGetLastError();
        gs = acf_hip_ctx::GraphSlot();
        c->graphBroken = 1; // (fall through: the plain path below does the work)
    }
    const int rc = pyramidThenDetect(c, frames, nF);
    if (!rc && c)
    {
        c->plainRuns++;
    }
    return rc;
}

int acf_hip_run_host(acf_hip_ctx* c, const float* frames_host, int nF)
{
    if (c && !c->kids.empty())
    {
        return runOnKids(c, "run_host", frames_host, nF, acf_hip_run_host);
    }
    if (int rc = needPlan(c, "run_host")) return rc;
    if (!frames_host || nF <= 0 || nF > c->maxBatch)
    {
        return fail(c, ACF_HIP_E_INVALID, "run_host: n_frames out of range");
    }
    HIPCHK(c, hipSetDevice(c->device));
    const size_t per = size_t(c->plan.d_in) * c->plan.H * c->plan.W;
    if (!c->d_stage)
    {
        int rc = devAlloc(c, &c->d_stage, size_t(c->maxBatch) * per);
        if (rc)
        {
            return rc;
        }
    }
    HIPCHK(c, hipMemcpyAsync(c->d_stage, frames_host, per * nF * sizeof(float), hipMemcpyHostToDevice, c->stream));
    return acf_hip_run(c, c->d_stage, nF);
}

// ---------------------------------------------------------------------------
// streaming front end: copy stream + per-slot events; see include/acf_hip.h
// ---------------------------------------------------------------------------
int acf_hip_stream_close(acf_hip_ctx* c)
{
    if (!c)
    {
        return ACF_HIP_E_INVALID;
    }
    (void)hipSetDevice(c->device);
    if (c->copyStream)
    {
        (void)hipStreamSynchronize(c->copyStream);
    }
    if (c->stream)
    {
        (void)hipStreamSynchronize(c->stream);
    }
    for (auto& s : c->slots)
    {
        if (s.d_in)
        {
            (void)hipFree(s.d_in);
        }
        if (s.d_rec)
        {
            (void)hipFree(s.d_rec);
        }
        if (s.h_rec)
        {
            (void)hipHostFree(s.h_rec);
        }
        if (s.evH2D)
        {
            (void)hipEventDestroy(s.evH2D);
        }
        if (s.evDone)
        {
            (void)hipEventDestroy(s.evDone);
        }
    }
    if (c->copyStream)
    {
        (void)hipStreamDestroy(c->copyStream);
    }
    static_cast<StreamFront&>(*c) = StreamFront{};
    return ACF_HIP_OK;
}

// A stream for batches of `src`: its slots (device input, device and pinned records, events) for up to max_batch frames of frameBytes
// each; replaces an open stream
static int streamSlots(acf_hip_ctx* c, const FrameSource& src, int64_t frameBytes, int cap, int depth)
{
    acf_hip_stream_close(c);
    HIPCHK(c, hipSetDevice(c->device));
    HIPCHK(c, hipStreamCreateWithFlags(&c->copyStream, hipStreamNonBlocking));
    c->stSrc = src;
    c->stFrameBytes = frameBytes;
    c->stCap = cap;
    c->slots.resize(size_t(depth));
    const size_t inBytes = size_t(c->maxBatch) * size_t(frameBytes);
    const size_t recBytes = size_t(c->maxBatch) * (1 + 6 * size_t(cap)) * sizeof(int32_t);
    for (auto& s : c->slots)
    {
        HIPCHK(c, hipMalloc(reinterpret_cast<void**>(&s.d_in), inBytes));
        HIPCHK(c, hipMalloc(reinterpret_cast<void**>(&s.d_rec), recBytes));
        HIPCHK(c, hipHostMalloc(reinterpret_cast<void**>(&s.h_rec), recBytes, hipHostMallocDefault));
        HIPCHK(c, hipEventCreateWithFlags(&s.evH2D, hipEventDisableTiming));
        HIPCHK(c, hipEventCreateWithFlags(&s.evDone, hipEventDisableTiming));
    }
    return ACF_HIP_OK;
}

int acf_hip_stream_open(acf_hip_ctx* c, int pix, int rowStride, int cap, int depth)
{
    if (int rc = needPlan(c, "stream_open")) return rc;
    if (!c->kids.empty())
    {
        return fail(c, ACF_HIP_E_UNSUPPORTED, "stream_open: not available with option \"streams\" > 1");
    }
    if (depth < 2 || depth > 8 || cap <= 0)
    {
        return fail(c, ACF_HIP_E_INVALID, "stream_open: depth must be 2..8, cap > 0");
    }
    // (with acf_hip_set_input_resize the submitted frames are the unreduced ones)
    const int inRows = c->rz.on ? c->rz.rows : c->plan.H, inCols = c->rz.on ? c->rz.cols : c->plan.W;
    U8Geom g;
    if (const char* bad = u8Geom(pix, inRows, inCols, rowStride, c->yuv.chromaOff, c->yuv.frameStride, g))
    {
        return fail(c, ACF_HIP_E_INVALID, std::string("stream_open: ") + bad);
    }
    if (!u8PlanesOk(g, c->plan.d_in))
    {
        return fail(c, ACF_HIP_E_INVALID, "stream_open: the plan's input planes (d) must be 3 for colour layouts (NV12 / NV21 included) and 1 for GRAY");
    }
    return streamSlots(c, FrameSource{ SRC_U8, nullptr, "pyramid_u8", pix, g.stride }, g.frameStride, cap, depth);
}

// The general open for frames described by three planes: every exported stream_open_yuv* / _video call is one call of it that fills in
// what it states (st), as the pyramid entries do (input_run.hip.h).  The call's own arguments first (sourceArgsBad) and, for unreduced
// frames, their size against the plan; then the context and the description; a reduced source's tables where the plan's planes are known.
static int streamOpenYuv(acf_hip_ctx* c, const char* who, const acf_hip_yuv_desc* desc, int64_t frameBytes, Stated st, int srcRows, int srcCols, int orient, double scale,
    const acf_hip_yuv_format* fmt, int cap, int depth)
{
    const std::string w = std::string(who) + ": ";
    if (int rc = needPlan(c, who)) return rc;
    FrameSource src{ SRC_YUV, nullptr, who, 0, 0, {}, {}, false, srcRows, srcCols, scale, orient, fmt ? *fmt : kDefaultVideoFormat };
    if (int rc = sourceArgsBad(c, who, st, src, true)) return rc;
    if (!src.resized)
    {
        if (int rc = sourceAgainstPlan(c, src)) return rc;
    }
    if (!c->kids.empty())
    {
        return fail(c, ACF_HIP_E_UNSUPPORTED, w + "not available with option \"streams\" > 1");
    }
    if (depth < 2 || depth > 8 || cap <= 0)
    {
        return fail(c, ACF_HIP_E_INVALID, w + "depth must be 2..8, cap > 0");
    }
    const char* bad = yuvDescBad(desc);
    if (!bad && src.fmt.bits > 8)
    {
        bad = video16DescBad(nullptr, *desc);
    }
    if (bad)
    {
        return fail(c, ACF_HIP_E_INVALID, w + bad);
    }
    if (c->plan.d_in != 3 || c->rz.on)
    {
        return fail(c, ACF_HIP_E_INVALID, w + "the plan's input planes (d) must be 3, and not with acf_hip_set_input_resize");
    }
    if (src.resized)
    {
        HIPCHK(c, hipSetDevice(c->device));
        if (int rc = sourceAgainstPlan(c, src)) return rc;
    }
    const bool ownSize = srcRows || srcCols; // the frames are srcRows x srcCols, not the plan's size
    int64_t first[3], last[3];
    yuvExtent(*desc, ownSize ? srcRows : c->plan.H, ownSize ? srcCols : c->plan.W, 1, first, last);
    for (int i = 0; i < 3; i++)
    {
        if (first[i] < 0 || last[i] + (src.fmt.bits > 8 ? 1 : 0) >= frameBytes) // (16-bit words: the last byte is the word's high byte)
        {
            return fail(c, ACF_HIP_E_INVALID, w + "every plane of a frame must lie in [0, frame_bytes)");
        }
    }
    if (desc->y.stride_n != frameBytes || desc->u.stride_n != frameBytes || desc->v.stride_n != frameBytes)
    {
        return fail(c, ACF_HIP_E_INVALID, w + "stride_n of every plane must be frame_bytes");
    }
    // (a batch runs under the name of the pyramid entry of its geometry)
    src.who = src.resized ? (orient ? "pyramid_yuv_oriented_resized" : "pyramid_yuv_resized") : (orient ? "pyramid_yuv_oriented" : "pyramid_yuv");
    src.yuv = *desc;
    return streamSlots(c, src, frameBytes, cap, depth);
}

int acf_hip_stream_open_yuv(acf_hip_ctx* c, const acf_hip_yuv_desc* desc, int64_t frameBytes, int cap, int depth)
{
    return streamOpenYuv(c, "stream_open_yuv", desc, frameBytes, ST_PLAN, 0, 0, 0, 0, nullptr, cap, depth);
}

int acf_hip_stream_open_yuv_resized(acf_hip_ctx* c, const acf_hip_yuv_desc* desc, int64_t frameBytes, int srcRows, int srcCols, double scale, int cap, int depth)
{
    return streamOpenYuv(c, "stream_open_yuv_resized", desc, frameBytes, ST_REDUCED, srcRows, srcCols, 0, scale, nullptr, cap, depth);
}

int acf_hip_stream_open_yuv_oriented(acf_hip_ctx* c, const acf_hip_yuv_desc* desc, int64_t frameBytes, int srcRows, int srcCols, int orient, int cap, int depth)
{
    return streamOpenYuv(c, "stream_open_yuv_oriented", desc, frameBytes, ST_TURNED, srcRows, srcCols, orient, 0, nullptr, cap, depth);
}

int acf_hip_stream_open_yuv_oriented_resized(acf_hip_ctx* c, const acf_hip_yuv_desc* desc, int64_t frameBytes, int srcRows, int srcCols, int orient, double scale,
    int cap, int depth)
{
    return streamOpenYuv(c, "stream_open_yuv_oriented_resized", desc, frameBytes, ST_TURNED_REDUCED, srcRows, srcCols, orient, scale, nullptr, cap, depth);
}

int acf_hip_stream_open_video(acf_hip_ctx* c, const acf_hip_yuv_desc* desc, const acf_hip_yuv_format* fmt, int64_t frameBytes, int srcRows, int srcCols, int orient,
    double scale, int cap, int depth)
{
    return streamOpenYuv(c, "stream_open_video", desc, frameBytes, ST_VIDEO, srcRows, srcCols, orient, scale, fmt, cap, depth);
}

int acf_hip_stream_submit(acf_hip_ctx* c, const uint8_t* frames_host, int nF, int* ticket)
{
    if (int rc = needStream(c, "stream_submit")) return rc;
    if (!frames_host || nF <= 0 || nF > c->maxBatch)
    {
        return fail(c, ACF_HIP_E_INVALID, "stream_submit: n_frames out of range");
    }
    const int depth = int(c->slots.size());
    if (c->nextTicket - c->nextCollect >= depth)
    {
        return fail(c, ACF_HIP_E_CAPACITY, "stream_submit: every slot is in flight; collect the oldest ticket first");
    }
    HIPCHK(c, hipSetDevice(c->device));
    acf_hip_ctx::StreamSlot& s = c->slots[size_t(c->nextTicket % depth)];
    // The slot's previous batch was collected (checked above), so its device input and host records are free.
    const size_t bytes = size_t(nF) * size_t(c->stFrameBytes);
    HIPCHK(c, hipMemcpyAsync(s.d_in, frames_host, bytes, hipMemcpyHostToDevice, c->copyStream));
    HIPCHK(c, hipEventRecord(s.evH2D, c->copyStream));
    HIPCHK(c, hipStreamWaitEvent(c->stream, s.evH2D, 0));
    FrameSource src = c->stSrc;
    src.base = s.d_in;
    int rc = runSource(c, src, nF);
    if (rc)
    {
        return rc;
    }
    if ((rc = acf_hip_export_detections(c, s.d_rec, c->stCap)))
    {
        return rc;
    }
    HIPCHK(c, hipMemcpyAsync(s.h_rec, s.d_rec, size_t(nF) * (1 + 6 * size_t(c->stCap)) * sizeof(int32_t), hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipEventRecord(s.evDone, c->stream));
    s.ticket = c->nextTicket;
    s.nFrames = nF;
    if (ticket)
    {
        *ticket = s.ticket;
    }
    c->nextTicket++;
    return ACF_HIP_OK;
}

int acf_hip_stream_collect(acf_hip_ctx* c, int ticket, const int32_t** records, int* nFrames)
{
    if (int rc = needStream(c, "stream_collect")) return rc;
    if (ticket != c->nextCollect || ticket >= c->nextTicket)
    {
        return fail(c, ACF_HIP_E_INVALID, "stream_collect: tickets are collected in submission order");
    }
    acf_hip_ctx::StreamSlot& s = c->slots[size_t(ticket % int(c->slots.size()))];
    HIPCHK(c, hipSetDevice(c->device));
    HIPCHK(c, hipEventSynchronize(s.evDone));
    if (records)
    {
        *records = s.h_rec;
    }
    if (nFrames)
    {
        *nFrames = s.nFrames;
    }
    c->nextCollect++;
    return ACF_HIP_OK;
}

int acf_hip_host_alloc(size_t bytes, void** out)
{
    if (!out || bytes == 0)
    {
        return ACF_HIP_E_INVALID;
    }
    return hipHostMalloc(out, bytes, hipHostMallocDefault) == hipSuccess ? ACF_HIP_OK : ACF_HIP_E_HIP;
}

int acf_hip_host_free(void* p)
{
    return (!p || hipHostFree(p) == hipSuccess) ? ACF_HIP_OK : ACF_HIP_E_HIP;
}

int acf_hip_synchronize(acf_hip_ctx* c)
{
    if (!c)
    {
        return ACF_HIP_E_INVALID;
    }
    for (acf_hip_ctx* k : c->kids)
    {
        HIPCHK(c, hipStreamSynchronize(k->stream));
    }
    HIPCHK(c, hipStreamSynchronize(c->stream));
    return ACF_HIP_OK;
}

static int checkNmsParams(acf_hip_ctx* c, const acf_hip_nms_params* q)
{
    if (q->type < 0 || q->type > 2 || !(q->overlap == q->overlap) || (q->prune && q->maxCount < 0))
    {
        return fail(c, ACF_HIP_E_INVALID, "nms: type 0..2, overlap a number, maxCount >= 0");
    }
    return ACF_HIP_OK;
}

int acf_hip_set_nms(acf_hip_ctx* c, const acf_hip_nms_params* q)
{
    if (!c)
    {
        return ACF_HIP_E_INVALID;
    }
    dropGraph(c);
    if (q)
    {
        const int rc = checkNmsParams(c, q);
        if (rc)
        {
            return rc;
        }
    }
    for (acf_hip_ctx* k : c->kids)
    {
        (void)acf_hip_set_nms(k, q);
    }
    c->nmsOn = q != nullptr;
    if (q)
    {
        c->nms = *q;
    }
    c->detectValid = false; // the resident detections were produced under the previous setting
    return ACF_HIP_OK;
}

#include "readback.hip.h" // fetchCounts, readRecords and the get_* entries, export_detections, read_level / _rank_level / _tap, profile_get

#include "ops.hip.h"      // the single-operator entries (acf_hip_op_*, acf_hip_chns_compute), the x86 tables and the self-tests

#include "crops_run.hip.h" // acf_hip_evaluate_crops / _u8: Detector::evaluate(const cv::Mat&) for a batch (k_crop_score, or staged)

#include "cut_run.hip.h"   // acf_hip_cut_crops / _cut_detections: crops of the stored frame under boxes or the last batch's detections (k_cut_crops)

#include "merge_run.hip.h" // acf_hip_merge_views / _op_merge_views: the views' detections merged into their stored frames (k_merge_views)

#include "bank_run.hip.h"  // acf_hip_set_bank / _detect_bank / _join_bank: a bank of classifiers on one pyramid, their lists joined (k_join_bank)

} // extern "C"
