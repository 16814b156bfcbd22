// cascade_run.hip.h — part of acf_hip.hip (included there and nowhere else): acf_hip_detect's launch logic.
//   pickers           the instantiations of the cascade's kernel templates, named once each (tile3Kernel ... cascadeQueueKernel)
//   planCascadeCall   decides ONCE what a call launches (CascadeCall): the path — depth 2 from LDS tiles (k_cascade_tile3 + tails), or
//                     the staged path with, for depths 1, 3, 4, a tile stage in front (k_cascade_tile3D / tileD) —, cell type, stage
//                     bounds, kernel forms and launch geometry.  cascadePath / wholeCascadeTiled answer from the same code.
//   noteCascadeForms  copies that record into the context for acf_hip_get_cascade_forms (read-only: no launch reads the copy)
//   runCascade        acfDetect1 on every level of a batch, straight down: clearCounters, ensureRankCells, launchTiled2 (+
//                     launchTiled2Tails) or launchTileStageD + launchStages (+ launchStagedTail), then sortHits (k_expand_hits for
//                     stride < shrink, k_sort_map: scale-ordered output + box mapping, ACF.cpp:302-329)
//   launchNms         bbNms + prune of the plan's batch on the device
//   runLdcf           the LDCF post-stage: the pyramid filtered and halved into the LDCF pyramid
// The cascade functions run on the CascState they are given (cell size, capacities, buffers): the plan's, or the one
// acf_hip_op_acf_detect1 built for its caller's buffer.  `ranks` != nullptr says that the cells are the plan's pyramid of the
// current batch: rank cells may stand for them, *ranks tells whether they have been written, and acf_hip_run may have cleared
// the counters already.
#pragma once

extern "C++" // (this file is included inside acf_hip.hip's extern "C" block)
{
// allowLds + the launch of a kernel that takes its arguments as one struct
template <class Args>
static int launchLds(acf_hip_ctx* c, void (*kernel)(Args), dim3 grid, dim3 block, size_t lds, const Args& a)
{
    int rc;
    if ((rc = allowLds(c, reinterpret_cast<const void*>(kernel), lds)))
    {
        return rc;
    }
    hipLaunchKernelGGL(kernel, grid, block, lds, c->stream, a);
    return ACF_HIP_OK;
}
}

// The instantiations of the cascade's kernel templates: the tile kernels by waves per workgroup (NW), tree depth (D, with TB trees
// per batch) and cell type; the staged kernels by mode (2: packed depth-2 table, 1: fixed depth, 0: child walk).
// (The order in which they are first named is their order in the code object.)
using TileKernel = void (*)(TileArgs);
using TileDKernel = void (*)(TileDArgs);
using CascKernel = void (*)(CascArgs);

static TileKernel tile3Kernel(int nw, bool rank)
{
    if (rank)
    {
        switch (nw)
        {
            case 16: return k_cascade_tile3<16, CellRank>;
            case 8: return k_cascade_tile3<8, CellRank>;
            case 4: return k_cascade_tile3<4, CellRank>;
            case 2: return k_cascade_tile3<2, CellRank>;
            default: return k_cascade_tile3<1, CellRank>;
        }
    }
    switch (nw)
    {
        case 16: return k_cascade_tile3<16, CellF32>;
        case 8: return k_cascade_tile3<8, CellF32>;
        case 4: return k_cascade_tile3<4, CellF32>;
        case 2: return k_cascade_tile3<2, CellF32>;
        default: return k_cascade_tile3<1, CellF32>;
    }
}

static TileKernel tail3Kernel(int waves, bool nodesLds)
{
    switch (waves)
    {
        case 4: return nodesLds ? k_cascade_tail3<4, true> : k_cascade_tail3<4, false>;
        case 2: return nodesLds ? k_cascade_tail3<2, true> : k_cascade_tail3<2, false>;
        default: return nodesLds ? k_cascade_tail3<1, true> : k_cascade_tail3<1, false>;
    }
}

static TileDKernel tile3DKernel(int nw, int depth, bool rank)
{
    if (nw == 8)
    {
        switch (depth)
        {
            case 1: return rank ? k_cascade_tile3D<8, 1, 4, CellRank> : k_cascade_tile3D<8, 1, 4, CellF32>;
            case 3: return rank ? k_cascade_tile3D<8, 3, 2, CellRank> : k_cascade_tile3D<8, 3, 2, CellF32>;
            default: return rank ? k_cascade_tile3D<8, 4, 1, CellRank> : k_cascade_tile3D<8, 4, 1, CellF32>;
        }
    }
    switch (depth)
    {
        case 1: return rank ? k_cascade_tile3D<4, 1, 4, CellRank> : k_cascade_tile3D<4, 1, 4, CellF32>;
        case 3: return rank ? k_cascade_tile3D<4, 3, 2, CellRank> : k_cascade_tile3D<4, 3, 2, CellF32>;
        default: return rank ? k_cascade_tile3D<4, 4, 1, CellRank> : k_cascade_tile3D<4, 4, 1, CellF32>;
    }
}

static TileDKernel tileDKernel(int nw, int depth)
{
    if (nw == 8)
    {
        switch (depth)
        {
            case 1: return k_cascade_tileD<8, 1, 4>;
            case 3: return k_cascade_tileD<8, 3, 2>;
            default: return k_cascade_tileD<8, 4, 1>;
        }
    }
    switch (depth)
    {
        case 1: return k_cascade_tileD<4, 1, 4>;
        case 3: return k_cascade_tileD<4, 3, 2>;
        default: return k_cascade_tileD<4, 4, 1>;
    }
}

static CascKernel cascadeFirstKernel(int mode)
{
    switch (mode)
    {
        case 2: return k_cascade_first<2>;
        case 1: return k_cascade_first<1>;
        default: return k_cascade_first<0>;
    }
}

static CascKernel tailScanDKernel(int depth)
{
    switch (depth)
    {
        case 1: return k_tail_scanD<1>;
        case 3: return k_tail_scanD<3>;
        case 4: return k_tail_scanD<4>;
        default: return k_tail_scanD<2>;
    }
}

static CascKernel cascadeTailKernel(int mode)
{
    switch (mode)
    {
        case 2: return k_cascade_tail<2>;
        case 1: return k_cascade_tail<1>;
        default: return k_cascade_tail<0>;
    }
}

static CascKernel cascadeQueueKernel(int mode)
{
    switch (mode)
    {
        case 2: return k_cascade_queue<2>;
        case 1: return k_cascade_queue<1>;
        default: return k_cascade_queue<0>;
    }
}

// The pooled tile kernels' grid for `total` tiles (of all frames) at `lds` bytes per workgroup: one workgroup per tile, or
// persistent workgroups that draw their tiles from one counter per XCD (option tile_persist: 0 one workgroup per tile, 1 as many
// workgroups as the device's CUs hold at once, n > 1 that many; rounded up to a multiple of 8 = the tile counters)
struct TileGrid
{
    unsigned int blocks;
    bool persist;
};

static TileGrid tileGrid(const acf_hip_ctx* c, size_t lds, int64_t total)
{
    const int64_t perX = (total + 7) / 8;
    const int64_t resident = int64_t(c->numCus) * std::max<int64_t>(1, int64_t(c->ldsPerCu) / int64_t((lds + 1279) / 1280 * 1280));
    const int64_t gridP = c->opt.tilePersist > 1 ? int64_t(c->opt.tilePersist) : resident;
    const bool persist = c->opt.tilePersist > 0 && (gridP + 7) / 8 * 8 < perX * 8;
    return { (unsigned int)(persist ? (gridP + 7) / 8 * 8 : perX * 8), persist };
}

// What the cascade runs on: nF frames of nChns channels, frame f's cells at pyr + f * pyr_fs
struct CascInput
{
    const float* pyr;
    int64_t pyr_fs;
    int nF, nChns;
};

enum class CascPath
{
    None,   // no windows: nothing but the (empty) sort
    Tiled2, // depth 2 with a tile set: k_cascade_tile3 takes every window, its tails the survivors
    Staged  // k_cascade_first / _queue / _tail over the stage bounds; depths 1, 3, 4 with a tile set: a tile kernel in front
};

// a tile kernel may run: there is a tile set (stride a multiple of shrink, a form that fits) and option cascade_tiles is on
static inline bool tilesOn(const acf_hip_ctx* c, const CascState& cs)
{
    return cs.tiles.ok && c->opt.cascadeTiles;
}

// the path of a cascade on cs under the context's options (the ONE statement; planCascadeCall builds on it)
static CascPath cascadePath(const acf_hip_ctx* c, const CascState& cs)
{
    if (tilesOn(c, cs) && c->p.treeDepth == 2)
    {
        return CascPath::Tiled2;
    }
    return cs.blocksPerFrame > 0 ? CascPath::Staged : CascPath::None;
}

// acf_hip_run clears the counters in front of the pyramid's launches for this path only
static inline bool wholeCascadeTiled(const acf_hip_ctx* c, const CascState& cs)
{
    return cascadePath(c, cs) == CascPath::Tiled2;
}

// Everything one runCascade decides, decided once (planCascadeCall); the launch functions below only read it.
struct CascadeCall
{
    CascInput in{};
    CascPath path = CascPath::None;
    bool countersCleared = false; // acf_hip_run has cleared this call's counters already (preZeroCounters)
    bool rank = false;            // rank cells stand for the floats in the tile kernel (and, depth 2, in the tail)
    // the tile launch (Tiled2: k_cascade_tile3; Staged: k_cascade_tile3D on a pooled set, else k_cascade_tileD); ts == nullptr: none
    const TileSet* ts = nullptr;
    size_t tileLds = 0;
    TileGrid grid{};
    TileKernel tile3 = nullptr;
    TileDKernel tileD = nullptr;
    // Staged: stage s evaluates trees [s ? bounds[s - 1] : 0, bounds[s]) (see kernels.hip.h: [0,16) [16,32) [32,128) [128,nTrees));
    // the tile kernel stands for stages [0, firstStage)
    int bounds[4] = { 0, 0, 0, 0 }, nStages = 0, firstStage = 0;
    int mode = 0;            // of the staged kernels (see the pickers)
    size_t winBytes = 0;     // a window's float cells: the dynamic LDS of the kernels with a wave per window
    // what finishes the survivors of the last tile stage / queue stage:
    bool codeScan = false;   // leaf codes of the first codes.cap queue entries + their ordered scan (k_tail_scan / k_tail_scanD)
    bool pooledTail = false; // Staged: k_cascade_tile3D has written those leaf codes, else k_tail_codesD does
    bool waveTail = false;   // a wave per queue entry (beyond the codes): k_cascade_tail_rank / _tail3 (Tiled2), k_cascade_tail (Staged)
    // (the k_rank launch that `rank` may need reads the float pyramid as well)
    bool readsFloats(bool ranksWritten) const
    {
        return !(path == CascPath::Tiled2 && rank && ranksWritten);
    }
};

static void planTiled2(const acf_hip_ctx* c, const CascState& cs, CascadeCall& call)
{
    const bool tail = cs.tiles.g.b[4] < c->p.nTrees; // (both sets end their tile kernel at the same tree)
    call.codeScan = tail && cs.codes.cap > 0;
    call.waveTail = tail;
    if (cs.tiles.nTiles > 0)
    {
        const TileSet& ts = call.rank ? cs.tilesR : cs.tiles; // the rank form has its own tile geometry, tile list and node records
        call.ts = &ts;
        call.tileLds = pooledTileLds(ts.g, call.rank ? 2 : 4, TILE3_LEAF_BYTES);
        call.grid = tileGrid(c, call.tileLds, int64_t(ts.nTiles) * call.in.nF);
        call.tile3 = tile3Kernel(ts.g.NW, call.rank);
    }
}

static void planStaged(const acf_hip_ctx* c, const CascState& cs, CascadeCall& call)
{
    const acf_hip_params& p = c->p;
    for (int b : { 16, 32, 128 })
    {
        if (b < p.nTrees)
        {
            call.bounds[call.nStages++] = b;
        }
    }
    call.bounds[call.nStages++] = p.nTrees;
    const int last = call.nStages - 1;
    call.mode = p.treeDepth == 2 ? 2 : (p.treeDepth > 0 ? 1 : 0);
    call.winBytes = sizeof(float) * size_t(call.in.nChns) * (p.modelDsPad_h / cs.cell) * (p.modelDsPad_w / cs.cell);
    call.waveTail = last > 0 && call.bounds[last - 1] >= 128 && call.winBytes <= 64 * 1024;
    call.codeScan = call.waveTail && call.mode == 1 && cs.codes.cap > 0 && call.bounds[last - 1] == 128;
    // Depths 1, 3, 4 with a tile set: trees [0, end) of every window from LDS tiles instead of the staged path's first per-lane
    // gathers from the pyramid, if a stage sD ends at `end`: the survivors enter that stage's queue (or, after the last, are hits)
    const TileSet& ts = call.rank ? cs.tilesR : cs.tiles; // (the rank set is always pooled)
    const int end = ts.g.pooled ? ts.g.b[4] : ts.t1D;     // last tree the tile kernel evaluates
    const int sD = tilesOn(c, cs) ? int(std::find(call.bounds, call.bounds + call.nStages, end) - call.bounds) : call.nStages;
    if (sD == call.nStages)
    {
        call.rank = false; // no tile kernel: every stage reads floats
        return;
    }
    call.ts = &ts;
    call.firstStage = sD + 1;
    const int64_t total = int64_t(ts.nTiles) * call.in.nF;
    if (ts.g.pooled)
    {
        call.pooledTail = sD < last && cs.codes.cap > 0;
        call.tileLds = pooledTileLds(ts.g, call.rank ? 2 : 4, size_t(128) * 4 << p.treeDepth);
        call.grid = tileGrid(c, call.tileLds, total); // (persistent workgroups where option tile_persist says so)
        call.tileD = tile3DKernel(ts.g.NW, p.treeDepth, call.rank);
    }
    else
    {
        call.tileLds = size_t(ts.g.tileFloats) * 4;
        call.grid = { (unsigned int)((total + 7) / 8 * 8), false };
        call.tileD = tileDKernel(ts.g.NW, p.treeDepth);
    }
}

// planPyramid: the cells are the plan's pyramid of the current batch (runCascade's `ranks` != nullptr)
static CascadeCall planCascadeCall(const acf_hip_ctx* c, const CascState& cs, const CascInput& in, bool planPyramid)
{
    CascadeCall call;
    call.in = in;
    call.path = cascadePath(c, cs);
    call.countersCleared = planPyramid && c->countersZeroed;
    call.rank = planPyramid && rankCellsOn(c, cs) && call.path != CascPath::None;
    if (call.path == CascPath::Tiled2)
    {
        planTiled2(c, cs, call);
    }
    else if (call.path == CascPath::Staged)
    {
        planStaged(c, cs, call);
    }
    return call;
}

// acf_hip_get_cascade_forms' record: the call as the launch functions below will read it, word for word (include/acf_hip.h).  It
// decides nothing and no launch reads it.
static std::atomic<uint64_t> g_cascadeFormSeq{ 0 };

static void noteCascadeForms(acf_hip_ctx* c, const CascState& cs, const CascadeCall& call)
{
    int32_t* w = c->cascadeForm;
    std::fill(w, w + ACF_HIP_CF_WORDS, 0);
    w[0] = call.path == CascPath::Tiled2 ? ACF_HIP_CF_PATH_TILED2 : call.path == CascPath::Staged ? ACF_HIP_CF_PATH_STAGED : ACF_HIP_CF_PATH_NONE;
    w[1] = call.rank;
    if (call.ts)
    {
        const TileGeom& g = call.ts->g;
        w[2] = call.tile3 ? ACF_HIP_CF_TILE_3 : g.pooled ? ACF_HIP_CF_TILE_3D : ACF_HIP_CF_TILE_D;
        w[3] = g.NW;
        w[4] = g.TR;
        w[5] = g.TC;
        w[6] = g.passW;
        w[7] = g.pooled;
        std::copy(g.b, g.b + 5, w + 8);
        w[13] = call.ts->nTiles;
        w[14] = int32_t(call.grid.blocks);
        w[15] = call.grid.persist;
        w[16] = int32_t(call.tileLds);
    }
    w[17] = call.nStages;
    std::copy(call.bounds, call.bounds + 4, w + 18);
    w[22] = call.firstStage;
    w[23] = call.mode;
    w[24] = call.codeScan;
    w[25] = call.pooledTail;
    w[26] = call.waveTail;
    w[27] = cs.codes.cap;
    w[28] = cs.qcap;
    w[29] = call.in.nF;
    c->cascadeFormSeq = ++g_cascadeFormSeq;
}

// The counters of the call's path to zero: the hit counts and what QueueCounters lists for the path
static int clearCounters(acf_hip_ctx* c, const CascState& cs, const CascadeCall& call)
{
    const QueueCounters qc = cs.counters();
    HIPCHK(c, hipMemsetAsync(cs.d_counts, 0, sizeof(int32_t) * call.in.nF, c->stream));
    if (call.path == CascPath::Tiled2)
    {
        HIPCHK(c, hipMemsetAsync(qc.d, 0, sizeof(int32_t) * qc.tiled2Count(), c->stream));
    }
    else if (call.path == CascPath::Staged)
    {
        HIPCHK(c, hipMemsetAsync(qc.d, 0, sizeof(int32_t) * qc.stagedCount(call.nStages), c->stream));
        if (call.ts && call.grid.persist)
        {
            HIPCHK(c, hipMemsetAsync(qc.tileNextD(), 0, sizeof(int32_t) * QueueCounters::TILE_COUNTERS, c->stream));
        }
    }
    return ACF_HIP_OK;
}

// The rank cells of this batch, if the call reads them and no level kernel has emitted them: the float pyramid ->
// threshold-rank cells, the one k_rank launch
static int ensureRankCells(acf_hip_ctx* c, const CascState& cs, const CascadeCall& call, bool* ranks)
{
    if (!call.rank || *ranks)
    {
        return ACF_HIP_OK;
    }
    const size_t ldsR = size_t(cs.rankMaxRec) * sizeof(RankRec);
    const auto kRank = cs.rankHasZero ? &k_rank<true> : &k_rank<false>;
    int rc;
    if ((rc = allowLds(c, reinterpret_cast<const void*>(kRank), ldsR)))
    {
        return rc;
    }
    prof(c, c->stream, "k_rank");
    hipLaunchKernelGGL(kRank, dim3(cdiv(cs.rankMaxWP, RANK_CHUNK_COLS), cs.nLevels * call.in.nChns, call.in.nF), dim3(256), ldsR, c->stream, call.in.pyr,
        call.in.pyr_fs, cs.d_pyrR, cs.pyrRCells, (const RankJob*)cs.d_rankJobs, call.in.nChns, (const RankChan*)cs.d_rankChan, (const RankRec*)cs.d_rankRec);
    LAUNCHCHK(c, "k_rank");
    *ranks = true;
    if (call.path == CascPath::Staged)
    {
        prof(c, c->stream, "k_cascade"); // (what follows is the staged cascade's time again)
    }
    return ACF_HIP_OK;
}

extern "C++"
{
// the fields that TileArgs, TileDArgs and CascArgs share (mH, mW: the model window in cells, for the two that walk a window)
template <class Args>
static void fillShared(Args& a, const acf_hip_ctx* c, const CascState& cs, const CascadeCall& call)
{
    a.pyr = call.in.pyr;
    a.pyr_fs = call.in.pyr_fs;
    a.levels = cs.d_cascLevels;
    a.nFrames = call.in.nF;
    a.nChns = call.in.nChns;
    a.cascThr = float(c->p.cascThr); // DetectionParams::cascThr is a float (acfDetect1.cpp:63,323)
    a.qcap = cs.qcap;
    a.hits = cs.d_hits;
    a.counts = cs.d_counts;
    a.maxHits = cs.maxHits;
    if constexpr (!std::is_same<Args, TileDArgs>::value)
    {
        a.mH = c->p.modelDsPad_h / cs.cell;
        a.mW = c->p.modelDsPad_w / cs.cell;
    }
}
}

// a TileArgs' view of one tile set: geometry, tile list and node records
static void setTiles(TileArgs& a, const TileSet& ts)
{
    a.g = ts.g;
    a.tiles = ts.d_tiles;
    a.nTiles = ts.nTiles;
    a.tileNodes = ts.d_tileNodes;
    a.tileNodesS = ts.d_tileNodesS;
    a.aTB = ts.aTB;
}

// Tiled2's arguments on the float tile set: what the scan and k_cascade_tail3 read
static TileArgs tiled2Args(const acf_hip_ctx* c, const CascState& cs, const CascadeCall& call)
{
    const QueueCounters qc = cs.counters();
    TileArgs a{};
    fillShared(a, c, cs, call);
    setTiles(a, cs.tiles);
    a.nTrees = c->p.nTrees;
    a.tailNodes = cs.d_tailNodes;
    a.q = cs.d_queue[0];
    a.qcount = qc.queueCount();
    a.qhead = qc.queueHead();
    a.tileNext = qc.tileNext2();
    a.tailScratch = cs.d_tailScratch;
    a.tailPad = cs.tailPad;
    a.tailSlab = cs.tailSlab;
    a.tailNodesLds = cs.tailNodesLds;
    a.tailCodes = cs.codes.d;
    a.codeCap = cs.codes.cap;
    a.codePitch = cs.codes.pitch;
    return a;
}

// Phase stamps of k_cascade_tile3, in a build with -DACF_HIP_STAMPS only (timing experiments, profiles/ab_*.sh):
// ACF_HIP_CASC_DEBUG -> a.debug and, for bits 4 and 8, the stamp buffer; after the launch the mean cycles per phase of thread 0 of
// every block to stderr
static int stampsBegin(acf_hip_ctx* c, const CascState& cs, int nF, TileArgs& a)
{
#ifdef ACF_HIP_STAMPS
    static const int cascDebug = getenv("ACF_HIP_CASC_DEBUG") ? atoi(getenv("ACF_HIP_CASC_DEBUG")) : 0;
    a.debug = cascDebug;
    if (a.debug & 12)
    {
        a.debug |= 4;
        const int64_t total = int64_t(std::max(cs.tiles.nTiles, cs.tilesR.nTiles)) * nF;
        HIPCHK(c, hipMalloc(&a.stamps, size_t((total + 7) / 8 * 8) * 8 * sizeof(long long)));
        HIPCHK(c, hipMemsetAsync(a.stamps, 0, size_t((total + 7) / 8 * 8) * 8 * sizeof(long long), c->stream));
    }
#endif
    return ACF_HIP_OK;
}

static int stampsReport(acf_hip_ctx* c, const TileArgs& a, unsigned int blocks)
{
#ifdef ACF_HIP_STAMPS
    if (a.debug & 4)
    {
        HIPCHK(c, hipStreamSynchronize(c->stream));
        std::vector<long long> st(size_t(blocks) * 8);
        HIPCHK(c, hipMemcpy(st.data(), a.stamps, st.size() * 8, hipMemcpyDeviceToHost));
        double acc[6] = { 0, 0, 0, 0, 0, 0 }, n1 = 0, n2 = 0, nE = 0, accE = 0;
        long long nb = 0, nbE = 0;
        for (size_t b = 0; b < size_t(blocks); b++)
        {
            if (st[b * 8 + 5] > st[b * 8])
            {
                for (int k = 0; k < 5; k++)
                {
                    acc[k] += double(st[b * 8 + k + 1] - st[b * 8 + k]);
                }
                n1 += double(st[b * 8 + 7] & 0xffff);
                n2 += double((st[b * 8 + 7] >> 16) & 0xffff);
                nE += double(st[b * 8 + 7] >> 32);
                nb++;
                if ((st[b * 8 + 7] >> 32) > 0 && st[b * 8 + 6] > st[b * 8 + 5]) // (tiles with windows in the tail queue: stage E ran)
                {
                    accE += double(st[b * 8 + 6] - st[b * 8 + 5]);
                    nbE++;
                }
            }
        }
        fprintf(stderr, "[casc stamps, pooled] blocks %lld  fill %.0f  A1 (thread 0) %.0f  barrier %.0f  A2 + barrier %.0f  S %.0f cycles;  survivors per tile: A1 %.1f  A2 %.1f  S %.2f;  E %.0f cycles in %.1f %% of the tiles\n",
            nb, acc[0] / nb, acc[1] / nb, acc[2] / nb, acc[3] / nb, acc[4] / nb, n1 / nb, n2 / nb, nE / nb, nbE ? accE / nbE : 0.0, 100.0 * nbE / std::max<long long>(nb, 1));
        (void)hipFree(a.stamps);
    }
#endif
    return ACF_HIP_OK;
}

// Tiled2's tails: the queue entries that k_cascade_tile3 left (a: on the float set; at: the tile kernel's view)
static int launchTiled2Tails(acf_hip_ctx* c, const CascState& cs, const CascadeCall& call, const TileArgs& a, const TileArgs& at)
{
    const int nF = call.in.nF;
    int rc;
    if (call.codeScan)
    {
        // the first codeCap queue entries of every frame carry leaf codes (stage E of the tile kernel): the ordered scan
        const size_t ldsS = size_t(c->p.nTrees - cs.tiles.g.b[4]) * 16;
        prof(c, c->stream, "k_tail_scan");
        if ((rc = launchLds(c, &k_tail_scan, dim3(nF * ((cs.codes.cap + 255) / 256)), dim3(256), ldsS, a)))
        {
            return rc;
        }
        LAUNCHCHK(c, "k_tail_scan");
    }
    if (!call.waveTail)
    {
        return ACF_HIP_OK;
    }
    // queue entries without codes (beyond codeCap): a wave per entry; the blocks leave at once when k_tail_scan has taken the
    // whole queue
    prof(c, c->stream, "k_cascade_tail3");
    if (call.rank)
    {
        hipLaunchKernelGGL(k_cascade_tail_rank, dim3(std::max(1, 1024 / nF) * nF), dim3(64), 0, c->stream, at, (const TreeNode*)cs.d_tailNodesR);
        LAUNCHCHK(c, "k_cascade_tail_rank");
        return ACF_HIP_OK;
    }
    const dim3 grid(std::min(cs.tailBlocks, std::max(1, 512 / nF) * nF)), block(cs.tailWaves * 64);
    const size_t lds = (size_t(cs.tailWaves) * a.tailSlab + size_t(a.tailNodesLds)) * 4;
    if ((rc = launchLds(c, tail3Kernel(cs.tailWaves, a.tailNodesLds != 0), grid, block, lds, a)))
    {
        return rc;
    }
    LAUNCHCHK(c, "k_cascade_tail3");
    return ACF_HIP_OK;
}

// The LDS-tiled cascade of depth 2: k_cascade_tile3, then the tails
static int launchTiled2(acf_hip_ctx* c, const CascState& cs, const CascadeCall& call)
{
    if (!call.ts)
    {
        return ACF_HIP_OK;
    }
    TileArgs a = tiled2Args(c, cs, call);
    int rc;
    if ((rc = stampsBegin(c, cs, call.in.nF, a)))
    {
        return rc;
    }
    TileArgs at = a;
    if (call.rank)
    {
        setTiles(at, *call.ts);
        at.pyrR = cs.d_pyrR;
        at.pyrR_fs = cs.pyrRCells;
    }
    if (!call.grid.persist)
    {
        at.tileNext = nullptr;
    }
    const bool turn = c->opt.cascadeTurns & 1;
    if (turn && (rc = turnBegin(c, 0, 0))) // (before the profile event: the wait for the turn is not the kernel's time)
    {
        return rc;
    }
    prof(c, c->stream, "k_cascade_tile");
    if ((rc = launchLds(c, call.tile3, dim3(call.grid.blocks), dim3(at.g.NW * 64), call.tileLds, at)))
    {
        return rc;
    }
    LAUNCHCHK(c, "k_cascade_tile");
    if ((turn && (rc = turnEnd(c, 0, 0))) || (rc = stampsReport(c, a, call.grid.blocks)))
    {
        return rc;
    }
    return launchTiled2Tails(c, cs, call, a, at);
}

// Staged, depths 1, 3, 4: the tile kernel in front of stage call.firstStage.  k_cascade_tile3D (pooled set) evaluates everything up
// to tree g.b[4] and can write the tail's leaf codes from its stage E; k_cascade_tileD trees [0, t1D).
static int launchTileStageD(acf_hip_ctx* c, const CascState& cs, const CascadeCall& call)
{
    if (!call.ts)
    {
        return ACF_HIP_OK;
    }
    const TileSet& ts = *call.ts;
    const int sD = call.firstStage - 1;
    TileDArgs at{};
    fillShared(at, c, cs, call);
    at.tiles = ts.d_tiles;
    at.nTiles = ts.nTiles;
    at.nBatches = ts.t1D / ts.tbD;
    at.g = ts.g;
    at.nodesD = ts.d_nodesD;
    at.last = sD == call.nStages - 1;
    at.qout = cs.d_queue[sD & 1];
    at.qoutCount = cs.counters().stage(sD);
    if (ts.g.pooled)
    {
        // the model's nodes [tree][nTreeNodes] and leaves; the tail's leaf codes from stage E
        at.tileOff = ts.d_tileOffD;
        at.thrs = call.rank ? reinterpret_cast<const float*>(ts.d_thrsRankD) : cs.d_thrs;
        at.hs = cs.d_hs;
        at.nTrees = c->p.nTrees;
        at.nTreeNodes = c->p.nTreeNodes;
        if (call.rank)
        {
            at.pyrR = cs.d_pyrR;
            at.pyrR_fs = cs.pyrRCells;
        }
        at.codes = call.pooledTail ? cs.codes.d : nullptr;
        at.codeCap = call.pooledTail ? cs.codes.cap : 0;
        at.codePitch = cs.codes.pitch;
        at.tileNext = call.grid.persist ? cs.counters().tileNextD() : nullptr;
        prof(c, c->stream, "k_cascade_tile");
    }
    int rc;
    if ((rc = launchLds(c, call.tileD, dim3(call.grid.blocks), dim3(ts.g.NW * 64), call.tileLds, at)))
    {
        return rc;
    }
    LAUNCHCHK(c, (ts.g.pooled ? "k_cascade_tile3D" : "k_cascade_tileD"));
    if (ts.g.pooled)
    {
        prof(c, c->stream, "k_cascade");
    }
    return ACF_HIP_OK;
}

// Staged, last stage with a wave per surviving window (a: the stage's arguments): enough waves per frame to fill the chip
static int launchStagedTail(acf_hip_ctx* c, const CascState& cs, const CascadeCall& call, CascArgs& a)
{
    const int nF = call.in.nF;
    const dim3 grid(std::max(1, 8192 / nF) * nF);
    if (call.codeScan)
    {
        // leaf codes of the first codes.cap entries, then their ordered sums with lanes = windows; k_cascade_tail (below) takes
        // the entries beyond and leaves at once when there are none
        a.codes = cs.codes.d;
        a.codeCap = cs.codes.cap;
        a.codePitch = cs.codes.pitch;
        if (!call.pooledTail)
        {
            hipLaunchKernelGGL(k_tail_codesD, grid, dim3(64), call.winBytes, c->stream, a);
            LAUNCHCHK(c, "k_tail_codesD");
        }
        const int nT = a.t1 - a.t0, NL = 1 << c->p.treeDepth;
        const size_t ldsS = size_t((nT + 15) / 16 * 16) * NL * sizeof(float);
        int rc;
        if ((rc = launchLds(c, tailScanDKernel(c->p.treeDepth), dim3(nF * ((a.codeCap + 255) / 256)), dim3(256), ldsS, a)))
        {
            return rc;
        }
        LAUNCHCHK(c, "k_tail_scanD");
        a.qskip = a.codeCap;
    }
    hipLaunchKernelGGL(cascadeTailKernel(call.mode), grid, dim3(64), call.winBytes, c->stream, a);
    return ACF_HIP_OK;
}

// Staged: stages [call.firstStage, call.nStages), each from the queue the one before it filled
static int launchStages(acf_hip_ctx* c, const CascState& cs, const CascadeCall& call)
{
    const acf_hip_params& p = c->p;
    const QueueCounters qc = cs.counters();
    const int nF = call.in.nF, bpf = cs.blocksPerFrame, last = call.nStages - 1;
    CascArgs a{};
    fillShared(a, c, cs, call);
    a.blockLevel = cs.d_blockLevel;
    a.blocksPerFrame = bpf;
    a.fids = cs.d_fids;
    a.nTrees = p.nTrees;
    a.nTreeNodes = p.nTreeNodes;
    a.treeDepth = p.treeDepth;
    a.stride = cs.dedupQ > 1 ? cs.cell : p.stride; // (the grid of distinct offsets: its windows are one cell apart)
    a.shrink = cs.cell;
    a.cidAll = cs.d_cidAll;
    a.thrs = cs.d_thrs;
    a.hs = cs.d_hs;
    a.child = cs.d_child;
    a.nodes2 = cs.d_nodes2;
    // later stages see a shrinking survivor set; grid-stride loops cover any count
    const int qGrid[3] = { std::max(1, bpf / 2), std::max(1, bpf / 8), std::max(1, std::min(bpf, 64)) };
    for (int s = call.firstStage; s <= last; s++)
    {
        a.t0 = s == 0 ? 0 : call.bounds[s - 1];
        a.t1 = call.bounds[s];
        a.last = s == last;
        a.qin = s > 0 ? cs.d_queue[(s - 1) & 1] : nullptr;
        a.qinCount = s > 0 ? qc.stage(s - 1) : nullptr;
        a.qout = cs.d_queue[s & 1];
        a.qoutCount = qc.stage(s);
        int rc;
        if (s == 0)
        {
            hipLaunchKernelGGL(cascadeFirstKernel(call.mode), dim3(bpf * nF), dim3(256), 0, c->stream, a);
        }
        else if (s == last && call.waveTail)
        {
            if ((rc = launchStagedTail(c, cs, call, a)))
            {
                return rc;
            }
        }
        else
        {
            hipLaunchKernelGGL(cascadeQueueKernel(call.mode), dim3(qGrid[std::min(s - 1, 2)] * nF), dim3(256), 0, c->stream, a);
        }
        LAUNCHCHK(c, "k_cascade stage");
    }
    return ACF_HIP_OK;
}

// The hits in scale order with their boxes: k_expand_hits where windows share an offset (stride < shrink), k_sort_map
static int sortHits(acf_hip_ctx* c, const CascState& cs, const CascadeCall& call, const BoxLevel* d_box)
{
    const acf_hip_params& p = c->p;
    const int nF = call.in.nF;
    // shift = (modelDsPad - modelDs)/2 - pad (ACF.cpp:275; cv::Size integer arithmetic)
    const int shift_h = (p.modelDsPad_h - p.modelDs_h) / 2 - p.pad_h;
    const int shift_w = (p.modelDsPad_w - p.modelDs_w) / 2 - p.pad_w;
    const acf_hip_hit* hitsForSort = cs.d_hits;
    if (cs.dedupQ > 1)
    {
        if (!cs.d_hitsX || !cs.d_realWin)
        {
            return fail(c, ACF_HIP_E_INVALID, "detect: no buffer for the windows that share an offset (stride < shrink)");
        }
        hipLaunchKernelGGL(k_expand_hits, dim3(nF), dim3(256), 0, c->stream, (const acf_hip_hit*)cs.d_hits, cs.d_counts, cs.d_hitsX, cs.maxHits,
            (const int2*)cs.d_realWin, cs.dedupQ);
        LAUNCHCHK(c, "k_expand_hits");
        hitsForSort = cs.d_hitsX;
    }
    prof(c, c->stream, "k_sort_map");
    hipLaunchKernelGGL(k_sort_map, dim3(SM_BLOCKS, nF), dim3(256), 0, c->stream, hitsForSort, (const int32_t*)cs.d_counts, cs.maxHits,
        d_box, p.stride, shift_h, shift_w, cs.d_sorted, cs.d_dets);
    LAUNCHCHK(c, "k_sort_map");
    return ACF_HIP_OK;
}

static int runCascade(acf_hip_ctx* c, const CascState& cs, const CascInput& in, const BoxLevel* d_box, bool* ranks = nullptr)
{
    const CascadeCall call = planCascadeCall(c, cs, in, ranks != nullptr);
    noteCascadeForms(c, cs, call);
    prof(c, c->stream, "k_cascade");
    int rc;
    if ((!call.countersCleared && (rc = clearCounters(c, cs, call))) || (rc = ensureRankCells(c, cs, call, ranks)))
    {
        return rc;
    }
    if (call.path == CascPath::Tiled2)
    {
        rc = launchTiled2(c, cs, call);
    }
    else if (call.path == CascPath::Staged && !(rc = launchTileStageD(c, cs, call)))
    {
        rc = launchStages(c, cs, call);
    }
    return rc ? rc : sortHits(c, cs, call, d_box);
}

static const size_t kNmsLds = size_t(NMS_CAP) * (8 + 16 + 4 + 1);

static void fillNmsArgs(NmsArgs& a, const acf_hip_nms_params& q)
{
    a.greedy = q.type == 2;
    a.ovrUnion = q.ovrDnmUnion != 0;
    a.doPrune = q.prune != 0;
    a.maxCount = q.maxCount;
    a.overlap = q.overlap;
    a.thr = q.thr;
    a.pruneRatio = q.pruneRatio;
}

// bbNms + prune of every frame's detections of the plan's batch (k_nms, one workgroup per frame)
static int launchNms(acf_hip_ctx* c, int nF)
{
    const CascState& cs = c->cs;
    int rc;
    if (!c->d_nmsKeep)
    {
        if ((rc = devAlloc(c, &c->d_nmsKeep, size_t(cs.batch) * NMS_CAP)) || (rc = devAlloc(c, &c->d_nmsN, size_t(cs.batch))) ||
            (rc = devAlloc(c, &c->d_nmsCounts, size_t(cs.batch))) || (rc = devAlloc(c, &c->d_nmsDets, size_t(cs.batch) * cs.maxHits)))
        {
            return rc;
        }
    }
    NmsArgs a{};
    a.dets = cs.d_dets;
    a.counts = cs.d_counts;
    a.maxHits = cs.maxHits;
    fillNmsArgs(a, c->nms);
    a.keep = c->d_nmsKeep;
    a.nKeep = c->d_nmsN;
    a.outDets = c->d_nmsDets;
    a.outCounts = c->d_nmsCounts;
    if ((rc = allowLds(c, reinterpret_cast<const void*>(&k_nms), kNmsLds)))
    {
        return rc;
    }
    prof(c, c->stream, "k_nms");
    hipLaunchKernelGGL(k_nms, dim3(nF), dim3(1024), kNmsLds, c->stream, a);
    LAUNCHCHK(c, "k_nms");
    return ACF_HIP_OK;
}

// acf_hip_detect runs launchNms after the cascade / the results to read are launchNms's (its buffers exist from its first launch on:
// before that, and after acf_hip_set_nms alone, the cascade's own results are current)
static inline bool nmsRequested(const acf_hip_ctx* c)
{
    return c->nmsOn && c->nms.type != 0;
}

static inline bool nmsActive(const acf_hip_ctx* c)
{
    return nmsRequested(c) && c->d_nmsDets;
}

// LDCF: every level of the batch's pyramid filtered (k 5x5 filters per channel) and halved into the LDCF pyramid, on which the
// cascade then runs with cells of 2*shrink pixels (include/acf_hip.h, acf_hip_params::ldcfK)
static int runLdcf(acf_hip_ctx* c, int nF)
{
    const Plan& pl = c->plan;
    const LdcfStage& L = c->ldcf;
    const ResampleDesc* descs = c->d_descs + L.descBase;
    if (L.tiles > 0)
    {
        // filters + half resample in one kernel: the filtered full-resolution planes stay in LDS
        prof(c, c->stream, "k_ldcf_tile");
        const int xoT = 16;
        const size_t ldsB = ldcfTileLdsFloats(L.tileRows, L.tileCols, xoT) * sizeof(float);
        auto kern = &k_ldcf_tile<8, 4>;
        int rc;
        if ((rc = allowLds(c, reinterpret_cast<const void*>(kern), ldsB)))
        {
            return rc;
        }
        hipLaunchKernelGGL(kern, dim3(L.tiles, pl.nChns, nF), dim3(256), ldsB, c->stream, (const float*)c->d_pyr, L.d_pyr, (const float*)L.d_filt,
            (const LdcfTileJob*)L.d_tileJobs, (const LdcfJob*)L.d_jobs, descs, (const int32_t*)c->d_it, (const float*)c->d_ft, L.tileRows, L.tileCols, xoT,
            c->p.ldcfK, pl.nChns, pl.pyr_floats);
        LAUNCHCHK(c, "k_ldcf_tile");
        return ACF_HIP_OK;
    }
    const int nL = int(pl.levels.size());
    prof(c, c->stream, "k_ldcf_conv");
    hipLaunchKernelGGL(k_ldcf_conv, dim3(cdiv(L.maxCells, 256), pl.nChns * c->p.ldcfK, nF * nL), dim3(256), 0, c->stream, (const float*)c->d_pyr, L.d_tmp,
        (const float*)L.d_filt, (const LdcfJob*)L.d_jobs, nL, pl.nChns, pl.pyr_floats, L.tmpFloats);
    LAUNCHCHK(c, "k_ldcf_conv");
    prof(c, c->stream, "k_resample(ldcf)");
    hipLaunchKernelGGL(k_resample, dim3(L.maxBlocks, nL, nF), dim3(64, 4), 0, c->stream, (const float*)L.d_tmp, L.d_pyr, descs, (const int32_t*)c->d_it,
        (const float*)c->d_ft, RS_XT);
    LAUNCHCHK(c, "k_resample(ldcf)");
    return ACF_HIP_OK;
}
