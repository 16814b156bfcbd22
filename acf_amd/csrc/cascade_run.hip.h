// cascade_run.hip.h — part of acf_hip.hip (included there and nowhere else): acf_hip_detect's launch logic.
//   runCascadeTiled   the LDS-tiled cascade of depth 2 (k_cascade_tile3) + tail (leaf codes + k_tail_scan, or
//                     k_cascade_tail3 / _tail_rank for what does not fit the code buffers)
//   runTileStageD     depths 1, 3, 4: the staged path's first stages from LDS tiles (k_cascade_tile3D / tileD)
//   runCascade        acfDetect1 on every level of a batch (tiled or staged), k_expand_hits for stride < shrink, k_sort_map
//                     (scale-ordered output + box mapping, ACF.cpp:302-329)
//   launchNms         bbNms + prune of the plan's batch on the device
//   runLdcf           the LDCF post-stage: the pyramid filtered and halved into the LDCF pyramid
// The cascade functions run on the CascState they are given (cell size, capacities, buffers): the plan's, or the one
// acf_hip_op_acf_detect1 built for its caller's buffer.  `ranks` != nullptr says that the cells are the plan's pyramid of the
// current batch: rank cells may stand for them, *ranks tells whether they have been written, and acf_hip_run may have cleared
// the counters already.
#pragma once

static int allowLds(acf_hip_ctx* c, const void* kernel, size_t bytes)
{
    if (bytes > 64 * 1024)
    {
        HIPCHK(c, hipFuncSetAttribute(kernel, hipFuncAttributeMaxDynamicSharedMemorySize, int(bytes)));
    }
    return ACF_HIP_OK;
}

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

// The instantiations of the tile kernels by waves per workgroup (NW), tree depth (D, with TB trees per batch) and cell type.
// (Each is named in a statement of its own: the order in which they are first named is their order in the code object.)
using TileKernel = void (*)(TileArgs);
using TileDKernel = void (*)(TileDArgs);

static TileKernel tile3Kernel(int nw, bool rank)
{
#define TILE3_NW(CT)                         \
    switch (nw)                              \
    {                                        \
        case 16: return k_cascade_tile3<16, CT>; \
        case 8: return k_cascade_tile3<8, CT>;   \
        case 4: return k_cascade_tile3<4, CT>;   \
        case 2: return k_cascade_tile3<2, CT>;   \
        default: return k_cascade_tile3<1, CT>;  \
    }
    if (rank)
    {
        TILE3_NW(CellRank)
    }
    TILE3_NW(CellF32)
#undef TILE3_NW
}

static TileKernel tail3Kernel(int waves, bool nodesLds)
{
    switch (waves)
    {
        case 4:
            if (nodesLds)
            {
                return k_cascade_tail3<4, true>;
            }
            return k_cascade_tail3<4, false>;
        case 2:
            if (nodesLds)
            {
                return k_cascade_tail3<2, true>;
            }
            return k_cascade_tail3<2, false>;
        default:
            if (nodesLds)
            {
                return k_cascade_tail3<1, true>;
            }
            return k_cascade_tail3<1, false>;
    }
}

static TileDKernel tile3DKernel(int nw, int depth, bool rank)
{
#define TILE3D_DEPTH(N)                                                                                      \
    switch (depth)                                                                                           \
    {                                                                                                        \
        case 1: if (rank) return k_cascade_tile3D<N, 1, 4, CellRank>; return k_cascade_tile3D<N, 1, 4, CellF32>; \
        case 3: if (rank) return k_cascade_tile3D<N, 3, 2, CellRank>; return k_cascade_tile3D<N, 3, 2, CellF32>; \
        default: if (rank) return k_cascade_tile3D<N, 4, 1, CellRank>; return k_cascade_tile3D<N, 4, 1, CellF32>; \
    }
    if (nw == 8)
    {
        TILE3D_DEPTH(8)
    }
    TILE3D_DEPTH(4)
#undef TILE3D_DEPTH
}

static TileDKernel tileDKernel(int nw, int depth)
{
#define TILED_DEPTH(N)                                  \
    switch (depth)                                      \
    {                                                   \
        case 1: return k_cascade_tileD<N, 1, 4>;        \
        case 3: return k_cascade_tileD<N, 3, 2>;        \
        default: return k_cascade_tileD<N, 4, 1>;       \
    }
    if (nw == 8)
    {
        TILED_DEPTH(8)
    }
    TILED_DEPTH(4)
#undef TILED_DEPTH
}

// depth 2 with a float tile set and option cascade_tiles: runCascadeTiled takes the whole cascade (runCascade's branch and
// acf_hip_run's early counter clear both ask this)
static inline bool wholeCascadeTiled(const acf_hip_ctx* c, const CascState& cs)
{
    return cs.tiles.ok && c->p.treeDepth == 2 && c->opt.cascadeTiles;
}

// the float pyramid -> threshold-rank cells (levels whose kernels did not emit them): the one k_rank launch
static int launchRankCells(acf_hip_ctx* c, const CascState& cs, const float* pyr, int64_t pyr_fs, int nF, int nChns)
{
    const size_t ldsR = size_t(cs.rankMaxRec) * sizeof(RankRec);
    int rc;
    if ((rc = allowLds(c, reinterpret_cast<const void*>(&k_rank), ldsR)))
    {
        return rc;
    }
    prof(c, "k_rank");
    hipLaunchKernelGGL(k_rank, dim3(cdiv(cs.rankMaxWP, RANK_CHUNK_COLS), cs.nLevels * nChns, nF), dim3(256), ldsR, c->stream, pyr, pyr_fs,
        cs.d_pyrR, cs.pyrRCells, (const RankJob*)cs.d_rankJobs, nChns, (const RankChan*)cs.d_rankChan, (const RankRec*)cs.d_rankRec);
    LAUNCHCHK(c, "k_rank");
    return ACF_HIP_OK;
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

static int runCascadeTiled(acf_hip_ctx* c, const CascState& cs, const float* pyr, int64_t pyr_fs, int nF, int nChns, bool* ranks)
{
    const acf_hip_params& p = c->p;
    const TileGeom& g = cs.tiles.g;
    if (!(ranks && c->countersZeroed))
    {
        HIPCHK(c, hipMemsetAsync(cs.d_qcounts, 0, sizeof(int32_t) * (2 * size_t(cs.batch) + 8), c->stream));
    }
    TileArgs a{};
    setTiles(a, cs.tiles);
    a.pyr = pyr;
    a.pyr_fs = pyr_fs;
    a.levels = cs.d_cascLevels;
    a.nFrames = nF;
    a.nChns = nChns;
    a.mH = p.modelDsPad_h / cs.cell;
    a.mW = p.modelDsPad_w / cs.cell;
    a.nTrees = p.nTrees;
    a.tailNodes = cs.d_tailNodes;
    a.cascThr = float(p.cascThr); // DetectionParams::cascThr is a float (acfDetect1.cpp:63,323)
    a.q = cs.d_queue[0];
    a.qcount = cs.d_qcounts;
    a.qhead = cs.d_qcounts + cs.batch;
    a.tileNext = cs.d_qcounts + 2 * size_t(cs.batch);
    a.qcap = cs.qcap;
    a.hits = cs.d_hits;
    a.counts = cs.d_counts;
    a.maxHits = cs.maxHits;
    a.tailScratch = cs.d_tailScratch;
    a.tailPad = cs.tailPad;
    a.tailSlab = cs.tailSlab;
    a.tailNodesLds = cs.tailNodesLds;
    a.tailCodes = cs.codes.d;
    a.codeCap = cs.codes.cap;
    a.codePitch = cs.codes.pitch;
    a.debug = 0;
#ifdef ACF_HIP_STAMPS
    static const int cascDebug = getenv("ACF_HIP_CASC_DEBUG") ? atoi(getenv("ACF_HIP_CASC_DEBUG")) : 0; // timing experiments (profiles/ab_*.sh)
    a.debug = cascDebug;
#endif
    if (a.debug & 12)
    {
        a.debug |= 4;
        const int64_t total = int64_t(std::max(cs.tiles.nTiles, cs.tilesR.nTiles)) * nF;
        HIPCHK(c, hipMalloc(&a.stamps, size_t((total + 7) / 8 * 8) * 8 * sizeof(long long)));
        HIPCHK(c, hipMemsetAsync(a.stamps, 0, size_t((total + 7) / 8 * 8) * 8 * sizeof(long long), c->stream));
    }
    const bool rank = ranks && rankCellsOn(c, cs);
    int rc = 0;
    if (rank && !*ranks)
    {
        if ((rc = launchRankCells(c, cs, pyr, pyr_fs, nF, nChns)))
        {
            return rc;
        }
        *ranks = true;
    }
    if (cs.tiles.nTiles > 0)
    {
        TileArgs at = a; // the tile kernel's view: the rank form has its own tile geometry, tile list and node records
        if (rank)
        {
            setTiles(at, cs.tilesR);
            at.pyrR = cs.d_pyrR;
            at.pyrR_fs = cs.pyrRCells;
        }
        const TileGeom& gt = at.g;
        const size_t lds = pooledTileLds(gt, rank ? 2 : 4, TILE3_LEAF_BYTES);
        const TileGrid tg = tileGrid(c, lds, int64_t(at.nTiles) * nF);
        if (!tg.persist)
        {
            at.tileNext = nullptr;
        }
        dim3 grid(tg.blocks), block(gt.NW * 64);
        if ((c->opt.cascadeTurns & 1) && (rc = turnBegin(c, 0, 0))) // (before the profile event: the wait for the turn is not the kernel's time)
        {
            return rc;
        }
        prof(c, "k_cascade_tile");
        if ((rc = launchLds(c, tile3Kernel(gt.NW, rank), grid, block, lds, at)))
        {
            return rc;
        }
        LAUNCHCHK(c, "k_cascade_tile");
        if ((c->opt.cascadeTurns & 1) && (rc = turnEnd(c, 0, 0)))
        {
            return rc;
        }
#ifdef ACF_HIP_STAMPS
        if (a.debug & 4)
        {
            // debug only: mean cycles per phase of thread 0 of every block
            HIPCHK(c, hipStreamSynchronize(c->stream));
            std::vector<long long> st(size_t(grid.x) * 8);
            HIPCHK(c, hipMemcpy(st.data(), a.stamps, st.size() * 8, hipMemcpyDeviceToHost));
            double acc[6] = { 0, 0, 0, 0, 0, 0 }, n1 = 0, n2 = 0, nE = 0, accE = 0;
            long long nb = 0, nbE = 0;
            for (size_t b = 0; b < size_t(grid.x); b++)
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
        if (g.b[4] < p.nTrees && cs.codes.cap > 0)
        {
            // the first codeCap queue entries of every frame carry leaf codes (stage E of the tile kernel): the ordered scan
            const size_t ldsS = size_t(p.nTrees - g.b[4]) * 16;
            if ((rc = allowLds(c, reinterpret_cast<const void*>(&k_tail_scan), ldsS)))
            {
                return rc;
            }
            prof(c, "k_tail_scan");
            hipLaunchKernelGGL(k_tail_scan, dim3(nF * ((cs.codes.cap + 255) / 256)), dim3(256), ldsS, c->stream, a);
            LAUNCHCHK(c, "k_tail_scan");
        }
        if (g.b[4] < p.nTrees && rank)
        {
            // queue entries without codes (beyond codeCap) from the rank cells: a wave per entry; its blocks leave at once
            // when k_tail_scan has taken the whole queue
            prof(c, "k_cascade_tail3");
            hipLaunchKernelGGL(k_cascade_tail_rank, dim3(std::max(1, 1024 / nF) * nF), dim3(64), 0, c->stream, at, (const TreeNode*)cs.d_tailNodesR);
            LAUNCHCHK(c, "k_cascade_tail_rank");
        }
        else if (g.b[4] < p.nTrees)
        {
            // queue entries without codes (beyond codeCap, or ACF_HIP_TAIL3): k_cascade_tail3; its blocks leave at once when
            // k_tail_scan has taken the whole queue
            dim3 tgrid(std::min(cs.tailBlocks, std::max(1, 512 / nF) * nF)), tblock(cs.tailWaves * 64);
            const size_t tl = (size_t(cs.tailWaves) * a.tailSlab + size_t(a.tailNodesLds)) * 4;
            prof(c, "k_cascade_tail3");
            if ((rc = launchLds(c, tail3Kernel(cs.tailWaves, a.tailNodesLds != 0), tgrid, tblock, tl, a)))
            {
                return rc;
            }
            LAUNCHCHK(c, "k_cascade_tail3");
        }
    }
    return ACF_HIP_OK;
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
    prof(c, "k_nms");
    hipLaunchKernelGGL(k_nms, dim3(nF), dim3(1024), kNmsLds, c->stream, a);
    LAUNCHCHK(c, "k_nms");
    return ACF_HIP_OK;
}

static inline bool nmsActive(const acf_hip_ctx* c)
{
    return c->nmsOn && c->nms.type != 0 && c->d_nmsDets;
}

// Depths 1, 3, 4: trees [0, end) of every window from LDS tiles (k_cascade_tile3D on a pooled set: everything up to tree g.b[4],
// the tail's leaf codes from its stage E; k_cascade_tileD: trees [0, t1D)) instead of the staged path's first per-lane gathers
// from the pyramid.  Its survivors enter the queue of the stage that ends at `end`.  firstStage: the first stage the staged path
// still runs (0 when no stage ends there: the tile kernel does not run); pooledTail: the tile kernel has written the tail's leaf codes.
static int runTileStageD(acf_hip_ctx* c, const CascState& cs, const float* pyr, int64_t pyr_fs, int nF, int nChns, bool* ranks, const std::vector<int>& bounds,
    int& firstStage, bool& pooledTail)
{
    const acf_hip_params& p = c->p;
    const bool rank = ranks && rankCellsOn(c, cs);
    const TileSet& ts = rank ? cs.tilesR : cs.tiles; // (the rank set is always pooled)
    const int end = ts.g.pooled ? ts.g.b[4] : ts.t1D; // last tree the tile kernel evaluates
    const int nStages = int(bounds.size());
    int sD = -1;
    for (int i = 0; i < nStages; i++)
    {
        if (bounds[size_t(i)] == end)
        {
            sD = i;
        }
    }
    if (sD < 0)
    {
        return ACF_HIP_OK;
    }
    TileDArgs at{};
    at.pyr = pyr;
    at.pyr_fs = pyr_fs;
    at.levels = cs.d_cascLevels;
    at.tiles = ts.d_tiles;
    at.nTiles = ts.nTiles;
    at.nFrames = nF;
    at.nChns = nChns;
    at.nBatches = ts.t1D / ts.tbD;
    at.g = ts.g;
    at.nodesD = ts.d_nodesD;
    at.cascThr = float(p.cascThr);
    at.last = sD == nStages - 1;
    at.qout = cs.d_queue[sD & 1];
    at.qoutCount = cs.d_qcounts + size_t(sD) * cs.batch;
    at.qcap = cs.qcap;
    at.hits = cs.d_hits;
    at.counts = cs.d_counts;
    at.maxHits = cs.maxHits;
    const int64_t total = int64_t(ts.nTiles) * nF;
    int rc = 0;
    if (rank && !*ranks)
    {
        if ((rc = launchRankCells(c, cs, pyr, pyr_fs, nF, nChns)))
        {
            return rc;
        }
        *ranks = true;
        prof(c, "k_cascade");
    }
    // k_cascade_tile3D on a pooled set (persistent workgroups where option tile_persist says so), else k_cascade_tileD
    size_t lds = size_t(ts.g.tileFloats) * 4;
    TileGrid tg = { (unsigned int)((total + 7) / 8 * 8), false };
    TileDKernel kernel = tileDKernel(ts.g.NW, p.treeDepth);
    if (ts.g.pooled)
    {
        // the model's nodes [tree][nTreeNodes] and leaves; the tail's leaf codes from stage E
        at.tileOff = ts.d_tileOffD;
        at.thrs = rank ? reinterpret_cast<const float*>(ts.d_thrsRankD) : cs.d_thrs;
        at.hs = cs.d_hs;
        at.nTrees = p.nTrees;
        at.nTreeNodes = p.nTreeNodes;
        if (rank)
        {
            at.pyrR = cs.d_pyrR;
            at.pyrR_fs = cs.pyrRCells;
        }
        pooledTail = !at.last && cs.codes.cap > 0;
        at.codes = pooledTail ? cs.codes.d : nullptr;
        at.codeCap = pooledTail ? cs.codes.cap : 0;
        at.codePitch = cs.codes.pitch;
        lds = pooledTileLds(ts.g, rank ? 2 : 4, size_t(128) * 4 << p.treeDepth);
        tg = tileGrid(c, lds, total);
        // (the staged path's counters [stage][frame] start at d_qcounts; the tile counters sit behind them)
        at.tileNext = tg.persist ? cs.d_qcounts + size_t(8) * cs.batch : nullptr;
        if (tg.persist)
        {
            HIPCHK(c, hipMemsetAsync(at.tileNext, 0, sizeof(int32_t) * 8, c->stream));
        }
        kernel = tile3DKernel(ts.g.NW, p.treeDepth, rank);
        prof(c, "k_cascade_tile");
    }
    if ((rc = launchLds(c, kernel, dim3(tg.blocks), dim3(ts.g.NW * 64), lds, at)))
    {
        return rc;
    }
    LAUNCHCHK(c, (ts.g.pooled ? "k_cascade_tile3D" : "k_cascade_tileD"));
    if (ts.g.pooled)
    {
        prof(c, "k_cascade");
    }
    firstStage = sD + 1;
    return ACF_HIP_OK;
}

static int runCascade(acf_hip_ctx* c, const CascState& cs, const float* pyr, int64_t pyr_fs, const BoxLevel* d_box, int nF, int nChns, bool* ranks = nullptr)
{
    const acf_hip_params& p = c->p;
    const int blocksPerFrame = cs.blocksPerFrame;
    prof(c, "k_cascade");
    if (!(ranks && c->countersZeroed))
    {
        HIPCHK(c, hipMemsetAsync(cs.d_counts, 0, sizeof(int32_t) * nF, c->stream));
    }
    int rc = 0;
    if (wholeCascadeTiled(c, cs))
    {
        if ((rc = runCascadeTiled(c, cs, pyr, pyr_fs, nF, nChns, ranks)))
        {
            return rc;
        }
    }
    else if (blocksPerFrame > 0)
    {
        // stage boundaries (see kernels.hip.h): [0,16) [16,32) [32,128) [128,nTrees)
        std::vector<int> bounds;
        for (int b : { 16, 32, 128 })
        {
            if (b < p.nTrees)
            {
                bounds.push_back(b);
            }
        }
        bounds.push_back(p.nTrees);
        const int nStages = int(bounds.size());
        HIPCHK(c, hipMemsetAsync(cs.d_qcounts, 0, sizeof(int32_t) * size_t(nStages) * cs.batch, c->stream));
        CascArgs a{};
        a.pyr = pyr;
        a.pyr_fs = pyr_fs;
        a.levels = cs.d_cascLevels;
        a.blockLevel = cs.d_blockLevel;
        a.blocksPerFrame = blocksPerFrame;
        a.nFrames = nF;
        a.mH = p.modelDsPad_h / cs.cell;
        a.mW = p.modelDsPad_w / cs.cell;
        a.nChns = nChns;
        a.fids = cs.d_fids;
        a.nTrees = p.nTrees;
        a.nTreeNodes = p.nTreeNodes;
        a.treeDepth = p.treeDepth;
        a.stride = cs.dedupQ > 1 ? cs.cell : p.stride; // (the grid of distinct offsets: its windows are one cell apart)
        a.shrink = cs.cell;
        a.cascThr = float(p.cascThr); // DetectionParams::cascThr is a float (acfDetect1.cpp:63,323)
        a.cidAll = cs.d_cidAll;
        a.thrs = cs.d_thrs;
        a.hs = cs.d_hs;
        a.child = cs.d_child;
        a.nodes2 = cs.d_nodes2;
        a.qcap = cs.qcap;
        a.hits = cs.d_hits;
        a.counts = cs.d_counts;
        a.maxHits = cs.maxHits;
        const int mode = p.treeDepth == 2 ? 2 : (p.treeDepth > 0 ? 1 : 0);
        // later stages see a shrinking survivor set; grid-stride loops cover any count
        const int qGrid[3] = { std::max(1, blocksPerFrame / 2), std::max(1, blocksPerFrame / 8), std::max(1, std::min(blocksPerFrame, 64)) };
        int firstStage = 0;
        bool pooledTail = false; // k_cascade_tile3D has written the tail's leaf codes: no k_tail_codesD
        if (cs.tiles.ok && p.treeDepth != 2 && c->opt.cascadeTiles && (rc = runTileStageD(c, cs, pyr, pyr_fs, nF, nChns, ranks, bounds, firstStage, pooledTail)))
        {
            return rc;
        }
        for (int sidx = firstStage; sidx < nStages; sidx++)
        {
            a.t0 = sidx == 0 ? 0 : bounds[sidx - 1];
            a.t1 = bounds[sidx];
            a.last = sidx == nStages - 1;
            a.qin = sidx > 0 ? cs.d_queue[(sidx - 1) & 1] : nullptr;
            a.qinCount = sidx > 0 ? cs.d_qcounts + size_t(sidx - 1) * cs.batch : nullptr;
            a.qout = cs.d_queue[sidx & 1];
            a.qoutCount = cs.d_qcounts + size_t(sidx) * cs.batch;
            dim3 block(256);
            const size_t winBytes = sizeof(float) * size_t(nChns) * a.mH * a.mW;
            const bool tail = a.last && sidx > 0 && a.t0 >= 128 && winBytes <= 64 * 1024;
            if (sidx == 0)
            {
                dim3 grid(blocksPerFrame * nF);
                if (mode == 2)
                {
                    hipLaunchKernelGGL(k_cascade_first<2>, grid, block, 0, c->stream, a);
                }
                else if (mode == 1)
                {
                    hipLaunchKernelGGL(k_cascade_first<1>, grid, block, 0, c->stream, a);
                }
                else
                {
                    hipLaunchKernelGGL(k_cascade_first<0>, grid, block, 0, c->stream, a);
                }
            }
            else if (tail)
            {
                // one wave per surviving window; enough waves per frame to fill the chip
                dim3 grid(std::max(1, 8192 / nF) * nF);
                if (mode == 1 && cs.codes.cap > 0 && a.t0 == 128)
                {
                    // leaf codes of the first codes.cap entries, then their ordered sums with lanes = windows; k_cascade_tail
                    // (below) takes the entries beyond and leaves at once when there are none
                    a.codes = cs.codes.d;
                    a.codeCap = cs.codes.cap;
                    a.codePitch = cs.codes.pitch;
                    if (!pooledTail)
                    {
                        hipLaunchKernelGGL(k_tail_codesD, grid, dim3(64), winBytes, c->stream, a);
                        LAUNCHCHK(c, "k_tail_codesD");
                    }
                    const int nT = a.t1 - a.t0, NL = 1 << p.treeDepth;
                    const size_t ldsS = size_t((nT + 15) / 16 * 16) * NL * sizeof(float);
                    dim3 gridS(nF * ((a.codeCap + 255) / 256));
                    void (*scan)(CascArgs) = nullptr;
                    switch (p.treeDepth)
                    {
                        case 1: scan = k_tail_scanD<1>; break;
                        case 3: scan = k_tail_scanD<3>; break;
                        case 4: scan = k_tail_scanD<4>; break;
                        default: scan = k_tail_scanD<2>; break;
                    }
                    if ((rc = launchLds(c, scan, gridS, dim3(256), ldsS, a)))
                    {
                        return rc;
                    }
                    LAUNCHCHK(c, "k_tail_scanD");
                    a.qskip = a.codeCap;
                }
                if (mode == 2)
                {
                    hipLaunchKernelGGL(k_cascade_tail<2>, grid, dim3(64), winBytes, c->stream, a);
                }
                else if (mode == 1)
                {
                    hipLaunchKernelGGL(k_cascade_tail<1>, grid, dim3(64), winBytes, c->stream, a);
                }
                else
                {
                    hipLaunchKernelGGL(k_cascade_tail<0>, grid, dim3(64), winBytes, c->stream, a);
                }
            }
            else
            {
                dim3 grid(qGrid[std::min(sidx - 1, 2)] * nF);
                if (mode == 2)
                {
                    hipLaunchKernelGGL(k_cascade_queue<2>, grid, block, 0, c->stream, a);
                }
                else if (mode == 1)
                {
                    hipLaunchKernelGGL(k_cascade_queue<1>, grid, block, 0, c->stream, a);
                }
                else
                {
                    hipLaunchKernelGGL(k_cascade_queue<0>, grid, block, 0, c->stream, a);
                }
            }
            LAUNCHCHK(c, "k_cascade stage");
        }
    }
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
    prof(c, "k_sort_map");
    hipLaunchKernelGGL(k_sort_map, dim3(SM_BLOCKS, nF), dim3(256), 0, c->stream, hitsForSort, (const int32_t*)cs.d_counts, cs.maxHits,
        d_box, p.stride, shift_h, shift_w, cs.d_sorted, cs.d_dets);
    LAUNCHCHK(c, "k_sort_map");
    return ACF_HIP_OK;
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
        prof(c, "k_ldcf_tile");
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
    prof(c, "k_ldcf_conv");
    hipLaunchKernelGGL(k_ldcf_conv, dim3(cdiv(L.maxCells, 256), pl.nChns * c->p.ldcfK, nF * nL), dim3(256), 0, c->stream, (const float*)c->d_pyr, L.d_tmp,
        (const float*)L.d_filt, (const LdcfJob*)L.d_jobs, nL, pl.nChns, pl.pyr_floats, L.tmpFloats);
    LAUNCHCHK(c, "k_ldcf_conv");
    prof(c, "k_resample(ldcf)");
    hipLaunchKernelGGL(k_resample, dim3(L.maxBlocks, nL, nF), dim3(64, 4), 0, c->stream, (const float*)L.d_tmp, L.d_pyr, descs, (const int32_t*)c->d_it,
        (const float*)c->d_ft, RS_XT);
    LAUNCHCHK(c, "k_resample(ldcf)");
    return ACF_HIP_OK;
}
