// plan_build.hip.h — part of acf_hip.hip (included there and nowhere else): acf_hip_plan's work, one function per stage of the path the
// plan serves.  Everything a run needs — buffers for max_batch frames, resampling tables, job lists, cascade tables — is built here
// once; nothing is allocated on the hot path.  PlanBuild holds what the stages share (the table arena, the job lists that are
// uploaded together at the end).
//
//   subBatchContexts()   option "streams" > 1: the plan's geometry stays here, every device buffer lives in a child context
//   colourBuffer()       rgbConvert's output (chnsPyramid.cpp:230-263)
//   realScales()         the real scales' images, smoothed planes, M / O / U / S (chnsPyramid.cpp:297-338)
//   imageStrips()        k_resample_strip's plans for the down-sampling image resamples
//   approxLevels()       resampling descriptors of the approximated levels (chnsPyramid.cpp:385-397)
//   finalJobs()          final smoothing + padding jobs, the rank pyramid's layout (chnsPyramid.cpp:399-435)
//   levelJobs()          the fused level kernels' job lists
//   ldcf()               the LDCF post-stage's levels, tiles and buffers (acf_hip_params::ldcfK)
//   uploadAndScratch()   tables to the device; raw channels, pyramid, the segment kernels' hand-over states
//   cascade()            cascade tables, box mapping, hit / queue buffers
#pragma once

namespace
{
struct PlanBuild
{
    acf_hip_ctx* const c;
    const acf_hip_params& p;
    Plan& pl;
    const int H, W, d_in, B, max_hits, shrink, d;
    const int64_t np0;
    TableArena arena;
    std::vector<SmoothJob> realJobs, finalJobList;
    std::vector<int64_t> rankOffs;
    std::vector<PadJob> padJobs, padJobsR;
    int py = 0, px = 0; // padding in cells

    PlanBuild(acf_hip_ctx* ctx, int H_, int W_, int d_in_, int max_batch, int max_hits_)
        : c(ctx), p(ctx->p), pl(ctx->plan), H(H_), W(W_), d_in(d_in_), B(max_batch), max_hits(max_hits_), shrink(ctx->p.shrink), d(ctx->plan.d), np0(int64_t(H_) * W_)
    {
    }
    int colourBuffer();
    int realScales();
    int imageStrips();
    int approxLevels();
    int finalJobs();
    int levelJobs();
    int ldcf();
    int uploadAndScratch();
    int cascade();
};

int PlanBuild::colourBuffer()
{
    int rc = ACF_HIP_OK;
    (void)rc;
    // colour conversion buffer (chnsPyramid.cpp:230-263)
    if (!colourPassthrough(p, d_in))
    {
        if ((rc = devAlloc(c, &c->d_color, size_t(B) * d * np0)))
        {
            return rc;
        }
    }

    return ACF_HIP_OK;
}

int PlanBuild::realScales()
{
    int rc = ACF_HIP_OK;
    (void)rc;
    // real scales: mirror the reference's shallow-copy bookkeeping (chnsPyramid.cpp:297-338)
    int curH = H, curW = W;
    for (size_t k = 0; k < pl.real.size(); k++)
    {
        RealScale rs;
        rs.level = pl.real[k];
        rs.h = pl.real_h[k];
        rs.w = pl.real_w[k];
        const double s = pl.levels[rs.level].scale;
        const bool same = (H == rs.h && W == rs.w); // sz == sz1 (:303), compared against the ORIGINAL size
        if (same && (curH != H || curW != W))
        {
            return fail(c, ACF_HIP_E_UNSUPPORTED, "plan: scale order");
        }
        rs.resampled = !same;
        rs.src_h = curH;
        rs.src_w = curW;
        const int64_t np = int64_t(rs.h) * rs.w;
        if (rs.resampled)
        {
            ResampleDesc dd;
            if ((rc = buildResample(curH, curW, rs.h, rs.w, dd, arena)))
            {
                return fail(c, rc, "plan: degenerate resample geometry");
            }
            const double one[3] = { 1.0, 1.0, 1.0 };
            setResampleGain(dd, one, d, d);
            dd.nplanes = d;
            dd.src_off = 0;
            dd.dst_off = 0;
            dd.src_frame_stride = int64_t(d) * curH * curW;
            dd.dst_frame_stride = int64_t(d) * np;
            rs.descIndex = int(c->h_descs.size());
            c->h_descs.push_back(dd);
            if ((rc = devAlloc(c, &rs.img, size_t(B) * d * np)))
            {
                return rc;
            }
        }
        const bool halfCond = (s == 0.5) && ((p.nApprox > 0) || (p.nPerOct == 1)); // :313-316
        rs.adoptAsI = same || halfCond;
        if (rs.adoptAsI)
        {
            curH = rs.h;
            curW = rs.w;
        }
        if ((rc = devAlloc(c, &rs.sm, size_t(B) * d * np)))
        {
            return rc;
        }
        if (p.gradMagEnabled || p.gradHistEnabled)
        {
            rs.moFloats = std::max<int64_t>(np, moBlockedFloats(rs.h, rs.w));
            if ((rc = devAlloc(c, &rs.M, size_t(B) * size_t(rs.moFloats))) || (rc = devAlloc(c, &rs.O, size_t(B) * size_t(rs.moFloats))))
            {
                return rc;
            }
            if (p.normRad)
            {
                // U: a plane (with room for the blocks' padding) — or, where convTri's x pass can leave checkpoints instead (triPlan's
                // ck; its shape conditions are stated here, the rest is decided per call), an eighth of one and NO plane: U is then
                // allocated by the first call that takes a form which reads it (PyramidRun::realScale -> allocU)
                rs.uFloats = std::max<int64_t>(np, uBlockedFloats(rs.h, rs.w));
                const bool ckShape = p.normRad == 5 && p.shrink == 4 && rs.h % 4 == 0 && rs.w % 4 == 0 && rs.h >= 48 && rs.w >= 48 &&
                    !c->opt.taps && !fallbackForced(FB_TRIY_STORED_U);
                if (ckShape)
                {
                    rs.ckFloats = triCkFloats(rs.h, rs.w);
                    if ((rc = devAlloc(c, &rs.Ck, size_t(B) * size_t(rs.ckFloats))))
                    {
                        return rc;
                    }
                }
                else if ((rc = allocU(c, rs, B)))
                {
                    return rc;
                }
                if ((rc = devAlloc(c, &rs.S, size_t(B) * np)))
                {
                    return rc;
                }
            }
            if (c->opt.taps)
            {
                if ((rc = devAlloc(c, &rs.Mn, size_t(B) * np)))
                {
                    return rc;
                }
            }
        }
        SmoothJob j{};
        j.h = rs.h;
        j.w = rs.w;
        j.nplanes = d;
        j.out_cs = rs.h;
        j.in_off = 0;
        j.out_off = 0;
        j.in_ps = np;
        j.out_ps = np;
        realJobs.push_back(j);
        c->real.push_back(rs);
    }
    return ACF_HIP_OK;
}

int PlanBuild::imageStrips()
{
    int rc = ACF_HIP_OK;
    (void)rc;
    c->nImgDescs = int(c->h_descs.size());
    // k_resample_strip (the march over strips of output columns) for every down-sampling image resample, and for two consecutive
    // real scales that share their source — the two small scales of a 1080p pyramid — in one pass (A/B: ACF_HIP_RESAMPLE_NO_STRIP)
    if (!fallbackForced(FB_RESAMPLE_NO_STRIP))
    {
        for (size_t k = 0; k < c->real.size(); k++)
        {
            RealScale& ra = c->real[k];
            if (!ra.resampled)
            {
                continue;
            }
            ra.strip = stripPlan(c->h_descs[ra.descIndex], nullptr, arena);
            if (k + 1 < c->real.size() && !fallbackForced(FB_RESAMPLE_NO_PAIR))
            {
                const RealScale& rb = c->real[k + 1];
                if (rb.resampled && !ra.adoptAsI && ra.src_h == rb.src_h && ra.src_w == rb.src_w && !(k > 0 && c->real[k - 1].stripPair.ok) && rb.w <= ra.w && rb.h <= ra.h)
                {
                    ra.stripPair = stripPlan(c->h_descs[ra.descIndex], &c->h_descs[rb.descIndex], arena);
                }
            }
        }
    }

    return ACF_HIP_OK;
}

int PlanBuild::approxLevels()
{
    int rc = ACF_HIP_OK;
    (void)rc;
    // approximated levels (chnsPyramid.cpp:385-397)
    const int nColor = p.colorEnabled ? d : 0;
    const int nMag = p.gradMagEnabled ? 1 : 0;
    for (size_t i = 0; i < pl.levels.size(); i++)
    {
        const acf_hip_level& l = pl.levels[i];
        if (l.isReal)
        {
            continue;
        }
        const acf_hip_level& lr = pl.levels[l.realIndex];
        ResampleDesc dd;
        if ((rc = buildResample(lr.hC, lr.wC, l.hC, l.wC, dd, arena)))
        {
            return fail(c, rc, "plan: degenerate resample geometry (approximated level)");
        }
        double ratio[3];
        for (int j = 0; j < 3; j++)
        {
            ratio[j] = std::pow(l.scale / lr.scale, -(p.nLambdas == 3 ? p.lambdas[j] : 0.0)); // :393 (image-specific lambdas: rewritten per frame)
        }
        setResampleGain(dd, ratio, nColor, nColor + nMag);
        dd.nplanes = pl.nChns;
        dd.src_off = pl.raw_off[l.realIndex];
        dd.dst_off = pl.raw_off[i];
        dd.src_frame_stride = pl.raw_floats;
        dd.dst_frame_stride = pl.raw_floats;
        c->h_descs.push_back(dd);
        c->approxMaxBlocks = std::max(c->approxMaxBlocks, resampleBlocks(dd));
    }
    c->nApproxDescs = int(c->h_descs.size()) - c->nImgDescs;
    c->autoLambdas = p.nApprox > 0 && p.nLambdas != 3;
    c->h_lambdas.assign(size_t(B) * 3, 0.0);
    if (c->autoLambdas && (rc = devAlloc(c, &c->d_planeSums, size_t(B) * 2 * pl.nChns)))
    {
        return rc;
    }

    return ACF_HIP_OK;
}

int PlanBuild::finalJobs()
{
    int rc = ACF_HIP_OK;
    (void)rc;
    // final smoothing + padding jobs (chnsPyramid.cpp:399-435)
    int64_t rankOff = 0; // the rank pyramid's layout (rankPitch): levels in order, nChns planes [wP][pitch] each
    py = p.pad_h / shrink;
    px = p.pad_w / shrink;
    for (size_t i = 0; i < pl.levels.size(); i++)
    {
        const acf_hip_level& l = pl.levels[i];
        SmoothJob j{};
        j.h = l.hC;
        j.w = l.wC;
        j.nplanes = pl.nChns;
        j.out_cs = l.hP;
        j.in_off = pl.raw_off[i];
        j.out_off = l.offset + int64_t(px) * l.hP + py;
        j.in_ps = int64_t(l.hC) * l.wC;
        j.out_ps = int64_t(l.hP) * l.wP;
        finalJobList.push_back(j);
        c->finalMaxH = std::max(c->finalMaxH, l.hC);
        PadJob q{};
        q.hC = l.hC;
        q.wC = l.wC;
        q.hP = l.hP;
        q.wP = l.wP;
        q.py = py;
        q.px = px;
        q.nplanes = pl.nChns;
        q.pitch = l.hP;
        q.off = l.offset;
        padJobs.push_back(q);
        q.pitch = rankPitch(l.hP);
        q.off = rankOff;
        padJobsR.push_back(q);
        c->padMaxElems = std::max<int64_t>(c->padMaxElems, int64_t(pl.nChns) * (int64_t(l.wP) * (l.hP - l.hC) + int64_t(l.wP - l.wC) * l.hC)); // border cells
        rankOffs.push_back(rankOff);
        rankOff += int64_t(pl.nChns) * rankPitch(l.hP) * l.wP;
    }
    return ACF_HIP_OK;
}

int PlanBuild::levelJobs()
{
    int rc = ACF_HIP_OK;
    (void)rc;
    // level jobs (k_level): every level, real ones read their raw channels, approximated ones resample on the
    // fly; sorted into runs of equal (rows-per-lane R, mode) because both are template parameters of the kernel
    {
        struct Keyed
        {
            int key;
            LevelJob j;
            int level;
        };
        std::vector<Keyed> fusedJobs, rawJobs;
        c->fusedOk = p.smooth > 0;
        // acf_hip_get_level_forms' words: every decision below leaves its bit on the level it was made for
        c->levelFormFused.assign(pl.levels.size(), 0);
        c->levelFormRaw.assign(pl.levels.size(), 0);
        auto notFused = [&](size_t level, int32_t why) {
            c->fusedOk = false;
            c->levelFormFused[level] |= why;
        };
        int ai = 0;
        for (size_t i = 0; i < pl.levels.size(); i++)
        {
            const acf_hip_level& l = pl.levels[i];
            LevelJob j{};
            j.hC = l.hC;
            j.wC = l.wC;
            j.out_cs = l.hP;
            j.in_off = pl.raw_off[i];
            j.raw_off = pl.raw_off[i];
            j.out_off = l.offset + int64_t(px) * l.hP + py;
            j.in_ps = int64_t(l.hC) * l.wC;
            j.out_ps = int64_t(l.hP) * l.wP;
            j.rank_cs = rankPitch(l.hP);
            j.rank_ps = int64_t(j.rank_cs) * l.wP;
            j.rank_off = rankOffs[i] + int64_t(px) * j.rank_cs + py;
            j.desc = -1;
            const int R = (l.hC + 63) / 64;
            int mode = LM_REAL;
            rawJobs.push_back({ R * 8 + LM_REAL, j, int(i) });
            if (l.hC > 64 * LEVEL_MAX_R_REAL)
            {
                notFused(i, ACF_HIP_LF_WHY_TALL); // (finalMaxH: no level kernel takes it, planLevels leaves the wave-per-plane paths)
            }
            if (!l.isReal)
            {
                j.desc = ai;
                const ResampleDesc& dd = c->h_descs[size_t(c->nImgDescs + ai)];
                if ((dd.ymode == RS_DOWN && dd.ybd0 > 3) || (dd.xmode == RS_DOWN && dd.xbd0 > 3))
                {
                    notFused(i, ACF_HIP_LF_WHY_TAPS); // more than three taps on an axis: separate launches
                }
                if (dd.ymode == RS_EXACT || dd.xmode == RS_EXACT)
                {
                    notFused(i, ACF_HIP_LF_WHY_EXACT); // an exact 1/k ratio: separate launches
                }
                mode = dd.xmode == RS_DOWN ? (dd.ymode == RS_DOWN ? LM_DD : LM_DU) : (dd.ymode == RS_DOWN ? LM_UD : LM_UU);
                if (R > 8)
                {
                    notFused(i, ACF_HIP_LF_WHY_ROWS); // (only copies of real levels are instantiated beyond eight rows per lane)
                }
                if (dd.ha >= 64 * (dd.ymode == RS_DOWN ? (3 * R + 1) / 2 : R))
                {
                    // more source rows than LevelWindow's registers hold (ratio beyond 2^(1/2)), or no row left in the
                    // column buffer for the zeros that taps beyond the source's last row read (level_column)
                    notFused(i, ACF_HIP_LF_WHY_WINDOW);
                }
                if (mode == LM_DU || mode == LM_UD)
                {
                    // one axis up, the other down: cannot happen with getScales' isotropic scales (an exhaustive scan of
                    // 64..330 x 64..330 frames finds none), so the fused kernel is not instantiated for it.  (An exact axis is "not
                    // down" above, so an exact x beside a down y lands here as well — tests/level_forms_case.py has such levels —
                    // after the exact ratio has ruled the fused path out already.)
                    notFused(i, ACF_HIP_LF_WHY_MIXED);
                }
                ai++;
            }
            fusedJobs.push_back({ R * 8 + mode, j, int(i) });
        }
        auto pack = [&](std::vector<Keyed>& v, std::vector<acf_hip_ctx::LevelGroup>& groups, LevelJob** dst, int* nAll, std::vector<int32_t>& form) {
            auto jobCost = [](const Keyed& k) {
                // one wave walks wC column steps; a step costs ~R row registers x (1 for a copy, 3 for a resampled column) + the recursion
                const int R = k.key / 8, mode = k.key % 8;
                return double(k.j.wC) * (R * (mode == LM_REAL ? 1.0 : 3.0) + 2.0);
            };
            for (auto& k : v)
            {
                k.j.kind = k.key;
            }
            // k_level_all takes every job whose specialisation fits 128 VGPRs, longest chain first; the rest go out as
            // one launch per (R, mode) run on the side streams
            std::vector<Keyed> all, rest;
            for (const auto& k : v)
            {
                const int R = k.key / 8, mode = k.key % 8;
                const bool toAll = (R <= 4 || (mode == LM_REAL && R <= 8)) && !fallbackForced(FB_LEVEL_GROUPS);
                (toAll ? all : rest).push_back(k);
                form[size_t(k.level)] |= R | mode << 8 | (toAll ? ACF_HIP_LF_BY_ALL : ACF_HIP_LF_BY_GROUP) << 12;
            }
            std::stable_sort(all.begin(), all.end(), [&](const Keyed& a, const Keyed& b) { return jobCost(a) > jobCost(b); });
            std::stable_sort(rest.begin(), rest.end(), [](const Keyed& a, const Keyed& b) { return a.key < b.key; });
            std::vector<LevelJob> flat;
            for (const auto& k : all)
            {
                flat.push_back(k.j);
            }
            *nAll = int(all.size());
            for (const auto& k : rest)
            {
                if (groups.empty() || groups.back().R * 8 + groups.back().mode != k.key)
                {
                    groups.push_back({ k.key / 8, k.key % 8, int(flat.size()), 0, 0.0, 0 });
                }
                groups.back().count++;
                groups.back().cost += jobCost(k);
                flat.push_back(k.j);
            }
            return devUpload(c, dst, flat);
        };
        if ((rc = pack(fusedJobs, c->levelGroups, &c->d_levelJobs, &c->nAllJobs, c->levelFormFused)) ||
            (rc = pack(rawJobs, c->levelGroupsRaw, &c->d_levelJobsRaw, &c->nAllJobsRaw, c->levelFormRaw)))
        {
            return rc;
        }
        c->levelsEmitRank = c->fusedOk && c->levelGroups.empty() && c->nAllJobs == int(pl.levels.size());
        for (const auto& l : pl.levels)
        {
            if ((py & 1) && l.hC % 64 == 0)
            {
                c->levelsEmitRank = false; // (level_body's paired rank stores: no lane holds row hC)
            }
        }
    }
    return ACF_HIP_OK;
}

int PlanBuild::ldcf()
{
    int rc = ACF_HIP_OK;
    // ---- LDCF post-stage (acf_hip_params::ldcfK): level table of the filtered, halved pyramid + one resample per level
    LdcfStage& L = c->ldcf;
    if (p.ldcfK <= 0)
    {
        return ACF_HIP_OK;
    }
    const int shrink2 = 2 * p.shrink, nCk = pl.nChns * p.ldcfK;
    L.descBase = int(c->h_descs.size());
    L.tmpFloats = int64_t(p.ldcfK) * pl.pyr_floats;
    std::vector<LdcfJob> jobs;
    for (size_t i = 0; i < pl.levels.size(); i++)
    {
        acf_hip_level l = pl.levels[i];
        const acf_hip_level& s0 = pl.levels[i];
        l.hP = l.hC = int(std::floor(0.5 * s0.hP + 0.5)); // imResample(C, .5): round(.5 * size)
        l.wP = l.wC = int(std::floor(0.5 * s0.wP + 0.5));
        if (l.hP < 1 || l.wP < 1)
        {
            return fail(c, ACF_HIP_E_UNSUPPORTED, "plan: LDCF level smaller than one cell");
        }
        l.nWinR = std::max(0, int(std::ceil(float(l.hP * shrink2 - p.modelDsPad_h + 1) / p.stride)));
        l.nWinC = std::max(0, int(std::ceil(float(l.wP * shrink2 - p.modelDsPad_w + 1) / p.stride)));
        l.offset = L.floats;
        L.floats += int64_t(nCk) * l.hP * l.wP;
        L.levels.push_back(l);
        ResampleDesc dd;
        if ((rc = buildResample(s0.hP, s0.wP, l.hP, l.wP, dd, arena)))
        {
            return fail(c, rc, "plan: degenerate LDCF resample geometry");
        }
        const double one[3] = { 1.0, 1.0, 1.0 };
        setResampleGain(dd, one, nCk, nCk);
        dd.nplanes = nCk;
        dd.src_off = int64_t(p.ldcfK) * s0.offset; // the filtered scratch holds every level: k planes per channel plane
        dd.dst_off = l.offset;
        dd.src_frame_stride = L.tmpFloats;
        c->h_descs.push_back(dd);
        LdcfJob j{};
        j.h = s0.hP;
        j.w = s0.wP;
        j.inOff = s0.offset;
        j.outOff = int64_t(p.ldcfK) * s0.offset;
        jobs.push_back(j);
        L.maxCells = std::max(L.maxCells, s0.hP * s0.wP);
        L.maxBlocks = std::max(L.maxBlocks, resampleBlocks(dd));
    }
    for (size_t i = 0; i < L.levels.size(); i++)
    {
        c->h_descs[size_t(L.descBase) + i].dst_frame_stride = L.floats;
    }
    // fused path: every level tiled for k_resample_tile's passes with 16 output columns per tile
    std::vector<LdcfTileJob> tj;
    bool ok = !fallbackForced(FB_LDCF_UNFUSED);
    const int xoMax = 16; // output columns per tile at most (source tile: twice as many columns)
    // tile sizes (outputs y, x) of at most 64 x 16 outputs, the largest first
    std::vector<std::pair<int, int>> cand;
    for (int y = RT_YO; y >= 32; y--)
    {
        for (int x = xoMax; x >= xoMax / 2; x--)
        {
            cand.push_back({ y, x });
        }
    }
    std::stable_sort(cand.begin(), cand.end(), [](const std::pair<int, int>& a, const std::pair<int, int>& b) { return a.first * a.second > b.first * b.second; });
    for (size_t i = 0; i < L.levels.size() && ok; i++)
    {
        const ResampleDesc& dd = c->h_descs[size_t(L.descBase) + i];
        // the largest tile whose source tile is at most 128 rows x 32 columns: the filter stage then has exactly two tile rows
        // per lane and eight column quads (k_ldcf_tile)
        ResampleTiling tl;
        int yo = 0, xo = 0;
        for (const auto& yx : cand)
        {
            tl = resampleTilePlan(dd, arena, yx.second, int64_t(40) * 1024, yx.first, 128, 2 * xoMax);
            if (tl.rows > 0)
            {
                yo = yx.first;
                xo = yx.second;
                break;
            }
        }
        if (tl.rows <= 0)
        {
            ok = false;
            break;
        }
        L.tileRows = std::max(L.tileRows, tl.rows);
        L.tileCols = std::max(L.tileCols, tl.cols);
        const int ntY = cdiv(dd.hb, yo), ntX = cdiv(dd.wb, xo);
        for (int x = 0; x < ntX; x++)
        {
            for (int y = 0; y < ntY; y++)
            {
                LdcfTileJob j{};
                j.level = int(i);
                j.ytile = y;
                j.xtile = x;
                j.tile_y = tl.tile_y;
                j.tile_x = tl.tile_x;
                j.yo = yo;
                j.xo = xo;
                tj.push_back(j);
            }
        }
    }
    if (ok && !tj.empty())
    {
        L.tiles = int(tj.size());
        if ((rc = devUpload(c, &L.d_tileJobs, tj)))
        {
            return rc;
        }
    }
    if ((rc = devUpload(c, &L.d_jobs, jobs)) || (rc = devUpload(c, &L.d_filt, c->ldcfFilters)) ||
        (L.tiles == 0 && (rc = devAlloc(c, &L.d_tmp, size_t(B) * L.tmpFloats + 64))) || (rc = devAlloc(c, &L.d_pyr, size_t(B) * L.floats + 64)))
    {
        return rc;
    }
    return ACF_HIP_OK;
}

int PlanBuild::uploadAndScratch()
{
    int rc = ACF_HIP_OK;
    (void)rc;
    if ((rc = devUpload(c, &c->d_descs, c->h_descs)) || (rc = devUpload(c, &c->d_it, arena.ints)) || (rc = devUpload(c, &c->d_ft, arena.floats)) ||
        (rc = devUpload(c, &c->d_realJobs, realJobs)) || (rc = devUpload(c, &c->d_finalJobs, finalJobList)) || (rc = devUpload(c, &c->d_padJobs, padJobs)) || (rc = devUpload(c, &c->d_padJobsR, padJobsR)))
    {
        return rc;
    }
    if ((rc = devAlloc(c, &c->d_chns, size_t(B) * pl.raw_floats)) || (rc = devAlloc(c, &c->d_pyr, size_t(B) * pl.pyr_floats + 64)) /* + slack: the cascade's 16-byte tile fill may read a few floats past the last plane */)
    {
        return rc;
    }
    {
        // k_smooth_vec's column segments: hand-over states of up to 32 segments per plane, one repair flag per plane
        c->segCap = 32;
        const size_t nState = size_t(B) * d * c->segCap * size_t(std::max(H, 4));
        if ((rc = devAlloc(c, &c->d_specState, nState)) || (rc = devAlloc(c, &c->d_trueState, nState)) || (rc = devAlloc(c, &c->d_redo, size_t(B) * d)))
        {
            return rc;
        }
        // (zero between calls: the repair launch takes its flags down; cleared on the context's own stream, which does not
        // synchronise with the null stream, and again on the error returns between a verify and its repair launch: clearRepairFlags)
        HIPCHK(c, hipMemsetAsync(c->d_redo, 0, sizeof(int32_t) * size_t(B) * d, c->stream));
        HIPCHK(c, hipStreamSynchronize(c->stream));
        c->redoInts = size_t(B) * d;
    }
    {
        // k_level_all's column segments: only small batches are bound by a level's chain length
        c->levelSegFrames = std::min(B, 8);
        c->levelSegCap = 8;
        c->levelHMax = std::max(c->finalMaxH, 4);
        const size_t nState = size_t(c->levelSegFrames) * pl.levels.size() * pl.nChns * c->levelSegCap * size_t(c->levelHMax);
        if ((rc = devAlloc(c, &c->d_lvSpec, nState)) || (rc = devAlloc(c, &c->d_lvTrue, nState)) ||
            (rc = devAlloc(c, &c->d_lvRedo, size_t(c->levelSegFrames) * pl.levels.size() * pl.nChns)))
        {
            return rc;
        }
        HIPCHK(c, hipMemsetAsync(c->d_lvRedo, 0, sizeof(int32_t) * size_t(c->levelSegFrames) * pl.levels.size() * pl.nChns, c->stream));
        HIPCHK(c, hipStreamSynchronize(c->stream));
        c->lvRedoInts = size_t(c->levelSegFrames) * pl.levels.size() * pl.nChns;
    }
    return ACF_HIP_OK;
}

int PlanBuild::cascade()
{
    int rc = ACF_HIP_OK;
    // with LDCF the cascade runs on the filtered pyramid: its tables are built for those levels, nChns*k channels, cells of 2*shrink pixels
    const bool ldcf = p.ldcfK > 0;
    const std::vector<acf_hip_level>& cascLevels = ldcf ? c->ldcf.levels : pl.levels;
    if ((rc = buildCascadeTables(c, cascLevels, pl.nChns * std::max(p.ldcfK, 1), p.shrink * (ldcf ? 2 : 1), B, c->thrs, c->cs, !ldcf)) ||
        (rc = allocCascadeRun(c, c->cs, cascLevels, c->thrs, max_hits)))
    {
        return rc;
    }
    std::vector<BoxLevel> box(pl.levels.size());
    for (size_t i = 0; i < pl.levels.size(); i++)
    {
        box[i].shw_h = pl.levels[i].scalehw_h;
        box[i].shw_w = pl.levels[i].scalehw_w;
        // cv::Size(cv::Size2d(modelDs) / scale): saturate_cast<int>(double) == cvRound (ACF.cpp:304)
        box[i].bh = int(std::lrint(double(p.modelDs_h) / pl.levels[i].scale));
        box[i].bw = int(std::lrint(double(p.modelDs_w) / pl.levels[i].scale));
    }
    return devUpload(c, &c->d_boxLevels, box);
}
} // namespace
