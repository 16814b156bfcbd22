// The threshold-rank cell's count (acf_amd/csrc/host_plan.h: rankCount, the one text RankTables::rankOfCell and the kernels
// run) against std::upper_bound, as a stand-alone program (tests/test_rank_count_host.py builds it with the sanitizers):
// three threshold sets; every threshold and its two float neighbours in every channel; ALL 2^32 bit patterns of one
// channel per set (NaNs excluded).  Prints one line per set; exit status 0 = no mismatch.
#include "../acf_amd/csrc/host_plan.h"

#include <algorithm>
#include <atomic>
#include <cmath>
#include <cstdio>
#include <cstring>
#include <thread>
#include <vector>

using namespace acfhip;

namespace
{
float asFloat(uint32_t b)
{
    float v;
    std::memcpy(&v, &b, 4);
    return v;
}
uint32_t asBits(float v)
{
    uint32_t b;
    std::memcpy(&b, &v, 4);
    return b;
}

struct Set
{
    const char* name;
    int nChns, sweepChn;
    std::vector<float> thrs;   // one per node
    std::vector<int32_t> chn;  // the node's channel
    std::vector<std::vector<float>> sorted; // per channel: distinct thresholds, -0.0 folded into +0.0
};

void finish(Set& s)
{
    s.sorted.assign(size_t(s.nChns), {});
    for (size_t q = 0; q < s.thrs.size(); q++)
    {
        s.sorted[size_t(s.chn[q])].push_back(s.thrs[q] == 0.f ? 0.f : s.thrs[q]);
    }
    for (auto& t : s.sorted)
    {
        std::sort(t.begin(), t.end());
        t.erase(std::unique(t.begin(), t.end()), t.end());
    }
}

uint32_t lcg(uint32_t& st)
{
    st = st * 1664525u + 1013904223u;
    return st >> 8;
}

// thresholds of a FACE80-like model: ~614 per channel (2048 trees x 3 nodes over 10 channels), uniform between channel quartiles
Set face80Like()
{
    Set s{ "face80-like", 4, 3, {}, {}, {} };
    const float lo[4] = { 0.13f, 0.38f, 0.355f, 0.034f }, hi[4] = { 0.20f, 0.50f, 0.44f, 0.088f };
    uint32_t st = 12345u;
    for (int z = 0; z < 4; z++)
    {
        for (int i = 0; i < 614; i++)
        {
            s.thrs.push_back(lo[z] + float(lcg(st)) / 16777216.f * (hi[z] - lo[z]));
            s.chn.push_back(z);
        }
    }
    finish(s);
    return s;
}

// 192 consecutive floats: buckets of four patterns, every bucket full, every slot of every dword in use
Set consecutive()
{
    Set s{ "192 consecutive floats", 2, 0, {}, {}, {} };
    float v = 0.25f;
    for (int i = 0; i < 192; i++)
    {
        s.thrs.push_back(v);
        s.chn.push_back(0);
        v = std::nextafter(v, 1.f);
    }
    // seven consecutive floats at the end of an aligned bucket of eight in the other channel: a full record with shift 3
    for (int i = 0; i < 7; i++)
    {
        s.thrs.push_back(asFloat(0x3f000001u + uint32_t(i)));
        s.chn.push_back(1);
    }
    finish(s);
    return s;
}

// zeros of both signs and duplicates
Set zeros()
{
    Set s{ "zeros and duplicates", 2, 0, {}, {}, {} };
    const float t0[] = { 0.5f, 0.0f, -0.0f, 0.75f, 0.5f, 0.5f, 0.75f, 0.625f, 0.5f };
    for (float t : t0)
    {
        s.thrs.push_back(t);
        s.chn.push_back(0);
    }
    const float t1[] = { 0.25f, 0.25f, 0.125f }; // no zero in this channel: its negative cells rank 0 through hasZero's select as well
    for (float t : t1)
    {
        s.thrs.push_back(t);
        s.chn.push_back(1);
    }
    finish(s);
    return s;
}

uint32_t want(const std::vector<float>& t, float v)
{
    return uint32_t(std::upper_bound(t.begin(), t.end(), v) - t.begin());
}

// patterns [b0, b1) of one sign in increasing |v|: for v >= 0 the expected rank only moves up, so it is carried along and
// checked against std::upper_bound at the chunk's first pattern; every negative v is below all thresholds but -0.0 == +0.0
uint64_t sweep(const RankTables& rt, int chn, const std::vector<float>& t, uint32_t b0, uint32_t b1)
{
    uint64_t bad = 0;
    uint32_t r = want(t, asFloat(b0));
    size_t next = r; // first threshold > the current value
    for (uint32_t b = b0; b != b1; b++)
    {
        const float v = asFloat(b);
        while (next < t.size() && t[next] <= v)
        {
            next++;
        }
        bad += rt.rankOfCell(chn, v) != uint32_t(next) ? 1u : 0u;
    }
    const uint32_t zr = want(t, -0.0f);
    for (uint32_t b = b0; b != b1; b++)
    {
        const uint32_t e = b == 0 ? zr : 0u;
        bad += rt.rankOfCell(chn, asFloat(b | 0x80000000u)) != e ? 1u : 0u;
    }
    return bad;
}
} // namespace

int main()
{
    Set sets[3] = { face80Like(), consecutive(), zeros() };
    const unsigned nThreads = std::max(1u, std::min(16u, std::thread::hardware_concurrency()));
    uint64_t total = 0;
    for (Set& s : sets)
    {
        RankTables rt;
        buildRankTables(s.thrs.data(), s.chn.data(), s.thrs.size(), s.nChns, rt);
        if (!rt.ok)
        {
            std::printf("%s: no tables: %s\n", s.name, rt.why.c_str());
            return 2;
        }
        uint64_t bad = 0, probes = 0;
        int full = 0; // records with seven slots in use
        for (int z = 0; z < s.nChns; z++)
        {
            const std::vector<float>& t = s.sorted[size_t(z)];
            if (rt.chan[size_t(z)].nThr != int32_t(t.size()))
            {
                bad++;
            }
            for (int b = 0; b < rt.chan[size_t(z)].nb; b++)
            {
                full += rt.rec[size_t(rt.chan[size_t(z)].recOff + b)].tr[5] != 0 ? 1 : 0;
            }
            std::vector<float> v = { 0.f, -0.f, 1e-45f, -1e-45f, -1.f, -3e38f, 3e38f, 1.f, INFINITY, -INFINITY };
            for (float x : t)
            {
                v.push_back(x);
                v.push_back(std::nextafter(x, -INFINITY));
                v.push_back(std::nextafter(x, INFINITY));
            }
            for (float x : v)
            {
                probes++;
                bad += rt.rankOfCell(z, x) != want(t, x) ? 1u : 0u;
            }
        }
        // all finite and infinite patterns of one channel (magnitudes 0 .. 0x7f800000, both signs)
        const uint32_t end = 0x7f800001u, step = (end + nThreads - 1) / nThreads;
        std::atomic<uint64_t> badSweep{ 0 };
        std::vector<std::thread> pool;
        for (unsigned i = 0; i < nThreads; i++)
        {
            const uint32_t b0 = std::min(end, i * step), b1 = std::min(end, b0 + step);
            pool.emplace_back([&, b0, b1] { badSweep += sweep(rt, s.sweepChn, s.sorted[size_t(s.sweepChn)], b0, b1); });
        }
        for (auto& th : pool)
        {
            th.join();
        }
        std::printf("%s: hasZero %d, %d full records, %llu probes + %llu patterns of channel %d, %llu mismatches\n", s.name, int(rt.hasZero), full,
            (unsigned long long)probes, 2ull * end, s.sweepChn, (unsigned long long)(bad + badSweep.load()));
        total += bad + badSweep.load();
    }
    return total == 0 ? 0 : 1;
}
