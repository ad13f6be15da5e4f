// work_map_test.cpp -- the region-major shards of a batch's work queue (crt_work_map.h, option "wf_affinity") enumerated on
// the CPU: for every frame size (in tiles) and sample count below, every shard's every local chunk is mapped and the
// whole is checked to be a partition of the batch's (sample, tile) chunks.  Built and run by tests/test_work_map_cpu.py;
// includes nothing but the mapping's header.
#include <cstdio>
#include <vector>

#include "crt_work_map.h"

using namespace crt;

static int g_failed = 0, g_checked = 0;
#define CHECK(cond)                                                                    \
    do {                                                                               \
        g_checked++;                                                                   \
        if (!(cond)) { g_failed++; std::printf("FAILED %s:%d: %s (tiles %u, samples %u)\n", __FILE__, __LINE__, #cond, T, n); } \
    } while (0)

static void enumerate(uint32_t T, uint32_t n)
{
    const uint32_t shards = kWmRegions * kWmGroups;
    // regions: consecutive runs of the tile order that cover it, sizes within one tile of each other
    uint32_t lo = 0xFFFFFFFFu, hi = 0, next = 0;
    for (uint32_t k = 0; k < kWmRegions; k++) {
        const uint32_t t = wm_region_tiles(T, k);
        CHECK(wm_region_first(T, k) == next);
        next += t;
        lo = t < lo ? t : lo; hi = t > hi ? t : hi;
    }
    CHECK(next == T);
    CHECK(hi - lo <= 1u);
    // sample groups cover the samples
    uint32_t ns = 0;
    for (uint32_t g = 0; g < kWmGroups; g++) ns += wm_group_samples(n, g);
    CHECK(ns == n);
    // every (sample, tile) chunk exactly once
    std::vector<uint32_t> seen((size_t)T * n, 0u);
    unsigned long long total = 0;
    uint32_t empty = 0;
    bool in_range = true, in_region = true, in_group = true, tile_major = true;
    for (uint32_t s = 0; s < shards; s++) {
        const uint32_t chunks = wm_shard_chunks(n, T, s), size = wm_shard_size(n, T, s);
        CHECK(size % 64u == 0u && size == 64u * chunks);         // a shard's range is [0, size) in whole chunks of 64 ids
        total += size;
        if (chunks == 0u) empty++;
        const uint32_t k = s % kWmRegions, g = s / kWmRegions;
        uint32_t last_tile = 0;
        for (uint32_t c = 0; c < chunks; c++) {
            const WmChunk w = wm_chunk(n, T, s, c);
            if (!(w.sample < n && w.tile < T)) { in_range = false; continue; }
            if (!(w.tile >= wm_region_first(T, k) && w.tile < wm_region_first(T, k) + wm_region_tiles(T, k))) in_region = false;
            if (w.sample % kWmGroups != g) in_group = false;
            if (c > 0 && w.tile < last_tile) tile_major = false;
            last_tile = w.tile;
            seen[(size_t)w.sample * T + w.tile]++;
        }
    }
    CHECK(in_range);
    CHECK(in_region);
    CHECK(in_group);
    CHECK(tile_major);
    CHECK(total == 64ull * T * n);
    bool once = true;
    for (uint32_t v : seen) once = once && v == 1u;
    CHECK(once);
    // fewer tiles than regions, or fewer samples than groups: empty shards, and (above) no lost work
    const uint32_t regions_used = T < kWmRegions ? T : kWmRegions, groups_used = n < kWmGroups ? n : kWmGroups;
    CHECK(empty == shards - regions_used * groups_used);
}

int main()
{
    const uint32_t tiles[] = {1, 5, 7, 8, 9, 45, 32400}, samples[] = {1, 3, 8, 13, 64};
    for (uint32_t T : tiles)
        for (uint32_t n : samples) enumerate(T, n);
    std::printf("%d checked, %d failed\n", g_checked, g_failed);
    return g_failed ? 1 : 0;
}
