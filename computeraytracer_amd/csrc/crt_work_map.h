// crt_work_map.h -- which (sample, tile) chunks a shard of a batch's work queue hands out under option "wf_affinity"
// (DESIGN.md 5.11).  Shared by host and device; compiles without HIP (tests/host/work_map_test.cpp).
//
// A work id keeps its meaning: id = sample_off * npix_padded + tile * 64 + lane, a chunk is the 64 ids of one 8x8 tile of
// one sample.  The queue has 64 shards; shard s = 8 * g + k serves image REGION k (= s mod 8) and sample GROUP g:
//   regions   runs of tiles in the frame's tile order (row-major 8x8 tiles of the tile rectangle), sizes differing by at
//             most one tile: region k holds tiles [wm_region_first(T, k), + wm_region_tiles(T, k)) of the T tiles
//   groups    the batch's samples congruent to g modulo 8: S_g = wm_group_samples(n, g) of its n samples
// and its local chunk c, 0 <= c < S_g * tiles of region k, is
//   tile      region_first[k] + c / S_g
//   sample    g + 8 * (c mod S_g)
// -- tile-major, sample-minor: a shard sweeps its region once, every tile S_g samples deep.  Fewer tiles than regions, or
// fewer samples than groups, leave shards empty; every chunk belongs to exactly one shard.
#pragma once
#include <stdint.h>

#if defined(__HIP__)                                             // (spelled out: the HIP runtime's header need not be included first)
#define CRT_WM_FN __attribute__((host)) __attribute__((device)) inline __attribute__((always_inline))
#else
#define CRT_WM_FN inline
#endif

namespace crt {

constexpr uint32_t kWmRegions = 8, kWmGroups = 8;               // kWmRegions * kWmGroups = kWfShards (crt_device.h)

CRT_WM_FN uint32_t wm_group_samples(uint32_t n, uint32_t g) { return n > g ? (n - g + kWmGroups - 1u) / kWmGroups : 0u; }
CRT_WM_FN uint32_t wm_region_tiles(uint32_t T, uint32_t k) { return T / kWmRegions + (k < T % kWmRegions ? 1u : 0u); }
CRT_WM_FN uint32_t wm_region_first(uint32_t T, uint32_t k) { const uint32_t r = T % kWmRegions; return k * (T / kWmRegions) + (k < r ? k : r); }

// chunks / work ids of shard s (its cursor runs over [0, wm_shard_size) in steps of 64)
CRT_WM_FN uint32_t wm_shard_chunks(uint32_t n, uint32_t T, uint32_t s) { return wm_group_samples(n, s / kWmRegions) * wm_region_tiles(T, s % kWmRegions); }
CRT_WM_FN uint32_t wm_shard_size(uint32_t n, uint32_t T, uint32_t s) { return 64u * wm_shard_chunks(n, T, s); }

struct WmChunk { uint32_t sample, tile; };                      // sample: offset within the batch

// local chunk c of shard s (c < wm_shard_chunks(n, T, s), so S_g > 0)
CRT_WM_FN WmChunk wm_chunk(uint32_t n, uint32_t T, uint32_t s, uint32_t c)
{
    const uint32_t g = s / kWmRegions, k = s % kWmRegions, S = wm_group_samples(n, g);
    WmChunk r;
    r.tile = wm_region_first(T, k) + c / S;
    r.sample = g + kWmGroups * (c % S);
    return r;
}

}  // namespace crt
