// crt_matte.hip -- the id mattes (include/crt.h, crt_render_mattes): per pixel, which ids its camera rays hit and how many
// rays hit each, in the Cryptomatte style.  The camera ray of sample s of pixel (x, y) is a pure function of (x, y, s)
// (primary_ray), so the mattes are rendered after the fact, as the feature planes are (crt_aov.hip): the path-tracing
// kernels are not involved.  DESIGN.md 6o has the definition this follows operation by operation (tests/matte_ref.py is
// its restatement).
#include "crt_launch.h"
#include "crt_shade.h"

namespace crt {

// grid = tiles_x * tiles_y blocks of 64 threads, block -> 8x8 pixel tile: k_aov's layout, walk, LDS stack and sample loop.
// Each lane keeps its pixel's table of P.slots (id, count) entries in LDS, laid out [slot][lane] so that the wave's
// access to slot s touches 64 consecutive dwords (the table is indexed at run time: a register array would go to
// scratch).  Dynamic LDS: P.slots * 64 ids, then P.slots * 64 counts.  A lane touches its own column only: no atomics,
// no barrier, no cross-lane step.
__global__ __launch_bounds__(64) void k_matte(const DevScene S, const MatteParams P)
{
    __shared__ int lds_stack[kStackDepth * 64];
    extern __shared__ uint32_t lds_table[];
    const uint32_t lane = threadIdx.x;
    const uint32_t lx = (blockIdx.x % P.tiles_x) * 8u + (lane & 7u), ly = (blockIdx.x / P.tiles_x) * 8u + (lane >> 3);
    if (lx >= P.tw || ly >= P.th) return;
    int *stk = lds_stack + lane;
    uint32_t *tid = lds_table + lane, *tcount = lds_table + P.slots * 64u + lane;     // entry s: tid[s * 64], tcount[s * 64]
    const uint32_t px = P.x0 + lx, py = P.y0 + ly;
    const uint32_t n = P.counts ? P.counts[blockIdx.x] : P.n;
    const uint32_t tea_xy = tea(px, py * 100u);
    uint32_t h = 0, used = 0, over = 0;
    for (uint32_t j = 1; j <= n; j++) {
        Rng rng;
        f3 o, d;
        primary_ray(S, px, py, P.first + j, tea_xy, rng, o, d);
        // the closest hit as k_aov finds it
        float t_max = CRT_INFINITY;
        uint32_t b_index = kNoHit, b_slot = kNoHit, cn = 0, cp = 0;
        if (P.brute || !finite3(o) || !finite3(d)) {
            for (uint32_t i = 0; i < S.nprim; i++)
                hit_test<true>(S, S.slot_of_index[i], o, d, 0xFFFFFFFFu, 0.001f, t_max, b_index, b_slot);
        } else {
            traverse<false>(S, stk, o, d, 0xFFFFFFFFu, false, t_max, b_index, b_slot, cn, cp);
        }
        if (b_slot == kNoHit) continue;
        uint32_t id = b_index;                                           // CRT_MATTE_PRIMITIVE
        if (P.source == CRT_MATTE_OBJECT) {
            id = P.table[b_index];
        } else if (P.source == CRT_MATTE_MATERIAL) {
            const uint32_t meta = f_bits(S.prim[3 * b_slot].w);
            id = (((meta >> 2) & 3u) << 24) | ((meta >> 18) & 0x3FFFu);   // k_dn_gbuffer's key: material, reflectance index
        }
        h++;
        uint32_t s = 0;
        while (s < used && tid[s * 64u] != id) s++;
        if (s < used) {
            tcount[s * 64u]++;
        } else if (used < P.slots) {
            tid[used * 64u] = id;
            tcount[used * 64u] = 1u;
            used++;
        } else {
            over++;
        }
    }
    // the ranking: selection in place, count descending, equal counts by id ascending; plane-major stores
    const size_t npix = (size_t)P.tw * P.th, pix = (size_t)ly * P.tw + lx;
    for (uint32_t r = 0; r < P.slots; r++) {
        uint32_t id = 0xFFFFFFFFu, count = 0;
        if (r < used) {
            uint32_t best = r;
            id = tid[r * 64u];
            count = tcount[r * 64u];
            for (uint32_t s = r + 1; s < used; s++) {
                const uint32_t is = tid[s * 64u], cs = tcount[s * 64u];
                if (cs > count || (cs == count && is < id)) { best = s; id = is; count = cs; }
            }
            if (best != r) {
                tid[best * 64u] = tid[r * 64u];
                tcount[best * 64u] = tcount[r * 64u];
            }
        }
        if (P.ids) P.ids[r * npix + pix] = id;
        if (P.counts_out) P.counts_out[r * npix + pix] = count;
    }
    if (P.hits) P.hits[pix] = h;
    if (P.overflow) P.overflow[pix] = over;
}

hipError_t matte_launch(const DevScene &S, const MatteParams &P, hipStream_t stream)
{
    const uint32_t tiles_y = (P.th + 7) / 8;
    if (P.tiles_x * tiles_y == 0) return hipSuccess;
    hipLaunchKernelGGL(k_matte, dim3(P.tiles_x * tiles_y), dim3(64), (size_t)P.slots * 64u * 2u * sizeof(uint32_t), stream, S, P);
    return hipGetLastError();
}

}  // namespace crt
