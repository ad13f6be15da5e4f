// crt_aov.hip -- the feature planes (include/crt.h, crt_render_aovs): anti-aliased alpha, depth, normal and albedo of the
// camera rays the beauty image is averaged over.  The camera ray of sample s of pixel (x, y) is a pure function of
// (x, y, s) (primary_ray), so the planes are rendered after the fact: the path-tracing kernels are not involved.
// DESIGN.md 6n has the definition this follows operation by operation (tests/aov_ref.py is its restatement).
#include "crt_launch.h"
#include "crt_shade.h"

namespace crt {

// grid = tiles_x * tiles_y blocks of 64 threads, block -> 8x8 pixel tile: k_dn_gbuffer's layout, walk and LDS stack, with
// a sample loop around the walk.  The block's tile is the adaptive state's tile, so the trip count is uniform per block.
// The running sums live in registers and are taken in sample order: no atomics, no cross-lane step.
__global__ __launch_bounds__(64) void k_aov(const DevScene S, const AovParams P)
{
    __shared__ int lds_stack[kStackDepth * 64];
    const uint32_t lane = threadIdx.x;
    const uint32_t lx = (blockIdx.x % P.tiles_x) * 8u + (lane & 7u), ly = (blockIdx.x / P.tiles_x) * 8u + (lane >> 3);
    if (lx >= P.tw || ly >= P.th) return;
    int *stk = lds_stack + lane;
    const uint32_t px = P.x0 + lx, py = P.y0 + ly;
    const uint32_t n = P.counts ? P.counts[blockIdx.x] : P.n;
    const uint32_t tea_xy = tea(px, py * 100u);
    uint32_t h = 0;
    float st = 0.0f;
    f3 sn = f3{0, 0, 0}, sa = f3{0, 0, 0};
    for (uint32_t j = 1; j <= n; j++) {
        Rng rng;
        f3 o, d;
        primary_ray(S, px, py, P.first + j, tea_xy, rng, o, d);
        // the closest hit as k_dn_gbuffer finds it
        float t_max = CRT_INFINITY;
        uint32_t b_index = kNoHit, b_slot = kNoHit, cn = 0, cp = 0;
        if (P.brute || !finite3(o) || !finite3(d)) {
            // intersect_all's loop, in line: the call takes the scene and its results by reference, which puts a copy of
            // the scene and the four results into scratch (240 bytes per lane in k_dn_gbuffer)
            for (uint32_t i = 0; i < S.nprim; i++)
                hit_test<true>(S, S.slot_of_index[i], o, d, 0xFFFFFFFFu, 0.001f, t_max, b_index, b_slot);
        } else {
            traverse<false>(S, stk, o, d, 0xFFFFFFFFu, false, t_max, b_index, b_slot, cn, cp);
        }
        if (b_slot != kNoHit) {
            f3 pos, nrm;
            uint32_t meta;
            hit_attributes(S, b_slot, o, d, t_max, pos, nrm, meta);
            const float *a = P.albedo + 3u * ((meta >> 18) & 0x3FFFu);      // the row of the reflectance index (data4.y)
            h++;
            st = st + t_max;
            sn = sn + nrm;
            sa = sa + f3{a[0], a[1], a[2]};
        }
    }
    const size_t pix = (size_t)ly * P.tw + lx;
    const float hf = (float)h;
    if (P.hits) P.hits[pix] = h;
    if (P.alpha) P.alpha[pix] = hf / (float)n;
    if (P.depth) P.depth[pix] = h ? st / hf : CRT_INFINITY;
    if (h) { sn = sn / hf; sa = sa / hf; }
    if (P.normal) P.normal[pix] = float4{sn.x, sn.y, sn.z, 0.0f};
    if (P.albedo_out) P.albedo_out[pix] = float4{sa.x, sa.y, sa.z, 0.0f};
}

hipError_t aov_launch(const DevScene &S, const AovParams &P, hipStream_t stream)
{
    const uint32_t tiles_y = (P.th + 7) / 8;
    if (P.tiles_x * tiles_y == 0) return hipSuccess;
    hipLaunchKernelGGL(k_aov, dim3(P.tiles_x * tiles_y), dim3(64), 0, stream, S, P);
    return hipGetLastError();
}

}  // namespace crt
