// crt_adaptive.hip -- adaptive sampling (include/crt.h "Adaptive sampling"): which 8x8 tiles of the
// context's rectangle get more samples.
//
//   k_as_select    one wave per tile: each lane the error e of its pixel (the f32 contract below), the wave the tile's
//                  error E = max e (NaN -> +inf, so the maximum does not depend on order); writes E and the active flag
//   k_as_select_var  the same shape for crt_trace_adaptive_filtered: each lane the variance v' that the
//                  adaptive filter left for its pixel, the wave E' = sqrt(max v'); E' and the flag go where E and its go
//   k_as_compact   one block: the active tiles into a list in ascending tile order (neighbouring tiles stay neighbouring
//                  work), and its length -- the only number the host reads back
//   k_as_commit    after the call's last resolve, in stream order: the active tiles' counts grow by the call's samples
//
// The sampling itself runs in the adaptive instantiations of k_trace (crt_kernels.hip) and of k_wf_gen / k_wf_resolve
// (crt_wavefront.hip); they take the tile's first sample from its count at the start of the call.
#include <hip/hip_runtime.h>

#include "crt_adaptive.h"
#include "crt_device.h"
#include "crt_launch.h"
#include "crt_math.h"

namespace crt {
namespace {

constexpr float kInf = __builtin_inff();

// (e of one pixel: pixel_error of crt_adaptive.h)

__global__ __launch_bounds__(64) void k_as_select(const AsParams A)
{
    const uint32_t tile = blockIdx.x, lane = threadIdx.x;
    const uint32_t lx = (tile % A.tiles_x) * 8u + (lane & 7u), ly = (tile / A.tiles_x) * 8u + (lane >> 3);
    const uint32_t n_t = A.counts[tile];
    float e = 0.0f;                                              // (e >= +0 for every pixel: 0 is neutral)
    if (lx < A.tw && ly < A.th && n_t >= 2u) {
        const size_t pix = (size_t)ly * A.tw + lx;
        e = pixel_error(A.accum[pix].y, A.q[pix], n_t);
        if (e != e) e = kInf;
    }
    for (int o = 32; o > 0; o >>= 1) e = fmaxf(e, __shfl_xor(e, o, 64));
    if (lane == 0) {
        const float E = n_t < 2u ? kInf : e;
        A.errors[tile] = E;
        const bool below_max = A.max_samples == 0u || n_t < A.max_samples;
        A.flags[tile] = (below_max && (n_t < A.min_samples || !(E <= A.threshold))) ? 1u : 0u;
    }
}

// v' >= +0 wherever it is a number, so 0 is neutral here too; the square root is taken once, of the maximum.
__global__ __launch_bounds__(64) void k_as_select_var(const AsVarParams V)
{
    const uint32_t tile = blockIdx.x, lane = threadIdx.x;
    const uint32_t lx = (tile % V.tiles_x) * 8u + (lane & 7u), ly = (tile / V.tiles_x) * 8u + (lane >> 3);
    const uint32_t n_t = V.counts[tile];
    float v = 0.0f;
    if (lx < V.tw && ly < V.th && n_t >= 2u) {
        v = V.var[(size_t)ly * V.tw + lx];
        if (v != v) v = kInf;
    }
    for (int o = 32; o > 0; o >>= 1) v = fmaxf(v, __shfl_xor(v, o, 64));
    if (lane == 0) {
        const float E = n_t < 2u ? kInf : sqrt_(v);
        V.errors[tile] = E;
        const bool below_max = V.max_samples == 0u || n_t < V.max_samples;
        V.flags[tile] = (below_max && (n_t < V.min_samples || !(E <= V.threshold))) ? 1u : 0u;
    }
}

__global__ __launch_bounds__(1024) void k_as_compact(const AsParams A)
{
    __shared__ uint32_t wsum[16];
    const uint32_t ntiles = A.tiles_x * A.tiles_y;
    const uint32_t t = threadIdx.x, lane = t & 63u, w = t >> 6;
    uint32_t base = 0;
    for (uint32_t c0 = 0; c0 < ntiles; c0 += 1024u) {
        const uint32_t i = c0 + t;
        const bool f = i < ntiles && A.flags[i] != 0u;
        const unsigned long long m = __ballot(f);
        if (lane == 0) wsum[w] = (uint32_t)__popcll(m);
        __syncthreads();
        uint32_t before = 0, total = 0;
        for (uint32_t k = 0; k < 16u; k++) {
            const uint32_t s = wsum[k];
            before += k < w ? s : 0u;
            total += s;
        }
        if (f) A.active[base + before + (uint32_t)__popcll(m & ((1ull << lane) - 1ull))] = i;
        base += total;
        __syncthreads();                                         // (wsum is rewritten by the next chunk)
    }
    if (t == 0) *A.n_active = base;
}

__global__ __launch_bounds__(256) void k_as_commit(uint32_t *counts, const uint32_t *active, uint32_t n_active, uint32_t samples)
{
    const uint32_t i = blockIdx.x * 256u + threadIdx.x;
    if (i < n_active) counts[active[i]] += samples;
}

}  // namespace

// Errors and flags of every tile; with compact, also the active list and its length.
hipError_t as_launch_select(const AsParams &A, bool compact, hipStream_t s)
{
    const uint32_t ntiles = A.tiles_x * A.tiles_y;
    if (ntiles == 0) return hipSuccess;
    hipLaunchKernelGGL(k_as_select, dim3(ntiles), dim3(64), 0, s, A);
    if (compact) hipLaunchKernelGGL(k_as_compact, dim3(1), dim3(1024), 0, s, A);
    return hipGetLastError();
}

// The same from the filter's variance plane (E' of DESIGN.md 6k); compact: null, or what k_as_compact takes.
hipError_t as_launch_select_var(const AsVarParams &V, const AsParams *compact, hipStream_t s)
{
    const uint32_t ntiles = V.tiles_x * V.tiles_y;
    if (ntiles == 0) return hipSuccess;
    hipLaunchKernelGGL(k_as_select_var, dim3(ntiles), dim3(64), 0, s, V);
    if (compact) hipLaunchKernelGGL(k_as_compact, dim3(1), dim3(1024), 0, s, *compact);
    return hipGetLastError();
}

hipError_t as_launch_commit(uint32_t *counts, const uint32_t *active, uint32_t n_active, uint32_t samples, hipStream_t s)
{
    if (n_active == 0) return hipSuccess;
    hipLaunchKernelGGL(k_as_commit, dim3((n_active + 255u) / 256u), dim3(256), 0, s, counts, active, n_active, samples);
    return hipGetLastError();
}

}  // namespace crt
