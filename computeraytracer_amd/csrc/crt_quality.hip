// crt_quality.hip -- the surface-area cost of a tree as it lies on the device (include/crt.h crt_accel_quality pins the
// definition).  A(box) = dx*dy + dy*dz + dz*dx in binary64 on the box values converted from what the
// device holds; per node i with box_i = the union of its live child boxes:
//   boxes = sum_i w_i * A(box_i)                      w_i = 2 (BVH2), the node's live children (4-wide)
//   prims = sum over leaf children  count * A(child box)
// both divided once, at the end, by A(root box).
//
//   k_quality_nodes<L>  one thread per node of the dense node array: the node's two terms, summed over the wave by
//                       shuffles of the doubles' halves, over the block's four waves through LDS, one pair stored per
//                       block; the root's thread stores A(root)
//   k_quality_sum       one block: the per-block pairs in index order (thread t takes t, t + 256, ...), the same block
//                       sum, the division
//
// Every sum has a fixed shape and there is no atomic: two calls on the same tree return the same bits.  Lanes past the
// end add +0, which is exact (every term is >= 0 or not finite).  L: 0 = BVH2 (16 floats per node), 1 = float 4-wide
// (32 floats), 2 = quantised 4-wide (16 dwords; plane = (double)base + (double)q * (double)scale, the product exact).
#include <hip/hip_runtime.h>

#include "crt_bvh.h"
#include "crt_launch.h"
#include "crt_math.h"

namespace crt {
namespace {

struct QGrid { double base[3], scale[3]; };

template <int L> struct QLayout;
template <> struct QLayout<0> { static constexpr int kDwords = 16, kWidth = 2; };
template <> struct QLayout<1> { static constexpr int kDwords = 32, kWidth = 4; };
template <> struct QLayout<2> { static constexpr int kDwords = 16, kWidth = 4; };

// Child c of a node held in w: its reference and its box.
template <int L>
__device__ __forceinline__ int quality_child(const uint32_t *w, int c, const QGrid &g, double lo[3], double hi[3])
{
    if (L == 0) {
        for (int a = 0; a < 3; a++) { lo[a] = (double)bits_f(w[6 * c + a]); hi[a] = (double)bits_f(w[6 * c + 3 + a]); }
        return (int)w[12 + c];
    }
    if (L == 1) {
        for (int a = 0; a < 3; a++) { lo[a] = (double)bits_f(w[4 * a + c]); hi[a] = (double)bits_f(w[12 + 4 * a + c]); }
        return (int)w[24 + c];
    }
    for (int a = 0; a < 3; a++) {
        const int jl = 4 * a + c, jh = 12 + 4 * a + c;           // 16-bit planes, two per dword (crt_bvh.h Bvh4Q)
        const uint32_t ql = (w[jl >> 1] >> (16 * (jl & 1))) & 0xFFFFu, qh = (w[jh >> 1] >> (16 * (jh & 1))) & 0xFFFFu;
        lo[a] = g.base[a] + (double)ql * g.scale[a];
        hi[a] = g.base[a] + (double)qh * g.scale[a];
    }
    return (int)w[12 + c];
}

__device__ __forceinline__ double quality_area(const double lo[3], const double hi[3])
{
    const double dx = hi[0] - lo[0], dy = hi[1] - lo[1], dz = hi[2] - lo[2];
    return (dx * dy + dy * dz) + dz * dx;
}

__device__ __forceinline__ double shfl_down_f64(double v, int off)
{
    const int lo = __shfl_down(__double2loint(v), off, 64), hi = __shfl_down(__double2hiint(v), off, 64);
    return __hiloint2double(hi, lo);
}

// The block's sums of b and p, in thread 0: lane l of a wave adds lane l + 32, 16, .. 1; wave w's sums meet as
// (w0 + w1) + (w2 + w3).
__device__ __forceinline__ void quality_block_sum(double &b, double &p)
{
    __shared__ double s[2][4];
    for (int off = 32; off > 0; off >>= 1) { b += shfl_down_f64(b, off); p += shfl_down_f64(p, off); }
    if ((threadIdx.x & 63u) == 0u) { s[0][threadIdx.x >> 6] = b; s[1][threadIdx.x >> 6] = p; }
    __syncthreads();
    if (threadIdx.x == 0u) { b = (s[0][0] + s[0][1]) + (s[0][2] + s[0][3]); p = (s[1][0] + s[1][1]) + (s[1][2] + s[1][3]); }
}

template <int L>
__global__ __launch_bounds__(256) void k_quality_nodes(const uint4 *__restrict__ nodes, uint32_t n, uint32_t root, QGrid g,
                                                       double2 *__restrict__ partial, double *__restrict__ root_area)
{
    constexpr int kDwords = QLayout<L>::kDwords, kWidth = QLayout<L>::kWidth;
    const uint32_t i = blockIdx.x * 256u + threadIdx.x;
    double boxes = 0.0, prims = 0.0;
    if (i < n) {
        uint32_t w[kDwords];
        for (int k = 0; k < kDwords / 4; k++) {
            const uint4 v = nodes[(size_t)i * (kDwords / 4) + k];
            w[4 * k + 0] = v.x; w[4 * k + 1] = v.y; w[4 * k + 2] = v.z; w[4 * k + 3] = v.w;
        }
        double blo[3] = {0.0, 0.0, 0.0}, bhi[3] = {0.0, 0.0, 0.0};
        uint32_t live = 0;
        for (int c = 0; c < kWidth; c++) {
            double lo[3], hi[3];
            const int ref = quality_child<L>(w, c, g, lo, hi);
            if (kWidth == 4 && ref == 0) continue;               // empty slot
            for (int a = 0; a < 3; a++) { blo[a] = live ? fmin(blo[a], lo[a]) : lo[a]; bhi[a] = live ? fmax(bhi[a], hi[a]) : hi[a]; }
            live++;
            if (ref < 0) prims += (double)(((uint32_t)(~ref) & 7u) + 1u) * quality_area(lo, hi);
        }
        const double A = quality_area(blo, bhi);
        boxes = (double)(kWidth == 2 ? 2u : live) * A;
        if (i == root) *root_area = A;
    }
    quality_block_sum(boxes, prims);
    if (threadIdx.x == 0u) partial[blockIdx.x] = double2{boxes, prims};
}

__global__ __launch_bounds__(256) void k_quality_sum(const double2 *__restrict__ partial, uint32_t nb, const double *__restrict__ root_area,
                                                     double *__restrict__ out)
{
    double boxes = 0.0, prims = 0.0;
    for (uint32_t j = threadIdx.x; j < nb; j += 256u) { const double2 v = partial[j]; boxes += v.x; prims += v.y; }
    quality_block_sum(boxes, prims);
    if (threadIdx.x == 0u) { const double A = *root_area; out[0] = boxes / A; out[1] = prims / A; }
}

}  // namespace

// nodes: n nodes of `layout` (0 BVH2, 1 float 4-wide, 2 quantised 4-wide on the grid base / scale), root < n.
// partial: (n + 255) / 256 pairs; out: 3 doubles -- boxes, prims, and A(root) as the first launch left it.
hipError_t quality_launch(int layout, const void *nodes, uint32_t n, uint32_t root, const float base[3], const float scale[3],
                          double2 *partial, double *out, hipStream_t s)
{
    if (n == 0 || root >= n) return hipErrorInvalidValue;
    QGrid g;
    for (int a = 0; a < 3; a++) { g.base[a] = (double)base[a]; g.scale[a] = (double)scale[a]; }
    const unsigned nb = (unsigned)((n + 255u) / 256u);
    const uint4 *nd = (const uint4 *)nodes;
    if (layout == 0) hipLaunchKernelGGL(k_quality_nodes<0>, dim3(nb), dim3(256), 0, s, nd, n, root, g, partial, out + 2);
    else if (layout == 1) hipLaunchKernelGGL(k_quality_nodes<1>, dim3(nb), dim3(256), 0, s, nd, n, root, g, partial, out + 2);
    else hipLaunchKernelGGL(k_quality_nodes<2>, dim3(nb), dim3(256), 0, s, nd, n, root, g, partial, out + 2);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(k_quality_sum, dim3(1), dim3(256), 0, s, (const double2 *)partial, nb, (const double *)(out + 2), out);
    return hipGetLastError();
}

}  // namespace crt
