// crt_ploc.hip -- BVH2 construction on the GPU by parallel locally-ordered clustering (D. Meister, J. Bittner, "Parallel
// Locally-Ordered Clustering for Bounding Volume Hierarchy Construction", TVCG 2018): bottom-up agglomerative
// clustering over the Morton-sorted primitives the LBVH build already produces (crt_lbvh.hip: bounds, keys, sort).
// Produces the same `Bvh` structure as the other builders, so collapse, quantisation, refit and every kernel are shared
// and the image is the same; the tree is closer to the SAH builder's than the LBVH's ("GPU build, clustered").
//
//   start   m = n clusters; cluster p is the leaf of sorted position p
//   round   (while m > 1)
//     k_ploc_nn     nn[i] = the j in [i - R, i + R], j != i, that minimises (surface of the union box, i XOR j)
//     k_ploc_mark   i leads a merge iff nn[nn[i]] == i and i < nn[i]; cluster nn[i] then disappears
//     (scan)        exclusive sums of the keep and made flags, one 64-bit scan
//     k_ploc_emit   survivors move to their scanned position; a leader writes the node record (crt_bvh.h) and the merged
//                   cluster.  The k-th node made is node n - 2 - k: the root is node 0, a child's id exceeds its parent's
//     the host reads the new m back (8 bytes), as the collapse loop does per level
//   slots   k_ploc_slots, one launch per round in reverse: first[child 0] = first[node], first[child 1] = first[node] +
//           count[child 0]; a leaf's slot is its first, its reference becomes ~(slot << 3), order[slot] its key
// Kernel boundaries are the only ordering: no fences, flags or arrival counters.  The XOR of the positions breaks ties
// symmetrically, so the smallest pair of a round is always mutual and equal costs pair up (0,1), (2,3), ... into a
// balanced tree (with "lowest index wins", 300 coincident triangles merge one pair per round into a 299-level chain).
#include <hip/hip_runtime.h>
#include <hipcub/hipcub.hpp>

#include <algorithm>
#include <cfloat>
#include <utility>
#include <vector>

#include "crt_bvh.h"
#include "crt_ctx.h"
#include "crt_launch.h"
#include "crt_math.h"

namespace crt {
namespace {

constexpr int kPlocBlock = 256;
constexpr int kPlocMaxRadius = 32;
constexpr int kPlocStage = kPlocBlock + 2 * kPlocMaxRadius;

// Clusters as arrays (cap entries each): box planes component-major (plane a of cluster i at box[a * cap + i]: lanes read
// consecutive dwords), the reference the cluster's parent will hold (>= 0 node id, < 0 ~sorted position), the number
// of primitives below and the height.
struct PlocClusters {
    float *box;
    int *ref;
    uint32_t *cnt;
    int *height;
};

__global__ __launch_bounds__(kPlocBlock) void k_ploc_init(const unsigned long long *__restrict__ keys, const float *__restrict__ lo,
                                                          const float *__restrict__ hi, uint32_t n, uint32_t cap, PlocClusters C)
{
    const uint32_t p = blockIdx.x * kPlocBlock + threadIdx.x;
    if (p >= n) return;
    const uint32_t prim = (uint32_t)(keys[p] & 0xFFFFFFFFull);
    if (prim >= n) return;                                  // (unreachable: a key's low half is a primitive index; a belt against reading past lo / hi)
    for (int a = 0; a < 3; a++) {
        C.box[(size_t)a * cap + p] = lo[3 * (size_t)prim + a];
        C.box[(size_t)(3 + a) * cap + p] = hi[3 * (size_t)prim + a];
    }
    C.ref[p] = ~(int)p;
    C.cnt[p] = 1u;
    C.height[p] = 0;
}

// The cost of merging two boxes: the surface of their union in cbox_area's order, every operation rounded (the build
// compiles with -ffp-contract=off); not finite (an unbounded primitive's +-3e38 box overflows on purpose) -> FLT_MAX.
__device__ __forceinline__ float merge_cost(const float a[6], float l0, float l1, float l2, float h0, float h1, float h2)
{
    const float dx = fmaxf(a[3], h0) - fminf(a[0], l0), dy = fmaxf(a[4], h1) - fminf(a[1], l1), dz = fmaxf(a[5], h2) - fminf(a[2], l2);
    const float s = (dx * dy + dy * dz) + dz * dx;
    return (f_bits(s) & 0x7F800000u) == 0x7F800000u ? FLT_MAX : s;
}

// 256 threads serve 256 consecutive clusters: the boxes of positions [base - R, base + 256 + R) go to LDS once (six float
// arrays: consecutive lanes, consecutive dwords), each thread evaluates its up to 2R neighbours from there.
__global__ __launch_bounds__(kPlocBlock) void k_ploc_nn(const float *__restrict__ box, uint32_t cap, uint32_t m, int R, int *__restrict__ nn)
{
    __shared__ float s[6][kPlocStage];
    const int base = (int)(blockIdx.x * kPlocBlock), first = base - R;
    for (int t = (int)threadIdx.x; t < kPlocBlock + 2 * R; t += kPlocBlock) {
        const int pos = first + t;
        if (pos >= 0 && pos < (int)m)
            for (int a = 0; a < 6; a++) s[a][t] = box[(size_t)a * cap + pos];
    }
    __syncthreads();
    const int i = base + (int)threadIdx.x;
    if (i >= (int)m) return;
    float me[6];
    for (int a = 0; a < 6; a++) me[a] = s[a][i - first];
    const int j0 = i - R > 0 ? i - R : 0, j1 = i + R < (int)m - 1 ? i + R : (int)m - 1;
    float bc = 0.0f;
    int bj = -1;
    for (int j = j0; j <= j1; j++) {
        if (j == i) continue;
        const int t = j - first;
        const float c = merge_cost(me, s[0][t], s[1][t], s[2][t], s[3][t], s[4][t], s[5][t]);
        if (bj < 0 || c < bc || (c == bc && (i ^ j) < (i ^ bj))) { bc = c; bj = j; }
    }
    nn[i] = bj;                                             // (m >= 2: there was a candidate)
}

// keep flag in the low half, made flag in the high half: one 64-bit scan gives both positions
__global__ __launch_bounds__(kPlocBlock) void k_ploc_mark(const int *__restrict__ nn, uint32_t m, unsigned long long *__restrict__ flags)
{
    const uint32_t i = blockIdx.x * kPlocBlock + threadIdx.x;
    if (i >= m) return;
    const uint32_t j = (uint32_t)nn[i];
    const bool mutual = j < m && (uint32_t)nn[j] == i;
    const unsigned long long keep = !(mutual && i > j), made = mutual && i < j;
    flags[i] = keep | (made << 32);
}

__global__ __launch_bounds__(kPlocBlock) void k_ploc_emit(PlocClusters in, const int *__restrict__ nn, const unsigned long long *__restrict__ flags,
                                                          const unsigned long long *__restrict__ scan, uint32_t m, uint32_t cap, uint32_t made_before,
                                                          uint32_t n, PlocClusters out, float *__restrict__ nodes, uint32_t *__restrict__ totals)
{
    const uint32_t i = blockIdx.x * kPlocBlock + threadIdx.x;
    if (i >= m) return;
    const unsigned long long f = flags[i], sc = scan[i];
    const uint32_t dst = (uint32_t)(sc & 0xFFFFFFFFull), k = (uint32_t)(sc >> 32);
    const bool keep = (f & 1ull) != 0ull, made = (f >> 32) != 0ull;
    if (i == m - 1u) { totals[0] = dst + (keep ? 1u : 0u); totals[1] = k + (made ? 1u : 0u); }
    if (!keep || dst >= m) return;                          // (dst >= m is unreachable: an exclusive sum of m flags; a belt for the stores below)
    float b[6];
    for (int a = 0; a < 6; a++) b[a] = in.box[(size_t)a * cap + i];
    int ref = in.ref[i], h = in.height[i];
    uint32_t cnt = in.cnt[i];
    if (made) {
        const uint32_t j = (uint32_t)nn[i];
        const long long id = (long long)n - 2 - ((long long)made_before + k);
        if (j >= m || id < 0) return;                       // (unreachable: k_ploc_mark saw j < m, and n - 1 merges are all there are; the host checks the totals)
        float o[6];
        for (int a = 0; a < 6; a++) o[a] = in.box[(size_t)a * cap + j];
        const int hj = in.height[j];
        float *nd = nodes + (size_t)id * kNodeFloats;
        for (int a = 0; a < 6; a++) { nd[a] = b[a]; nd[6 + a] = o[a]; }
        nd[12] = __int_as_float(ref); nd[13] = __int_as_float(in.ref[j]);
        nd[14] = __int_as_float((int)cnt);                  // primitives below child 0, for k_ploc_slots (which clears it)
        nd[15] = 0.0f;
        for (int a = 0; a < 3; a++) { b[a] = fminf(b[a], o[a]); b[3 + a] = fmaxf(b[3 + a], o[3 + a]); }
        ref = (int)id; cnt += in.cnt[j]; h = (h > hj ? h : hj) + 1;
    }
    for (int a = 0; a < 6; a++) out.box[(size_t)a * cap + dst] = b[a];
    out.ref[dst] = ref; out.cnt[dst] = cnt; out.height[dst] = h;
}

// The nodes [base, base + count) of one round, after the rounds that made their parents: first slot of each child, final
// leaf references, order[slot] = the key of the leaf's sorted position.
__global__ __launch_bounds__(kPlocBlock) void k_ploc_slots(float *__restrict__ nodes, uint32_t base, uint32_t count, uint32_t n, uint32_t *__restrict__ first,
                                                           const unsigned long long *__restrict__ keys, unsigned long long *__restrict__ order)
{
    const uint32_t t = blockIdx.x * kPlocBlock + threadIdx.x;
    if (t >= count || base + t >= n - 1u) return;           // (the second test and the range tests below are unreachable belts: the host hands over the rounds it counted)
    const uint32_t id = base + t;
    float *nd = nodes + (size_t)id * kNodeFloats;
    uint32_t f = first[id];
    const uint32_t cnt0 = (uint32_t)__float_as_int(nd[14]);
    for (int c = 0; c < 2; c++) {
        const int r = __float_as_int(nd[12 + c]);
        if (r >= 0) {
            if ((uint32_t)r < n - 1u) first[r] = f;
        } else {
            const uint32_t p = (uint32_t)~r;
            if (p < n && f < n) { order[f] = keys[p]; nd[12 + c] = __int_as_float(~(int)(f << 3)); }
        }
        f += cnt0;
    }
    nd[14] = 0.0f;
}

#define PL(call) do { e = (call); if (e != hipSuccess) return e; } while (0)

// The rounds and the slot pass over sorted keys and the boxes they index.  d_nodes2: (n - 1) x 16 floats; d_order: n keys,
// order[slot] = the key of the primitive in that slot.  info.abandoned != 0: nothing usable was written.
hipError_t ploc_core(const unsigned long long *d_sorted, const float *d_lo, const float *d_hi, uint32_t n, const PlocOptions &opt,
                     float *d_nodes2, unsigned long long *d_order, PlocInfo &info, hipStream_t stream)
{
    info = PlocInfo();
    const uint32_t cap = n;
    const int R = (int)std::min<uint32_t>(std::max<uint32_t>(opt.radius, 1u), (uint32_t)kPlocMaxRadius);
    DevBuf<float> d_box[2];
    DevBuf<int> d_ref[2], d_height[2], d_nn;
    DevBuf<uint32_t> d_cnt[2], d_first, d_totals;
    DevBuf<unsigned long long> d_flags, d_scan;
    DevBuf<char> d_tmp;
    hipError_t e;
    PlocClusters C[2];
    for (int b = 0; b < 2; b++) {
        PL(d_box[b].alloc((size_t)6 * cap)); PL(d_ref[b].alloc(cap)); PL(d_cnt[b].alloc(cap)); PL(d_height[b].alloc(cap));
        C[b] = PlocClusters{d_box[b].p, d_ref[b].p, d_cnt[b].p, d_height[b].p};
    }
    PL(d_nn.alloc(cap)); PL(d_flags.alloc(cap)); PL(d_scan.alloc(cap)); PL(d_first.alloc(n - 1)); PL(d_totals.alloc(2));
    size_t tmp_bytes = 0;
    PL(hipcub::DeviceScan::ExclusiveSum(nullptr, tmp_bytes, d_flags.p, d_scan.p, (int)cap, stream));
    PL(d_tmp.alloc(std::max<size_t>(tmp_bytes, 1)));
    const auto blocks = [](uint32_t k) { return dim3((k + kPlocBlock - 1u) / kPlocBlock); };
    hipLaunchKernelGGL(k_ploc_init, blocks(n), dim3(kPlocBlock), 0, stream, d_sorted, d_lo, d_hi, n, cap, C[0]);
    PL(hipGetLastError());
    std::vector<std::pair<uint32_t, uint32_t>> rounds;      // (first node id, nodes) made per round
    uint32_t m = n, made = 0;
    int cur = 0;
    while (m > 1) {
        if (rounds.size() >= opt.max_rounds) { info.abandoned = 2; info.rounds = (uint32_t)rounds.size(); return hipSuccess; }
        hipLaunchKernelGGL(k_ploc_nn, blocks(m), dim3(kPlocBlock), 0, stream, (const float *)C[cur].box, cap, m, R, d_nn.p);
        PL(hipGetLastError());
        hipLaunchKernelGGL(k_ploc_mark, blocks(m), dim3(kPlocBlock), 0, stream, (const int *)d_nn.p, m, d_flags.p);
        PL(hipGetLastError());
        PL(hipcub::DeviceScan::ExclusiveSum(d_tmp.p, tmp_bytes, d_flags.p, d_scan.p, (int)m, stream));
        hipLaunchKernelGGL(k_ploc_emit, blocks(m), dim3(kPlocBlock), 0, stream, C[cur], (const int *)d_nn.p, (const unsigned long long *)d_flags.p,
                           (const unsigned long long *)d_scan.p, m, cap, made, n, C[cur ^ 1], d_nodes2, d_totals.p);
        PL(hipGetLastError());
        uint32_t tot[2] = {0, 0};
        PL(hipMemcpyAsync(tot, d_totals.p, sizeof tot, hipMemcpyDeviceToHost, stream));
        PL(hipStreamSynchronize(stream));
        if (tot[1] == 0 || tot[0] + tot[1] != m || made + tot[1] > n - 1) return hipErrorUnknown;   // (every round merges at least one pair)
        made += tot[1];
        rounds.emplace_back(n - 1 - made, tot[1]);
        m = tot[0];
        cur ^= 1;
    }
    info.rounds = (uint32_t)rounds.size();
    int depth = 0;
    PL(hipMemcpyAsync(&depth, C[cur].height, sizeof depth, hipMemcpyDeviceToHost, stream));
    PL(hipStreamSynchronize(stream));
    info.depth = (uint32_t)depth;
    if (made != n - 1) return hipErrorUnknown;
    if (info.depth > opt.max_depth) { info.abandoned = 1; return hipSuccess; }
    PL(hipMemsetAsync(d_first.p, 0, (size_t)(n - 1) * 4, stream));
    PL(hipMemsetAsync(d_order, 0, (size_t)n * 8, stream));     // (every slot is written below; the gather indexes records by these)
    for (size_t r = rounds.size(); r-- > 0;) {               // parents are made in later rounds than their children
        hipLaunchKernelGGL(k_ploc_slots, blocks(rounds[r].second), dim3(kPlocBlock), 0, stream, d_nodes2, rounds[r].first, rounds[r].second, n,
                           d_first.p, d_sorted, d_order);
        PL(hipGetLastError());
    }
    return hipStreamSynchronize(stream);                    // (the temporaries go with this scope)
}

}  // namespace

// lo/hi: n x 3 floats on the host, as build_lbvh takes them.  Needs n >= 2.  info.abandoned != 0: `out` is empty.
hipError_t build_ploc(const float *lo, const float *hi, uint32_t n, const PlocOptions &opt, Bvh &out, PlocInfo &info, hipStream_t stream)
{
    out = Bvh();
    info = PlocInfo();
    if (n < 2) return hipErrorInvalidValue;
    DevBuf<float> d_lo, d_hi, d_nodes;
    DevBuf<unsigned long long> d_keys, d_sorted, d_order;
    DevBuf<char> d_tmp;
    hipError_t e;
    PL(d_lo.alloc((size_t)n * 3)); PL(d_hi.alloc((size_t)n * 3));
    PL(d_keys.alloc(n)); PL(d_sorted.alloc(n)); PL(d_order.alloc(n));
    PL(d_nodes.alloc((size_t)(n - 1) * kNodeFloats));
    PL(lbvh_sorted_keys_host(lo, hi, n, d_lo.p, d_hi.p, d_keys.p, d_sorted.p, d_tmp, stream));
    PL(ploc_core(d_sorted.p, d_lo.p, d_hi.p, n, opt, d_nodes.p, d_order.p, info, stream));
    if (info.abandoned) return hipSuccess;
    out.nodes.resize((size_t)(n - 1) * kNodeFloats);
    std::vector<unsigned long long> keys(n);
    PL(hipMemcpyAsync(out.nodes.data(), d_nodes.p, out.nodes.size() * sizeof(float), hipMemcpyDeviceToHost, stream));
    PL(hipMemcpyAsync(keys.data(), d_order.p, (size_t)n * 8, hipMemcpyDeviceToHost, stream));
    PL(hipStreamSynchronize(stream));
    out.order.resize(n);
    for (size_t s = 0; s < n; s++) out.order[s] = (uint32_t)(keys[s] & 0xFFFFFFFFull);
    out.root = 0;
    out.n_inner = n - 1;
    out.n_leaves = n;
    out.max_depth = info.depth;
    return hipSuccess;
}

// The whole build on the device, build_lbvh_device's contract: bounds from the 80-byte records, keys, sort, the rounds, the
// slots, the leaf-ordered records, then the collapse to the quantised 4-wide tree from node 0.
hipError_t build_ploc_device(const unsigned char *d_raw, uint32_t n, float hit_pad, const PlocOptions &opt, float4 *d_prim, float4 *d_primD,
                             uint32_t *d_slot_of_index, float *d_nodes2, uint4 *d_nodes4q, LbvhDeviceResult &res, PlocInfo &info,
                             hipStream_t stream)
{
    res = LbvhDeviceResult();
    info = PlocInfo();
    if (n < 2) return hipErrorInvalidValue;
    DevBuf<float> d_lo, d_hi;
    DevBuf<unsigned long long> d_keys, d_sorted, d_order;
    DevBuf<uint32_t> d_cbox;
    DevBuf<char> d_tmp;
    hipError_t e;
    PL(d_lo.alloc((size_t)n * 3)); PL(d_hi.alloc((size_t)n * 3));
    PL(d_keys.alloc(n)); PL(d_sorted.alloc(n)); PL(d_order.alloc(n)); PL(d_cbox.alloc(8));
    PL(lbvh_sorted_keys_device(d_raw, n, hit_pad, d_lo.p, d_hi.p, d_cbox.p, d_keys.p, d_sorted.p, d_tmp, stream));
    PL(ploc_core(d_sorted.p, d_lo.p, d_hi.p, n, opt, d_nodes2, d_order.p, info, stream));
    if (info.abandoned) return hipSuccess;
    PL(lbvh_launch_gather(d_raw, d_order.p, n, d_prim, d_primD, d_slot_of_index, stream));
    res.max_depth = info.depth;
    return lbvh_collapse_device(d_nodes2, n, d_nodes4q, res, stream);
}
#undef PL

}  // namespace crt
