// crt_refit.hip -- edits of a built scene (include/crt.h "Scene edits"): the scene scale behind hit_pad, the leaf-ordered
// records of edited primitives, and the refit of a tree whose topology is kept and whose boxes are recomputed from the
// current primitives.  The bound rule and the record gather are crt_prim.h's, shared with the LBVH build.
//
//   k_refit_pad       max |corner coordinate| over the primitives, as scene_hit_pad computes it (NaN ignored, inf kept)
//   k_refit_prims     48-byte records + D of primitives [first, first+count) into their slots (slot_of_index)
//   k_refit_transform every op of one crt_transform_primitives call: the 80-byte records moved where they lie, and their
//                     48-byte records + D in the same thread
//   k_edit_compact    crt_remove_primitives: the surviving 80-byte records into a fresh array, renumbered
//   k_refit_expand    once per tree: the inner nodes level by level from the root (one launch per level), so that a
//                     refit can walk the levels bottom-up
//   k_refit_bvh2      one launch per BVH2 level, deepest first: each node's two child boxes, from the leaf's primitives
//                     or from the union of the child node's own two boxes (written by the previous launch)
//   k_refit_wide      the same over the 4-wide tree, with float boxes (32 floats per node: the float tree itself, or
//                     scratch for the quantised one)
//   k_refit_quant4    re-quantises every 4-wide node's child planes from the float boxes against a new grid
//
// The kernel boundary between two levels is the only ordering the refit needs: no flags, atomics or fences (a
// bottom-up climb with an arrival counter per node, as k_lbvh_bounds builds, spent most of its time in the fences:
// DESIGN.md 6b).  Empty child slots of a wide node have reference 0 (the root is nobody's child, leaves are negative).
#include <hip/hip_runtime.h>

#include <vector>

#include "../../include/crt.h"
#include "crt_bvh.h"
#include "crt_launch.h"
#include "crt_math.h"
#include "crt_prim.h"

namespace crt {
namespace {

// Union of the bounds of the leaf's primitives (leaf-ordered records: A.w holds the category in its low bits).
__device__ __forceinline__ void leaf_box(const float4 *__restrict__ prim, uint32_t first, uint32_t count, float pad, float b[6])
{
    for (uint32_t k = 0; k < count; k++) {
        const float4 A = prim[3 * (size_t)(first + k) + 0], B = prim[3 * (size_t)(first + k) + 1], C = prim[3 * (size_t)(first + k) + 2];
        float l[3], h[3];
        prim_bounds(f_bits(A.w) & 3u, f3{A.x, A.y, A.z}, f3{B.x, B.y, B.z}, f3{C.x, C.y, C.z}, pad, l, h);
        for (int a = 0; a < 3; a++) {
            b[a] = k ? fminf(b[a], l[a]) : l[a];
            b[3 + a] = k ? fmaxf(b[3 + a], h[a]) : h[a];
        }
    }
}

__global__ __launch_bounds__(256) void k_refit_pad(const unsigned char *__restrict__ raw, uint32_t n, uint32_t *__restrict__ out)
{
    const uint32_t i = blockIdx.x * 256u + threadIdx.x;
    float S = 0.0f;
    if (i < n) {
        const RawPrim p = load_raw(raw, i);
        f3 c[4];
        int nc;
        if (p.category == 1u) {                                   // prim_corners (crt_api.cpp), op for op
            const float r = abs_(p.d2.x);
            c[0] = f3{p.d1.x - r, p.d1.y - r, p.d1.z - r}; c[1] = f3{p.d1.x + r, p.d1.y + r, p.d1.z + r}; nc = 2;
        } else {
            c[0] = p.d1; c[1] = p.d1 + p.d2; c[2] = p.d1 + p.d3; nc = 3;
            if (p.category == 0u) { c[3] = c[1] + p.d3; nc = 4; }
        }
        for (int k = 0; k < nc; k++) { S = max_(S, abs_(c[k].x)); S = max_(S, abs_(c[k].y)); S = max_(S, abs_(c[k].z)); }
    }
    // S >= 0 and never NaN (max_ keeps S against a NaN): as bits, the order of non-negative floats, inf included
    uint32_t u = f_bits(S);
    for (int off = 32; off > 0; off >>= 1) { const uint32_t o = (uint32_t)__shfl_xor((int)u, off, 64); u = o > u ? o : u; }
    if ((threadIdx.x & 63u) == 0u) atomicMax(out, u);
}

__global__ __launch_bounds__(256) void k_refit_prims(const unsigned char *__restrict__ raw, uint32_t first, uint32_t count,
                                                     const uint32_t *__restrict__ slot_of_index, float4 *__restrict__ prim,
                                                     float4 *__restrict__ primD)
{
    const uint32_t k = blockIdx.x * 256u + threadIdx.x;
    if (k >= count) return;
    const RawPrim p = load_raw(raw, (size_t)first + k);
    float4 A, B, C, D;
    prim_record(p, A, B, C, D);
    const uint32_t slot = slot_of_index[first + k];
    prim[3 * (size_t)slot + 0] = A; prim[3 * (size_t)slot + 1] = B; prim[3 * (size_t)slot + 2] = C;
    primD[slot] = D;
}

// crt_transform_primitives (include/crt.h pins the arithmetic: every product and sum rounded, in this order).
__device__ __forceinline__ f3 xf_vector(const float *__restrict__ m, f3 v)
{
    return f3{__fadd_rn(__fadd_rn(__fmul_rn(m[0], v.x), __fmul_rn(m[1], v.y)), __fmul_rn(m[2], v.z)),
              __fadd_rn(__fadd_rn(__fmul_rn(m[4], v.x), __fmul_rn(m[5], v.y)), __fmul_rn(m[6], v.z)),
              __fadd_rn(__fadd_rn(__fmul_rn(m[8], v.x), __fmul_rn(m[9], v.y)), __fmul_rn(m[10], v.z))};
}
__device__ __forceinline__ f3 xf_point(const float *__restrict__ m, f3 p)
{
    const f3 v = xf_vector(m, p);
    return f3{__fadd_rn(v.x, m[3]), __fadd_rn(v.y, m[7]), __fadd_rn(v.z, m[11])};
}

// Thread t of the concatenated ranges: its op is the last one whose start (prefix sum of the counts; start[n_ops] =
// total, no op empty) is <= t.  Only the nine (spheres: four) geometry floats of the 80-byte record are stored, so every
// other byte stays as it was; prim / primD may be null (no structure built yet: the build makes them).
__global__ __launch_bounds__(256) void k_refit_transform(unsigned char *raw, const uint32_t *__restrict__ start, const crt_prim_transform *__restrict__ ops,
                                                         uint32_t n_ops, uint32_t total, const uint32_t *__restrict__ slot_of_index,
                                                         float4 *__restrict__ prim, float4 *__restrict__ primD)
{
    const uint32_t t = blockIdx.x * 256u + threadIdx.x;
    if (t >= total) return;
    uint32_t lo = 0, hi = n_ops;                                 // start[lo] <= t < start[hi]
    while (hi - lo > 1u) {
        const uint32_t mid = (lo + hi) >> 1;
        if (start[mid] <= t) lo = mid; else hi = mid;
    }
    const crt_prim_transform &op = ops[lo];                     // (include/crt.h: first, count, m[12], radius_scale)
    const size_t i = (size_t)op.first + (t - start[lo]);
    RawPrim p = load_raw(raw, i);
    float *rec = (float *)(raw + i * 80);
    p.d1 = xf_point(op.m, p.d1);
    rec[4] = p.d1.x; rec[5] = p.d1.y; rec[6] = p.d1.z;
    if (p.category == 1u) {
        p.d2.x = __fmul_rn(p.d2.x, op.radius_scale);
        rec[8] = p.d2.x;
    } else {
        p.d2 = xf_vector(op.m, p.d2);
        p.d3 = xf_vector(op.m, p.d3);
        rec[8] = p.d2.x; rec[9] = p.d2.y; rec[10] = p.d2.z;
        rec[12] = p.d3.x; rec[13] = p.d3.y; rec[14] = p.d3.z;
    }
    if (!prim) return;
    float4 A, B, C, D;
    prim_record(p, A, B, C, D);
    const uint32_t slot = slot_of_index[i];
    prim[3 * (size_t)slot + 0] = A; prim[3 * (size_t)slot + 1] = B; prim[3 * (size_t)slot + 2] = C;
    primD[slot] = D;
}

// crt_remove_primitives: the surviving records, in their order, into a fresh array (out of place: a record's new home
// may be another survivor's old one).  One thread per 16 bytes of the new array, five per record, so the reads within a
// run of survivors and all the writes are whole coalesced 16-byte accesses.  gap[k] (ascending; touching ranges give
// equal entries) is the new index before which removed range k fell, cum[k] the primitives the first k ranges removed
// (cum[0] = 0): new record j was old record j + cum[r], r = the number of gaps <= j.  Chunk 4 is data4, whose .w is the
// record's position.  No atomics, no LDS; the same launch parameters serve d_raw and the history's snapshot of it.
__global__ __launch_bounds__(256) void k_edit_compact(const uint4 *__restrict__ src, uint4 *__restrict__ dst, const uint32_t *__restrict__ gap,
                                                      const uint32_t *__restrict__ cum, uint32_t n_gaps, uint32_t n_new)
{
    const size_t t = (size_t)blockIdx.x * 256u + threadIdx.x;
    if (t >= (size_t)n_new * 5u) return;
    const uint32_t j = (uint32_t)(t / 5u), chunk = (uint32_t)(t - (size_t)j * 5u);
    uint32_t lo = 0, hi = n_gaps;                                // gap[k] <= j for k < lo, gap[k] > j for k >= hi
    while (lo < hi) {
        const uint32_t mid = (lo + hi) >> 1;
        if (gap[mid] <= j) lo = mid + 1; else hi = mid;
    }
    uint4 v = src[((size_t)j + cum[lo]) * 5u + chunk];
    if (chunk == 4u) v.w = j;
    dst[t] = v;
}

// One level of the walk from the root: the inner children of the nodes in `in` are appended to `out` (at most cap
// entries).  Refs are dwords ref_at.. of a node of `stride` dwords (BVH2: 16 / 12, float 4-wide: 32 / 24, quantised
// 4-wide: 16 / 12); width 2 has no empty slots, width 4 marks them with 0.  nch (width 4): the node's children.
__global__ __launch_bounds__(256) void k_refit_expand(const uint32_t *__restrict__ nodes, uint32_t stride, uint32_t ref_at, uint32_t width,
                                                      const int *__restrict__ in, uint32_t count, int *__restrict__ out, uint32_t cap,
                                                      uint32_t *__restrict__ out_count, uint32_t *__restrict__ nch)
{
    const uint32_t t = blockIdx.x * 256u + threadIdx.x;
    if (t >= count) return;
    const int node = in[t];
    int inner[4];
    uint32_t k = 0, m = 0;
    for (uint32_t c = 0; c < width; c++) {
        const int ref = (int)nodes[(size_t)node * stride + ref_at + c];
        if (width == 4 && ref == 0) continue;
        m++;
        if (ref >= 0) inner[k++] = ref;
    }
    if (nch) nch[node] = m;
    if (!k) return;
    const uint32_t pos = atomicAdd(out_count, k);
    for (uint32_t j = 0; j < k; j++)
        if (pos + j < cap) out[pos + j] = inner[j];
}

// One BVH2 level: both child boxes of every listed node (crt_bvh.h record: c0.lo c0.hi c1.lo c1.hi refs).
__global__ __launch_bounds__(256) void k_refit_bvh2(const float4 *__restrict__ prim, float pad, const int *__restrict__ list, uint32_t count,
                                                    float *__restrict__ nodes)
{
    const uint32_t t = blockIdx.x * 256u + threadIdx.x;
    if (t >= count) return;
    float *nd = nodes + (size_t)list[t] * kNodeFloats;
    for (int c = 0; c < 2; c++) {
        const int ref = (int)f_bits(nd[12 + c]);
        float b[6];
        if (ref < 0) {
            leaf_box(prim, (uint32_t)(~ref) >> 3, ((uint32_t)(~ref) & 7u) + 1u, pad, b);
        } else {
            const float4 *ch = (const float4 *)(nodes + (size_t)ref * kNodeFloats);
            const float4 q0 = ch[0], q1 = ch[1], q2 = ch[2];        // c0.lo c0.hi | c1.lo c1.hi
            b[0] = fminf(q0.x, q1.z); b[1] = fminf(q0.y, q1.w); b[2] = fminf(q0.z, q2.x);
            b[3] = fmaxf(q0.w, q2.y); b[4] = fmaxf(q1.x, q2.z); b[5] = fmaxf(q1.y, q2.w);
        }
        for (int a = 0; a < 6; a++) nd[6 * c + a] = b[a];
    }
}

// One level of the 4-wide tree in the float layout of crt_bvh.h (32 floats per node: lo.x[4] lo.y[4] lo.z[4] hi.x[4]
// hi.y[4] hi.z[4] refs[4] -); `refs` holds the child references (stride / ref_at as for k_refit_expand).
__global__ __launch_bounds__(256) void k_refit_wide(const float4 *__restrict__ prim, float pad, const int *__restrict__ list, uint32_t count,
                                                    const uint32_t *__restrict__ refs, uint32_t stride, uint32_t ref_at,
                                                    const uint32_t *__restrict__ nch, float *__restrict__ fb)
{
    const uint32_t t = blockIdx.x * 256u + threadIdx.x;
    if (t >= count) return;
    const int node = list[t];
    float *nd = fb + (size_t)node * kNode4Floats;
    for (uint32_t c = 0; c < 4; c++) {
        const int ref = (int)refs[(size_t)node * stride + ref_at + c];
        if (ref == 0) continue;                                  // empty slot: stays as the build left it
        float b[6];
        if (ref < 0) {
            leaf_box(prim, (uint32_t)(~ref) >> 3, ((uint32_t)(~ref) & 7u) + 1u, pad, b);
        } else {
            const float *ch = fb + (size_t)ref * kNode4Floats;
            const uint32_t k = nch[ref];
            for (int a = 0; a < 6; a++) b[a] = ch[4 * a];
            for (uint32_t i = 1; i < k; i++)
                for (int a = 0; a < 3; a++) { b[a] = fminf(b[a], ch[4 * a + i]); b[3 + a] = fmaxf(b[3 + a], ch[12 + 4 * a + i]); }
        }
        for (int a = 0; a < 6; a++) nd[4 * a + c] = b[a];
    }
}

// quantize_bvh4's plane rule (k_lbvh_collapse_level's arithmetic): floor / ceil in double, one grid unit of slack,
// clamped to 16 bits.  Empty slots keep lo = 65535, hi = 0; the references are not touched.
__global__ __launch_bounds__(256) void k_refit_quant4(const float *__restrict__ fb, const uint32_t *__restrict__ nch, uint32_t n4,
                                                      uint4 *__restrict__ nodes4q, double bx, double by, double bz, double sx, double sy, double sz)
{
    const uint32_t t = blockIdx.x * 256u + threadIdx.x;
    if (t >= n4) return;
    const float *nd = fb + (size_t)t * kNode4Floats;
    const uint32_t n = nch[t];
    const double base[3] = {bx, by, bz}, scale[3] = {sx, sy, sz};
    uint32_t q[24];
    for (int i = 0; i < 4; i++)
        for (int a = 0; a < 3; a++) {
            if ((uint32_t)i >= n) { q[4 * a + i] = 65535u; q[12 + 4 * a + i] = 0u; continue; }
            const double l = ((double)nd[4 * a + i] - base[a]) / scale[a], h = ((double)nd[12 + 4 * a + i] - base[a]) / scale[a];
            long long ql = (long long)floor(l) - 1, qh = (long long)ceil(h) + 1;
            ql = ql < 0 ? 0 : (ql > 65535 ? 65535 : ql); qh = qh < 0 ? 0 : (qh > 65535 ? 65535 : qh);
            q[4 * a + i] = (uint32_t)ql; q[12 + 4 * a + i] = (uint32_t)qh;
        }
    uint4 *o = nodes4q + 4 * (size_t)t;
    o[0] = uint4{q[0] | (q[1] << 16), q[2] | (q[3] << 16), q[4] | (q[5] << 16), q[6] | (q[7] << 16)};
    o[1] = uint4{q[8] | (q[9] << 16), q[10] | (q[11] << 16), q[12] | (q[13] << 16), q[14] | (q[15] << 16)};
    o[2] = uint4{q[16] | (q[17] << 16), q[18] | (q[19] << 16), q[20] | (q[21] << 16), q[22] | (q[23] << 16)};
}

inline unsigned blocks_of(size_t n) { return (unsigned)((n + 255u) / 256u); }

}  // namespace

hipError_t refit_launch_pad(const unsigned char *raw, uint32_t n, uint32_t *out, hipStream_t s)
{
    hipError_t e = hipMemsetAsync(out, 0, 4, s);
    if (e != hipSuccess || n == 0) return e;
    hipLaunchKernelGGL(k_refit_pad, dim3(blocks_of(n)), dim3(256), 0, s, raw, n, out);
    return hipGetLastError();
}

hipError_t refit_launch_prims(const unsigned char *raw, uint32_t first, uint32_t count, const uint32_t *slot_of_index, float4 *prim,
                              float4 *primD, hipStream_t s)
{
    if (count == 0) return hipSuccess;
    hipLaunchKernelGGL(k_refit_prims, dim3(blocks_of(count)), dim3(256), 0, s, raw, first, count, slot_of_index, prim, primD);
    return hipGetLastError();
}

// start: n_ops + 1 prefix sums (start[n_ops] = total), ops: n_ops records, both on the device; no op is empty.
hipError_t refit_launch_transform(unsigned char *raw, const uint32_t *start, const crt_prim_transform *ops, uint32_t n_ops, uint32_t total,
                                  const uint32_t *slot_of_index, float4 *prim, float4 *primD, hipStream_t s)
{
    if (total == 0) return hipSuccess;
    hipLaunchKernelGGL(k_refit_transform, dim3(blocks_of(total)), dim3(256), 0, s, raw, start, ops, n_ops, total, slot_of_index, prim, primD);
    return hipGetLastError();
}

// tab: n_gaps gaps, then n_gaps + 1 prefix sums, on the device; src holds n_new + tab[2 * n_gaps] records, dst n_new.
hipError_t refit_launch_compact(const unsigned char *src, unsigned char *dst, const uint32_t *tab, uint32_t n_gaps, uint32_t n_new, hipStream_t s)
{
    if (n_new == 0) return hipSuccess;
    hipLaunchKernelGGL(k_edit_compact, dim3(blocks_of((size_t)n_new * 5u)), dim3(256), 0, s, (const uint4 *)src, (uint4 *)dst, tab, tab + n_gaps,
                       n_gaps, n_new);
    return hipGetLastError();
}

// The inner nodes of a tree level by level from `root` into list (cap entries); off receives the level boundaries
// (level l = list[off[l] .. off[l+1])).  Once per tree: one launch and one readback per level.  Trees: width 2 = the BVH2
// (16-float nodes), width 4 = the 4-wide tree, quantised (16 dwords) or float (32 floats); nch: children per node (width 4).
hipError_t refit_levels(const void *nodes, uint32_t width, bool quantised, int root, uint32_t cap, int *list, uint32_t *counter,
                        uint32_t *nch, std::vector<uint32_t> &off, hipStream_t s)
{
    off.assign(1, 0u);
    if (root < 0 || cap == 0) return hipSuccess;
    const uint32_t stride = (width == 2 || quantised) ? 16u : 32u, ref_at = (width == 2 || quantised) ? 12u : 24u;
    hipError_t e = hipMemcpyAsync(list, &root, 4, hipMemcpyHostToDevice, s);
    uint32_t count = 1;
    while (e == hipSuccess && count) {
        const uint32_t base = off.back();
        off.push_back(base + count);
        if (off.size() > 130) return hipErrorUnknown;                       // deeper than any tree the builders make
        e = hipMemsetAsync(counter, 0, 4, s);
        if (e != hipSuccess) break;
        hipLaunchKernelGGL(k_refit_expand, dim3(blocks_of(count)), dim3(256), 0, s, (const uint32_t *)nodes, stride, ref_at, width,
                           list + base, count, list + base + count, cap - (base + count), counter, nch);
        e = hipGetLastError();
        uint32_t next = 0;
        if (e == hipSuccess) e = hipMemcpyAsync(&next, counter, 4, hipMemcpyDeviceToHost, s);
        if (e == hipSuccess) e = hipStreamSynchronize(s);
        if (e == hipSuccess && next > cap - (base + count)) return hipErrorUnknown;   // not a tree
        count = next;
    }
    return e;
}

hipError_t refit_launch_bvh2(const float4 *prim, float pad, const int *list, const std::vector<uint32_t> &off, float *nodes, hipStream_t s)
{
    for (size_t l = off.size() - 1; l-- > 0;) {
        const uint32_t count = off[l + 1] - off[l];
        hipLaunchKernelGGL(k_refit_bvh2, dim3(blocks_of(count)), dim3(256), 0, s, prim, pad, list + off[l], count, nodes);
        const hipError_t e = hipGetLastError();
        if (e != hipSuccess) return e;
    }
    return hipSuccess;
}

// refs: the tree's own nodes (quantised or float); fb: n4 x 32 floats (the float tree itself when there is one)
hipError_t refit_launch_wide(const float4 *prim, float pad, const int *list, const std::vector<uint32_t> &off, const void *refs,
                             bool quantised, const uint32_t *nch, float *fb, hipStream_t s)
{
    for (size_t l = off.size() - 1; l-- > 0;) {
        const uint32_t count = off[l + 1] - off[l];
        hipLaunchKernelGGL(k_refit_wide, dim3(blocks_of(count)), dim3(256), 0, s, prim, pad, list + off[l], count, (const uint32_t *)refs,
                           quantised ? 16u : 32u, quantised ? 12u : 24u, nch, fb);
        const hipError_t e = hipGetLastError();
        if (e != hipSuccess) return e;
    }
    return hipSuccess;
}

hipError_t refit_launch_quant4(const float *fb, const uint32_t *nch, uint32_t n4, uint4 *nodes4q, const double base[3], const double scale[3],
                               hipStream_t s)
{
    if (n4 == 0) return hipSuccess;
    hipLaunchKernelGGL(k_refit_quant4, dim3(blocks_of(n4)), dim3(256), 0, s, fb, nch, n4, nodes4q, base[0], base[1], base[2], scale[0],
                       scale[1], scale[2]);
    return hipGetLastError();
}

}  // namespace crt
