// crt_query.hip -- ray queries (include/crt.h, crt_query_rays / crt_query_rays_device / crt_pick): "here are my rays,
// what do they hit?".  One lane per ray through the single-ray walks k_wf_finish uses (crt_shade.h), the winner's
// attributes and surface coordinates recomputed from its record after the walk.  The kernel reads the scene, the tree
// and the id table and writes the caller's planes: nothing of the path tracer's state is involved.  DESIGN.md 6p has the
// definition this follows (tests/query_ref.py is its restatement).
#include "crt_launch.h"
#include "crt_shade.h"

namespace crt {

// grid = ceil(n / 64) blocks of 64 threads, lane -> ray: k_debug_walk_rays' layout and LDS stack (kStackDepth x 64
// entries, lane i on column i).  MODE: CRT_QUERY_CLOSEST or CRT_QUERY_ANY (which stores `hit` alone and carries no
// attribute code).  PICK: the ray is the G-buffer's ray of pixel xy[i], generated here.  BRUTE: CRT_ACCEL_NONE, the
// reference's loop in line (as k_aov: a call of intersect_all puts the scene into scratch).  A lane touches its own ray
// and its own outputs only: no atomics, no barrier, no cross-lane step.
template <int MODE, bool PICK, bool BRUTE>
__global__ __launch_bounds__(64) void k_query(const DevScene S, const QueryParams P)
{
    __shared__ int lds_stack[BRUTE ? 64 : kStackDepth * 64];
    const size_t i = (size_t)blockIdx.x * 64u + threadIdx.x;
    if (i >= P.n) return;
    int *stk = lds_stack + threadIdx.x;
    f3 o, d;
    float t_max;
    uint32_t excl;
    if (PICK) {
        const uint2 p = P.xy[i];
        Rng rng;
        primary_ray(S, p.x, p.y, kDnSample, tea(p.x, p.y * 100u), rng, o, d);
        t_max = CRT_INFINITY;
        excl = 0xFFFFFFFFu;
    } else {
        const float4 r0 = P.rays[2 * i], r1 = P.rays[2 * i + 1];
        o = f3{r0.x, r0.y, r0.z}; d = f3{r1.x, r1.y, r1.z};
        t_max = r0.w;
        excl = f_bits(r1.w);
    }
    uint32_t b_index = kNoHit, b_slot = kNoHit, cn = 0, cp = 0;
    // a non-finite ray is a miss and costs nothing (not the loop over every primitive the G-buffer gives it); a NaN or
    // negative limit can never be beaten -- the literal test of the loop below would let a NaN limit through
    if (finite3(o) && finite3(d) && t_max >= 0.0f) {
        if (BRUTE) {
            for (uint32_t k = 0; k < S.nprim; k++) {
                hit_test<true>(S, S.slot_of_index[k], o, d, excl, 0.001f, t_max, b_index, b_slot);
                if (MODE == CRT_QUERY_ANY && b_slot != kNoHit) break;
            }
        } else {
            const bool wide = P.wide_ok && finish_walks_wide(S);
            if (MODE == CRT_QUERY_ANY) {
                // finish_walk_extension's pattern with anyhit and nothing primed: the first accepted primitive ends the walk
                if (!wide || !traverse4q<false>(S, stk, o, d, excl, true, t_max, b_index, b_slot, cn, cp))
                    traverse<false>(S, stk, o, d, excl, true, t_max, b_index, b_slot, cn, cp);
            } else {
                uint32_t how;
                finish_walk_extension<false>(S, stk, wide, o, d, excl, t_max, b_index, b_slot, cn, cp, how);
            }
        }
    }
    const bool hit = b_slot != kNoHit;
    if (P.hit) P.hit[i] = hit ? 1u : 0u;
    if (MODE == CRT_QUERY_ANY) return;
    if (P.prim) P.prim[i] = hit ? b_index : kNoHit;
    if (P.id) P.id[i] = hit ? P.table[b_index] : kNoHit;
    if (P.t) P.t[i] = t_max;                                     // (a miss: the ray's own limit, untouched)
    if (!P.position && !P.normal && !P.uv) return;
    f3 pos = f3{0, 0, 0}, nrm = f3{0, 0, 0};
    float u = 0.0f, v = 0.0f;
    if (hit) {
        const float4 A = S.prim[3 * b_slot + 0], B = S.prim[3 * b_slot + 1], C = S.prim[3 * b_slot + 2];
        float4 D = float4{0.0f, 0.0f, 0.0f, 0.0f};
        if ((f_bits(A.w) & 3u) == 0u) D = S.primD[b_slot];
        uint32_t meta;
        hit_attributes_rec(A, B, C, D, o, d, t_max, pos, nrm, meta);
        if (P.uv) hit_uv_rec(A, B, C, D, o, d, t_max, u, v);
    }
    if (P.position) P.position[i] = float4{pos.x, pos.y, pos.z, 0.0f};
    if (P.normal) P.normal[i] = float4{nrm.x, nrm.y, nrm.z, 0.0f};
    if (P.uv) P.uv[i] = float2{u, v};
}

template <int MODE, bool PICK>
static void query_launch_as(const DevScene &S, const QueryParams &P, bool brute, dim3 grid, hipStream_t stream)
{
    if (brute) hipLaunchKernelGGL((k_query<MODE, PICK, true>), grid, dim3(64), 0, stream, S, P);
    else hipLaunchKernelGGL((k_query<MODE, PICK, false>), grid, dim3(64), 0, stream, S, P);
}

hipError_t query_launch(const DevScene &S, const QueryParams &P, int mode, bool pick, bool brute, hipStream_t stream)
{
    if (P.n == 0) return hipSuccess;
    if (P.n > 0xFFFFFFFFull || (mode != CRT_QUERY_CLOSEST && mode != CRT_QUERY_ANY) || (pick && mode != CRT_QUERY_CLOSEST))
        return hipErrorInvalidValue;
    const dim3 grid((unsigned)((P.n + 63) / 64));
    if (pick) query_launch_as<CRT_QUERY_CLOSEST, true>(S, P, brute, grid, stream);
    else if (mode == CRT_QUERY_ANY) query_launch_as<CRT_QUERY_ANY, false>(S, P, brute, grid, stream);
    else query_launch_as<CRT_QUERY_CLOSEST, false>(S, P, brute, grid, stream);
    return hipGetLastError();
}

}  // namespace crt
