// crt_denoise.hip -- the denoised preview (include/crt.h, crt_denoise): a first-hit G-buffer and an edge-aware
// a-trous wavelet filter (Dammertz et al. 2010) over the accumulator's average.  It only READS the accumulator:
// the bit-exact image and everything that produces it are untouched.  DESIGN.md "Denoised preview" has the
// definition this follows operation by operation (tests/denoise_ref.py is its numpy restatement).
//
// crt_denoise_adaptive is the same filter for the adaptive state: per-tile counts, and a colour weight
// scaled by the pixels' own variance (k_dn_prepare_as, k_dn_vblur, k_dn_atrous_as below).
#include <algorithm>
#include <type_traits>

#include "crt_adaptive.h"
#include "crt_launch.h"
#include "crt_shade.h"

namespace crt {

// Per tile pixel: gbuf[2p] = (t, position), gbuf[2p+1] = (normal, hit index bits) -- crt_debug_intersect's record,
// so the readback is a copy -- and key[p] = material << 24 | reflectance index (kNoHit: the ray left the scene).
struct DnParams {
    const float4 *c_in;         // linear rgb (w unused) of the previous iteration
    float4 *c_out;              // ... of this one (w = 0)
    const float4 *gbuf;
    const uint32_t *key;
    uchar4 *rgba;               // null, or the rgba8 of c_out (last iteration)
    uint32_t tw, th, step;      // step = 2^i
    float inv_c;                // 2^i / sigma_color^2
    float inv_n;                // 1 / sigma_normal^2
    float inv_x;                // 1 / sigma_plane
};

// The primary ray of sample kDnSample (crt_device.h) of each pixel.
// grid = tiles_x * tiles_y blocks of 64 threads, block -> 8x8 pixel tile (spatially coherent rays, like k_trace).
__global__ __launch_bounds__(64) void k_dn_gbuffer(const DevScene S, uint32_t x0, uint32_t y0, uint32_t tw, uint32_t th,
                                                  uint32_t tiles_x, float4 *__restrict__ gbuf, uint32_t *__restrict__ key, int brute)
{
    __shared__ int lds_stack[kStackDepth * 64];
    const uint32_t lane = threadIdx.x;
    const uint32_t lx = (blockIdx.x % tiles_x) * 8u + (lane & 7u), ly = (blockIdx.x / tiles_x) * 8u + (lane >> 3);
    if (lx >= tw || ly >= th) return;
    int *stk = lds_stack + lane;
    const uint32_t px = x0 + lx, py = y0 + ly;
    Rng rng;
    f3 o, d;
    primary_ray(S, px, py, kDnSample, tea(px, py * 100u), rng, o, d);
    // the closest hit as k_debug_intersect finds it
    float t_max = CRT_INFINITY;
    uint32_t b_index = kNoHit, b_slot = kNoHit, cn = 0, cp = 0;
    if (brute || !finite3(o) || !finite3(d)) intersect_all(S, o, d, 0xFFFFFFFFu, t_max, b_index, b_slot, cp);
    else traverse<false>(S, stk, o, d, 0xFFFFFFFFu, false, t_max, b_index, b_slot, cn, cp);
    f3 pos = f3{0, 0, 0}, nrm = f3{0, 0, 0};
    uint32_t meta = 0, k = kNoHit;
    if (b_slot != kNoHit) {
        hit_attributes(S, b_slot, o, d, t_max, pos, nrm, meta);
        k = (((meta >> 2) & 3u) << 24) | ((meta >> 18) & 0x3FFFu);    // material, reflectance index (data4.z, data4.y)
    }
    const size_t pix = (size_t)ly * tw + lx;
    gbuf[2 * pix + 0] = float4{t_max, pos.x, pos.y, pos.z};
    gbuf[2 * pix + 1] = float4{nrm.x, nrm.y, nrm.z, bits_f(b_slot != kNoHit ? b_index : kNoHit)};
    key[pix] = k;
}

// The exposure curve of tonemap_rgba8: colour distances are measured where the image is displayed.
__device__ __forceinline__ f3 dn_display(float4 c)
{
    return f3{1.0f - exp_(-2.2f * max_(c.x, 0.0f)), 1.0f - exp_(-2.2f * max_(c.y, 0.0f)), 1.0f - exp_(-2.2f * max_(c.z, 0.0f))};
}

// The filter's input: linear rgb of accum / n (the first half of tonemap_rgba8), and its rgba8 when no iteration follows.
__global__ __launch_bounds__(256) void k_dn_prepare(const float4 *__restrict__ accum, float n, float4 *__restrict__ c,
                                                    uchar4 *__restrict__ rgba, size_t npix)
{
    const size_t i = (size_t)blockIdx.x * 256u + threadIdx.x;
    if (i >= npix) return;
    const float4 a = accum[i];
    const f3 rgb = xyz_to_linear_rgb(f3{a.x, a.y, a.z} / n);
    c[i] = float4{rgb.x, rgb.y, rgb.z, 0.0f};
    if (rgba) rgba[i] = linear_rgb_to_rgba8(rgb);
}

constexpr float kDnMaxFinite = 3.40282347e38f;                  // v is finite where |v| <= this (false for a NaN)
__device__ __forceinline__ bool dn_finite(float v) { return abs_(v) <= kDnMaxFinite; }
__device__ __forceinline__ bool finite4(float4 c) { return dn_finite(c.x) && dn_finite(c.y) && dn_finite(c.z); }

// ---------------------------------------------------------------- what the a-trous kernels share
// The pixel of a thread where block -> B x B pixels: grid (ceil(tw/B), ceil(th/B)) blocks of B * B threads.
template <uint32_t B> __device__ __forceinline__ int dn_xb() { return (int)(blockIdx.x * B + (threadIdx.x & (B - 1u))); }
template <uint32_t B> __device__ __forceinline__ int dn_yb() { return (int)(blockIdx.y * B + threadIdx.x / B); }
__device__ __forceinline__ int dn_x16() { return dn_xb<16>(); }
__device__ __forceinline__ int dn_y16() { return dn_yb<16>(); }

// The B3 spline (1, 4, 6, 4, 1) / 16 at tap i + 2.
__device__ __forceinline__ float dn_h(int i)
{
    const float h[5] = {1.0f / 16.0f, 1.0f / 4.0f, 3.0f / 8.0f, 1.0f / 4.0f, 1.0f / 16.0f};
    return h[i];
}

// The centre pixel's guides: position and normal (zeros at a miss, where no tap reads them).
struct DnGuides { f3 x, n; };
__device__ __forceinline__ DnGuides dn_centre_guides(const float4 *gbuf, size_t p, bool hit)
{
    f3 x_p = f3{0, 0, 0}, n_p = f3{0, 0, 0};
    if (hit) {
        const float4 g0 = gbuf[2 * p], g1 = gbuf[2 * p + 1];
        x_p = f3{g0.y, g0.z, g0.w};
        n_p = f3{g1.x, g1.y, g1.z};
    }
    return DnGuides{x_p, n_p};
}

// e plus the normal and plane terms of a tap with normal n_q at x_q against the centre's guides.
__device__ __forceinline__ float dn_guide_term(float e, f3 n_q, f3 x_q, f3 n_p, f3 x_p, float inv_n, float inv_x)
{
    const f3 dn = n_p - n_q;
    e = e + dot(dn, dn) * inv_n;
    const f3 v = x_q - x_p;
    // (length > 0, not v != 0: positions ~1e-24 apart give v != 0 with dot(v, v) = 0, and 0 / 0 = NaN)
    const float len = length(v);
    if (len > 0.0f) e = e + (abs_(dot(n_p, v)) / len) * inv_x;
    return e;
}

// ... of tap q of the G-buffer.
__device__ __forceinline__ float dn_guide_term(float e, const float4 *gbuf, size_t q, f3 n_p, f3 x_p, float inv_n, float inv_x)
{
    const float4 g0 = gbuf[2 * q], g1 = gbuf[2 * q + 1];
    return dn_guide_term(e, f3{g1.x, g1.y, g1.z}, f3{g0.y, g0.z, g0.w}, n_p, x_p, inv_n, inv_x);
}

// One a-trous iteration.  Taps at step * (-2..2)^2 inside the tile; the centre pixel's guides stay in registers, a tap's
// guides are fetched only when its key matches.  A pixel's result does not depend on B: the block shape only says which
// lane computes it.
template <uint32_t B>
__device__ __forceinline__ void dn_atrous_pixel(const DnParams &P)
{
    const int x = dn_xb<B>(), y = dn_yb<B>();
    const int tw = (int)P.tw, th = (int)P.th, s = (int)P.step;
    if (x >= tw || y >= th) return;
    const size_t p = (size_t)y * P.tw + (size_t)x;
    const uint32_t key_p = P.key[p];
    const bool hit = key_p != kNoHit;
    const DnGuides g_p = dn_centre_guides(P.gbuf, p, hit);
    const f3 x_p = g_p.x, n_p = g_p.n;
    const float4 cp4 = P.c_in[p];
    const f3 t_p = dn_display(cp4);
    float sw = 0.0f;
    f3 sc = f3{0, 0, 0};
#pragma unroll
    for (int dy = -2; dy <= 2; dy++) {
        const int qy = y + dy * s;
        if (qy < 0 || qy >= th) continue;
#pragma unroll
        for (int dx = -2; dx <= 2; dx++) {
            const int qx = x + dx * s;
            if (qx < 0 || qx >= tw) continue;
            if (dx == 0 && dy == 0) {                       // the centre: weight h[2]^2, every other factor is 1
                sw = sw + dn_h(2) * dn_h(2);
                sc = sc + f3{cp4.x, cp4.y, cp4.z} * (dn_h(2) * dn_h(2));
                continue;
            }
            const size_t q = (size_t)qy * P.tw + (size_t)qx;
            if (P.key[q] != key_p) continue;
            const float4 cq4 = P.c_in[q];
            if (!finite4(cq4)) continue;
            // (recomputed per tap: a stored dn_display(c) costs another 16 B per tap, and the pass is bound by tap traffic)
            const f3 dt = t_p - dn_display(cq4);
            float e = dot(dt, dt) * P.inv_c;
            if (hit) e = dn_guide_term(e, P.gbuf, q, n_p, x_p, P.inv_n, P.inv_x);
            const float w = (dn_h(dx + 2) * dn_h(dy + 2)) * exp_(-e);
            sw = sw + w;
            sc = sc + f3{cq4.x, cq4.y, cq4.z} * w;
        }
    }
    const f3 c = sc / sw;
    P.c_out[p] = float4{c.x, c.y, c.z, 0.0f};
    if (P.rgba) P.rgba[p] = linear_rgb_to_rgba8(c);
}

// grid: dn_x16
__global__ __launch_bounds__(256) void k_dn_atrous(const DnParams P) { dn_atrous_pixel<16>(P); }
// The same pass in one-wave blocks of 8x8 pixels, for launches beside a live wavefront pool (crt_denoise_latest, DESIGN.md
// 6m): a block of several waves waits for as many free slots on one CU.
__global__ __launch_bounds__(64) void k_dn_atrous_w64(const DnParams P) { dn_atrous_pixel<8>(P); }

// ---------------------------------------------------------------- the variance-guided filter (crt_denoise_adaptive)
// DESIGN.md 6d defines it operation by operation (tests/denoise_adaptive_ref.py is its numpy restatement).  The colour
// buffers carry the pixel's variance v in their w lane, so v_q rides along with c_q; the blurred variance rides along
// with the key in one 8-byte word, so a matching tap costs the four requests of the plain filter.
struct DnAsParams {
    const float4 *c_in;         // linear rgb, w = variance v of the previous iteration
    float4 *c_out;
    const float4 *gbuf;
    const uint2 *kv;            // per pixel: (key, bits of the 3x3 blur of v)
    uchar4 *rgba;               // null, or the rgba8 of c_out (last iteration)
    float *var;                 // null, or v of c_out (last iteration)
    uint32_t tw, th, step;
    float sv2;                  // sigma_variance^2
    float inv_n, inv_x;
};

constexpr float kDnEps = (0.5f / 255.0f) * (0.5f / 255.0f);      // half an 8-bit step, squared

// The filter's input in the adaptive state: c = M (accum / n) and v = e * e with the count n of the pixel's 8x8 tile.
// v = 1 ("nothing known") below 2 samples or where e * e is not finite (e NaN or infinite, or its square overflows).
__global__ __launch_bounds__(256) void k_dn_prepare_as(const float4 *__restrict__ accum, const float *__restrict__ q,
                                                       const uint32_t *__restrict__ counts, uint32_t tw, uint32_t th,
                                                       uint32_t tiles_x, float4 *__restrict__ c, uchar4 *__restrict__ rgba,
                                                       float *__restrict__ var)
{
    const uint32_t x = blockIdx.x * 64u + (threadIdx.x & 63u), y = blockIdx.y * 4u + (threadIdx.x >> 6);
    if (x >= tw || y >= th) return;
    const size_t i = (size_t)y * tw + x;
    const uint32_t n_t = counts[(y >> 3) * tiles_x + (x >> 3)];
    const float4 a = accum[i];
    const f3 rgb = xyz_to_linear_rgb(f3{a.x, a.y, a.z} / (float)n_t);
    float v = 1.0f;
    if (n_t >= 2u) {
        const float e = pixel_error(a.y, q[i], n_t);
        const float ee = e * e;
        if (ee <= kDnMaxFinite) v = ee;
    }
    c[i] = float4{rgb.x, rgb.y, rgb.z, v};
    if (rgba) rgba[i] = linear_rgb_to_rgba8(rgb);
    if (var) var[i] = v;
}

// (1,2,1) x (1,2,1) / 16 of v at unit step over the taps inside the tile whose key equals the centre's, renormalised;
// written next to the key.  grid as k_dn_atrous.
__global__ __launch_bounds__(256) void k_dn_vblur(const float4 *__restrict__ c, const uint32_t *__restrict__ key,
                                                  uint2 *__restrict__ kv, uint32_t utw, uint32_t uth)
{
    const int x = dn_x16(), y = dn_y16();
    const int tw = (int)utw, th = (int)uth;
    if (x >= tw || y >= th) return;
    const size_t p = (size_t)y * utw + (size_t)x;
    const uint32_t key_p = key[p];
    const float g[3] = {0.25f, 0.5f, 0.25f};
    float sv = 0.0f, sw = 0.0f;
#pragma unroll
    for (int dy = -1; dy <= 1; dy++) {
        const int qy = y + dy;
        if (qy < 0 || qy >= th) continue;
#pragma unroll
        for (int dx = -1; dx <= 1; dx++) {
            const int qx = x + dx;
            if (qx < 0 || qx >= tw) continue;
            const size_t q = (size_t)qy * utw + (size_t)qx;
            if (key[q] != key_p) continue;                      // (the centre always passes)
            const float w = g[dx + 1] * g[dy + 1];
            sv = sv + w * c[q].w;
            sw = sw + w;
        }
    }
    kv[p] = uint2{key_p, f_bits(sv / sw)};
}

// One iteration: k_dn_atrous with the colour term scaled by the two pixels' blurred variances, and the variance carried
// through the same weights.
__global__ __launch_bounds__(256) void k_dn_atrous_as(const DnAsParams P)
{
    const int x = dn_x16(), y = dn_y16();
    const int tw = (int)P.tw, th = (int)P.th, s = (int)P.step;
    if (x >= tw || y >= th) return;
    const size_t p = (size_t)y * P.tw + (size_t)x;
    const uint2 kv_p = P.kv[p];
    const uint32_t key_p = kv_p.x;
    const float vt_p = bits_f(kv_p.y);
    const bool hit = key_p != kNoHit;
    const DnGuides g_p = dn_centre_guides(P.gbuf, p, hit);
    const f3 x_p = g_p.x, n_p = g_p.n;
    const float4 cp4 = P.c_in[p];
    const f3 t_p = dn_display(cp4);
    float sw = 0.0f, sv = 0.0f;
    f3 sc = f3{0, 0, 0};
#pragma unroll
    for (int dy = -2; dy <= 2; dy++) {
        const int qy = y + dy * s;
        if (qy < 0 || qy >= th) continue;
#pragma unroll
        for (int dx = -2; dx <= 2; dx++) {
            const int qx = x + dx * s;
            if (qx < 0 || qx >= tw) continue;
            if (dx == 0 && dy == 0) {
                const float w = dn_h(2) * dn_h(2);
                sw = sw + w;
                sc = sc + f3{cp4.x, cp4.y, cp4.z} * w;
                sv = sv + (w * w) * cp4.w;
                continue;
            }
            const size_t q = (size_t)qy * P.tw + (size_t)qx;
            const uint2 kv_q = P.kv[q];
            if (kv_q.x != key_p) continue;
            const float4 cq4 = P.c_in[q];
            if (!finite4(cq4)) continue;
            const f3 dt = t_p - dn_display(cq4);
            float e = dot(dt, dt) / (P.sv2 * (vt_p + bits_f(kv_q.y)) + kDnEps);
            if (hit) e = dn_guide_term(e, P.gbuf, q, n_p, x_p, P.inv_n, P.inv_x);
            const float w = (dn_h(dx + 2) * dn_h(dy + 2)) * exp_(-e);
            sw = sw + w;
            sc = sc + f3{cq4.x, cq4.y, cq4.z} * w;
            sv = sv + (w * w) * cq4.w;
        }
    }
    const f3 c = sc / sw;
    // (a centre whose colour is not finite has NaN weights: it keeps its v, so that v stays finite and the NaN reaches
    // no neighbour through the blurred variance either)
    const float v = finite4(cp4) ? sv / (sw * sw) : cp4.w;
    P.c_out[p] = float4{c.x, c.y, c.z, v};
    if (P.rgba) P.rgba[p] = linear_rgb_to_rgba8(c);
    if (P.var) P.var[p] = v;
}

// ---------------------------------------------------------------- temporal reuse (crt_denoise_temporal)
// DESIGN.md 6e defines it operation by operation (tests/denoise_temporal_ref.py is its numpy restatement).
// What k_dn_reproject and k_dn_motion share, so that the motion output cannot drift from the blend: steps 1-2 of 6e (the
// film position of the pixel's first hit in the previous camera, binary64, nothing contracted), and with MOTION the map
// of 6f before them -- the hit carried through its primitive's record as the PREVIOUS slot saw it (P.raw_prev).
struct DnMapped {
    double u, v;                    // rectangle-local film position in the previous camera
    f3 x, n;                        // x~ rounded to float and n~: what the taps' plane and normal tests compare against
};

__device__ __forceinline__ double dn_dot64(const double a[3], const double b[3]) { return (a[0] * b[0] + a[1] * b[1]) + a[2] * b[2]; }
__device__ __forceinline__ f3 dn_xyz(uint4 w) { return f3{bits_f(w.x), bits_f(w.y), bits_f(w.z)}; }
__device__ __forceinline__ bool dn_same_xyz(uint4 a, uint4 b) { return a.x == b.x && a.y == b.y && a.z == b.z; }

// false: the pixel takes no history (a changed spectrum, a map that refuses, depth <= 0 or not finite).
template <bool MOTION>
__device__ __forceinline__ bool dn_film_position(const DnReprojParams &P, f3 x_p, f3 n_p, uint32_t index, DnMapped &o)
{
    double X[3] = {(double)x_p.x, (double)x_p.y, (double)x_p.z};
    o.x = x_p; o.n = n_p;
    if constexpr (MOTION) {
        if (index >= P.nprim) return false;                     // (no hit names one: the loads below stay inside the buffers)
        const uint4 *rc = (const uint4 *)(P.raw + (size_t)index * 80), *rp = (const uint4 *)(P.raw_prev + (size_t)index * 80);
        const uint4 c1 = rc[1], c2 = rc[2], c3 = rc[3], c4 = rc[4], p1 = rp[1], p2 = rp[2], p3 = rp[3], p4 = rp[4];
        // compared before anything is computed: a pixel on a record that did not change pays the loads alone
        if (!(dn_same_xyz(c1, p1) && dn_same_xyz(c2, p2) && dn_same_xyz(c3, p3) && c4.x == p4.x && c4.y == p4.y)) {
            if (c4.x != p4.x || c4.y != p4.y) return false;     // emission or reflectance changed: what the history holds is stale
            const f3 d1 = dn_xyz(c1), d2 = dn_xyz(c2), d3 = dn_xyz(c3), q1 = dn_xyz(p1), q2 = dn_xyz(p2), q3 = dn_xyz(p3);
            const double D1[3] = {(double)d1.x, (double)d1.y, (double)d1.z}, Q1[3] = {(double)q1.x, (double)q1.y, (double)q1.z};
            if (rc[0].x == 1u) {                                // sphere: same direction from the centre, radius scaled
                const double rho = (double)q2.x / (double)d2.x;
                if (!(d2.x != 0.0f) || !(fabs(rho) <= 1.7976931348623157e308)) return false;
                for (int k = 0; k < 3; k++) X[k] = Q1[k] + (X[k] - D1[k]) * rho;
            } else {                                            // patch, triangle: same coordinates in the edges' frame
                const double D2[3] = {(double)d2.x, (double)d2.y, (double)d2.z}, D3[3] = {(double)d3.x, (double)d3.y, (double)d3.z};
                const double E[3] = {X[0] - D1[0], X[1] - D1[1], X[2] - D1[2]};
                const double g11 = dn_dot64(D2, D2), g22 = dn_dot64(D3, D3), g12 = dn_dot64(D2, D3);
                const double det = g11 * g22 - g12 * g12;
                if (!(det > 0.0 && det <= 1.7976931348623157e308)) return false;
                const double b1 = dn_dot64(E, D2), b2 = dn_dot64(E, D3);
                const double beta = (b1 * g22 - b2 * g12) / det, gamma = (b2 * g11 - b1 * g12) / det;
                const double Q2[3] = {(double)q2.x, (double)q2.y, (double)q2.z}, Q3[3] = {(double)q3.x, (double)q3.y, (double)q3.z};
                for (int k = 0; k < 3; k++) X[k] = (Q1[k] + beta * Q2[k]) + gamma * Q3[k];
                const f3 m = normalize(cross(q2, q3));          // hit_attributes_rec's normal of the old pose, on n_p's side
                o.n = dot(n_p, normalize(cross(d2, d3))) < 0.0f ? f3{-m.x, -m.y, -m.z} : m;
            }
            o.x = f3{(float)X[0], (float)X[1], (float)X[2]};
        }
    }
    const double dx_ = X[0] - P.eye_prev[0], dy_ = X[1] - P.eye_prev[1], dz_ = X[2] - P.eye_prev[2];
    const double pa = (P.m[0] * dx_ + P.m[1] * dy_) + P.m[2] * dz_;
    const double pb = (P.m[3] * dx_ + P.m[4] * dy_) + P.m[5] * dz_;
    const double pc = (P.m[6] * dx_ + P.m[7] * dy_) + P.m[8] * dz_;
    if (!(pc > 0.0 && pc <= 1.7976931348623157e308)) return false;
    o.u = ((pa / pc) * P.W - 0.53125) - P.x0;
    o.v = ((P.H + 0.53125) - (pb / pc) * P.H) - P.y0;
    return true;
}

// k_dn_prepare's work, the reprojection into the previous frame and the blend in one pass: grid as k_dn_atrous.  The
// pixel's own guides stay in registers; a tap's history and G-buffer are fetched only when its key matches.
// <false, *>: PREVIOUS saw the scene as it is (6e alone); <true, *>: PREVIOUS has a geometry snapshot (6f).
// <*, true> (crt_denoise_svgf; tests/denoise_svgf_ref.py): the accepted taps also carry the temporal moments
// of the luminance -- one more float4 per tap that passed every test -- and the variance they give goes out as the w of
// the filter's input P.cv.  What reaches P.h_cur is <*, false>'s bit for bit.
// <*, *, true> (option "adaptive_temporal"; tests/denoise_temporal_adaptive_ref.py): the context is in the
// adaptive state, and the n of the pixel is the count of its 8x8 tile wherever 6e-6g say n.  Nothing else differs.
// 6g's variance of a pixel from its moments and whether it is known: F = Mw / n >= min_frames and t finite.  v = t where
// known, 1 elsewhere.  The one statement of that test: k_dn_reproject<*, true> and k_dn_spatial_var (6j) both call it.
__device__ __forceinline__ bool dn_known(float m1, float ms, float Mw, float n, float min_frames, float &v)
{
    v = 1.0f;
    const float F = Mw / n;
    if (!(F >= min_frames)) return false;
    const float g = 2.2f * exp_(-2.2f * max_(m1, 0.0f));
    const float t = (g * g) * (ms / (F - 1.0f));
    if (!dn_finite(t)) return false;
    v = t;
    return true;
}

// ---------------------------------------------------------------- the clip box (option "temporal_clip_pct")
// DESIGN.md 6l defines it operation by operation (tests/denoise_clip_ref.py is its numpy restatement).  Launched before
// k_dn_reproject on the same grid: every pixel that can reuse history gets lo = mu - gamma sigma and hi = mu + gamma sigma
// per channel from the frame's own c_new over the 7x7 taps of its key, and the blend clamps the reprojected h to them.
//
// The block's 22 x 22 halo is staged once in LDS as four planes (key, r, g, b) in k_dn_spatial_var's layout (explained
// there): pitch 48 dwords, two planes per set of rows.  accum -> c_new is converted once per staged cell.
constexpr int kSvRadius = 3, kSvTile = 16 + 2 * kSvRadius, kSvPitch = 48, kSvPair = kSvTile * kSvPitch;
constexpr uint32_t kDnNoTap = 0xFFFFFFFEu;                       // the key of a cell no pixel accepts (keys are < 2^26, or kNoHit)
__device__ __forceinline__ constexpr int dn_sv_plane(int k) { return (k >> 1) * kSvPair + (k & 1) * (kSvPitch / 2); }

template <bool ADAPT>
__global__ __launch_bounds__(256) void k_dn_clip_box(const std::conditional_t<ADAPT, DnAdaptive<DnClipParams>, DnClipParams> P)
{
    __shared__ float tile[2 * kSvPair];
    const int x = dn_x16(), y = dn_y16();
    const int tw = (int)P.tw, th = (int)P.th;
    const bool inside = x < tw && y < th;
    const size_t p = (size_t)y * P.tw + (size_t)x;
    // c_new of the pixel at (qx, qy) inside the rectangle: k_dn_reproject's expression
    const auto c_new_at = [&](int qx, int qy) {
        const float4 a = P.accum[(size_t)qy * P.tw + (size_t)qx];
        float n = P.n;
        if constexpr (ADAPT) n = (float)P.counts[(size_t)((uint32_t)qy >> 3) * P.tiles_x + ((uint32_t)qx >> 3)];
        return xyz_to_linear_rgb(f3{a.x, a.y, a.z} / n);
    };
    uint32_t key_p = kNoHit;
    bool need = false;
    if (inside) {
        key_p = P.key[p];
        if (key_p != kNoHit && (key_p >> 24) != kGlass) {
            const f3 c = c_new_at(x, y);
            need = finite4(float4{c.x, c.y, c.z, 0.0f});
        }
    }
    // no pixel of the block can have a box (sky, glass): nothing is staged
    const bool any = __syncthreads_or(need ? 1 : 0) != 0;
    if (inside && !need) { P.box[2 * p] = float4{0, 0, 0, 0}; P.box[2 * p + 1] = float4{0, 0, 0, 0}; }
    if (!any) return;
    const int bx = (int)(blockIdx.x * 16u) - kSvRadius, by = (int)(blockIdx.y * 16u) - kSvRadius;
    for (int i = (int)threadIdx.x; i < kSvTile * kSvTile; i += 256) {
        const int cy = i / kSvTile, cx = i - cy * kSvTile;
        const int qx = bx + cx, qy = by + cy;
        uint32_t k = kDnNoTap;                                  // outside the rectangle, or a colour that is not finite
        f3 c = f3{0, 0, 0};
        if (qx >= 0 && qx < tw && qy >= 0 && qy < th) {
            const f3 cq = c_new_at(qx, qy);
            if (finite4(float4{cq.x, cq.y, cq.z, 0.0f})) { k = P.key[(size_t)qy * P.tw + (size_t)qx]; c = cq; }
        }
        const int cell = cy * kSvPitch + cx;
        tile[dn_sv_plane(0) + cell] = bits_f(k);
        tile[dn_sv_plane(1) + cell] = c.x; tile[dn_sv_plane(2) + cell] = c.y; tile[dn_sv_plane(3) + cell] = c.z;
    }
    __syncthreads();
    if (!need) return;
    const int c0 = ((int)(threadIdx.x >> 4) + kSvRadius) * kSvPitch + (int)(threadIdx.x & 15u) + kSvRadius;
    // Both loops are unrolled in full; only the accepted taps' 49-bit mask stays in registers between them.
    constexpr int kSide = 2 * kSvRadius + 1;
    uint64_t accepted = 0;
    float N = 0.0f;
    f3 sum = f3{0, 0, 0}, S = f3{0, 0, 0};
#pragma unroll
    for (int dy = -kSvRadius; dy <= kSvRadius; dy++)
#pragma unroll
        for (int dx = -kSvRadius; dx <= kSvRadius; dx++) {
            const int c = c0 + dy * kSvPitch + dx, i = (dy + kSvRadius) * kSide + dx + kSvRadius;
            if (f_bits(tile[dn_sv_plane(0) + c]) != key_p) continue;        // (the centre always passes)
            accepted |= 1ull << i;
            N = N + 1.0f;
            sum = sum + f3{tile[dn_sv_plane(1) + c], tile[dn_sv_plane(2) + c], tile[dn_sv_plane(3) + c]};
        }
    const f3 mu = sum / N;
    // (a second pass, not m2 - m1^2: 6g's cancellation; the window is in LDS, so it costs no traffic)
#pragma unroll
    for (int dy = -kSvRadius; dy <= kSvRadius; dy++)
#pragma unroll
        for (int dx = -kSvRadius; dx <= kSvRadius; dx++) {
            const int c = c0 + dy * kSvPitch + dx, i = (dy + kSvRadius) * kSide + dx + kSvRadius;
            if (!((accepted >> i) & 1ull)) continue;
            const f3 d = f3{tile[dn_sv_plane(1) + c], tile[dn_sv_plane(2) + c], tile[dn_sv_plane(3) + c]} - mu;
            S = S + f3{d.x * d.x, d.y * d.y, d.z * d.z};
        }
    const f3 v = S / N;
    const f3 r = f3{sqrt_(v.x), sqrt_(v.y), sqrt_(v.z)} * P.gamma;
    const f3 lo = mu - r, hi = mu + r;
    const bool valid = N >= 4.0f && finite4(float4{lo.x, lo.y, lo.z, 0.0f}) && finite4(float4{hi.x, hi.y, hi.z, 0.0f});
    P.box[2 * p] = float4{lo.x, lo.y, lo.z, N};
    P.box[2 * p + 1] = float4{hi.x, hi.y, hi.z, valid ? 1.0f : 0.0f};
}

template <bool MOMENTS, bool ADAPT>
using DnReprojArg = std::conditional_t<ADAPT, DnAdaptive<std::conditional_t<MOMENTS, DnSvgfParams, DnReprojParams>>,
                                       std::conditional_t<MOMENTS, DnSvgfParams, DnReprojParams>>;

template <bool MOTION, bool MOMENTS, bool ADAPT>
__global__ __launch_bounds__(256) void k_dn_reproject(const DnReprojArg<MOMENTS, ADAPT> P)
{
    const int x = dn_x16(), y = dn_y16();
    const int tw = (int)P.tw, th = (int)P.th;
    if (x >= tw || y >= th) return;
    const size_t p = (size_t)y * P.tw + (size_t)x;
    const float4 a = P.accum[p];
    float n = P.n;
    if constexpr (ADAPT) n = (float)P.counts[(size_t)((uint32_t)y >> 3) * P.tiles_x + ((uint32_t)x >> 3)];
    const f3 c_new = xyz_to_linear_rgb(f3{a.x, a.y, a.z} / n);
    f3 c = c_new;
    float Hw = n;
    const float lum = a.y / n;                                  // y of 6g: the frame's mean luminance
    float m1 = lum, ms = 0.0f, Mw = n;                            // (MOMENTS only)
    const uint32_t key_p = P.key[p];
    if (P.h_prev && key_p != kNoHit && (key_p >> 24) != kGlass && finite4(float4{c_new.x, c_new.y, c_new.z, 0.0f})) {
        const float4 g0 = P.gbuf[2 * p], g1 = P.gbuf[2 * p + 1];
        const f3 x_p = f3{g0.y, g0.z, g0.w}, n_p = f3{g1.x, g1.y, g1.z};
        DnMapped mp;
        if (dn_film_position<MOTION>(P, x_p, n_p, f_bits(g1.w), mp)) {
            const double u = mp.u, v = mp.v;
            const f3 x_m = mp.x, n_m = mp.n;
            // (a NaN fails both comparisons; the bounds also keep the conversions to int defined)
            if (u >= -1.0 && u < (double)tw && v >= -1.0 && v < (double)th) {
                const double fu = floor(u), fv = floor(v);
                const int ix = (int)fu, iy = (int)fv;
                const float fx = (float)(u - fu), fy = (float)(v - fv);
                const float wx[2] = {1.0f - fx, fx}, wy[2] = {1.0f - fy, fy};
                const f3 d = x_m - f3{(float)P.eye_prev[0], (float)P.eye_prev[1], (float)P.eye_prev[2]};
                const float r_p = max_(P.kappa * length(x_p - f3{P.eye[0], P.eye[1], P.eye[2]}), P.kappa_prev * length(d));
                const float plane_max = P.plane_tol * r_p;
                float sw = 0.0f, sh = 0.0f;
                f3 sc = f3{0, 0, 0};
                f3 sm = f3{0, 0, 0};                            // (MOMENTS only) sums of w m1', w s', w Mw'
#pragma unroll
                for (int dy = 0; dy < 2; dy++) {
                    const int qy = iy + dy;
                    if (qy < 0 || qy >= th) continue;
#pragma unroll
                    for (int dx = 0; dx < 2; dx++) {
                        const int qx = ix + dx;
                        if (qx < 0 || qx >= tw) continue;
                        const size_t q = (size_t)qy * P.tw + (size_t)qx;
                        if (P.key_prev[q] != key_p) continue;
                        const float4 hq = P.h_prev[q];
                        if (!(hq.w > 0.0f) || !finite4(hq)) continue;
                        const float4 q0 = P.gbuf_prev[2 * q], q1 = P.gbuf_prev[2 * q + 1];
                        const f3 dn = n_m - f3{q1.x, q1.y, q1.z};
                        if (!(dot(dn, dn) <= P.normal_tol2)) continue;
                        if (!(abs_(dot(n_m, f3{q0.y, q0.z, q0.w} - x_m)) <= plane_max)) continue;
                        const float w = wx[dx] * wy[dy];
                        sw = sw + w;
                        sc = sc + f3{hq.x, hq.y, hq.z} * w;
                        sh = sh + w * hq.w;
                        if constexpr (MOMENTS) {
                            if (P.m_prev) {
                                const float4 mq = P.m_prev[q];
                                sm = sm + f3{mq.x, mq.y, mq.z} * w;
                            }
                        }
                    }
                }
                if (sw > 0.0f) {
                    f3 h = sc / sw;
                    if (P.box) {                                // 6l: the history clamped to the frame's own neighbourhood
                        const float4 b0 = P.box[2 * p], b1 = P.box[2 * p + 1];
                        if (b1.w != 0.0f) h = f3{min_(max_(h.x, b0.x), b1.x), min_(max_(h.y, b0.y), b1.y), min_(max_(h.z, b0.z), b1.z)};
                    }
                    const float Hp = min_(sh / sw, P.max_history);
                    Hw = n + Hp;
                    c = (c_new * n + h * Hp) / Hw;
                    if constexpr (MOMENTS) {
                        if (P.m_prev) {                         // the pairwise merge of (lum, 0, n) with the taps' (h1, hs, Mp)
                            const float h1 = sm.x / sw, hs = sm.y / sw;
                            const float Mp = min_(sm.z / sw, P.max_history);
                            const float d = lum - h1;
                            Mw = n + Mp;
                            m1 = (lum * n + h1 * Mp) / Mw;
                            ms = (Mp / Mw) * hs + ((n * Mp) * (d * d)) / (Mw * Mw);
                        }
                    }
                }
            }
        }
    }
    P.h_cur[p] = float4{c.x, c.y, c.z, Hw};
    if (P.rgba) P.rgba[p] = linear_rgb_to_rgba8(c);
    if (P.hist) P.hist[p] = Hw;
    if constexpr (MOMENTS) {
        // the variance of the blend in display units: s / (F - 1) over F = Mw / n frames, through the exposure curve's slope
        // at m1 (as pixel_error); 1 ("nothing known", as k_dn_prepare_as) below min_frames or where it is not finite
        float v;
        dn_known(m1, ms, Mw, n, P.min_frames, v);
        P.m_cur[p] = float4{m1, ms, Mw, 0.0f};
        P.cv[p] = float4{c.x, c.y, c.z, v};
        if (P.var) P.var[p] = v;
    }
}

// crt_read_motion: where the blend above looks for each pixel in the PREVIOUS slot -- (u, v) rounded to float, NaN where
// no position exists.  grid as k_dn_atrous.
template <bool MOTION>
__global__ __launch_bounds__(256) void k_dn_motion(const DnReprojParams P, float2 *__restrict__ out)
{
    const int x = dn_x16(), y = dn_y16();
    if (x >= (int)P.tw || y >= (int)P.th) return;
    const size_t p = (size_t)y * P.tw + (size_t)x;
    const float nan = bits_f(0x7FC00000u);
    float2 uv = float2{nan, nan};
    const uint32_t key_p = P.key[p];
    if (P.h_prev && key_p != kNoHit && (key_p >> 24) != kGlass) {
        const float4 g0 = P.gbuf[2 * p], g1 = P.gbuf[2 * p + 1];
        DnMapped mp;
        if (dn_film_position<MOTION>(P, f3{g0.y, g0.z, g0.w}, f3{g1.x, g1.y, g1.z}, f_bits(g1.w), mp)) uv = float2{(float)mp.u, (float)mp.v};
    }
    out[p] = uv;
}

// ---------------------------------------------------------------- the spatial variance estimate (option "svgf_spatial_pct")
// DESIGN.md 6j defines it operation by operation (tests/denoise_svgf_spatial_ref.py is its numpy restatement).  Launched
// after k_dn_reproject<*, true> on the same grid: a pixel that is not `known` (dn_known) and not excluded takes
// v = b g^2 (S / (A - 1)) / Mw_p from the precision-weighted spread of m1 over the 7x7 taps of its own key.
//
// The block's 22 x 22 halo tile is staged once in LDS as nine planes (key, m1, Mw, normal, position); both passes read LDS
// only.  Row pitch 48 dwords: the two rows a 32-lane half of the wave reads in one ds_read_b32 lie 48 = 16 (mod 32) banks
// apart, 16 consecutive dwords each, so the 32 lanes hit 32 different banks.  A row holds 22 of its 48 dwords, so two
// planes share one set of rows, the second from dword 24 on (kSvPitch, dn_sv_plane: declared above k_dn_clip_box, which
// stages its four planes the same way).

// What a pixel's moments must hold to take part, as centre or as tap: m1 and Mw finite, Mw > 0.
__device__ __forceinline__ bool dn_sv_holds(float m1, float Mw) { return dn_finite(m1) && dn_finite(Mw) && Mw > 0.0f; }

template <bool ADAPT>
__global__ __launch_bounds__(256) void k_dn_spatial_var(const std::conditional_t<ADAPT, DnAdaptive<DnSpatialParams>, DnSpatialParams> P)
{
    __shared__ float tile[5 * kSvPair];
    const int x = dn_x16(), y = dn_y16();
    const int tw = (int)P.tw, th = (int)P.th;
    const size_t p = (size_t)y * P.tw + (size_t)x;
    uint32_t key_p = kNoHit;
    float Mw_p = 0.0f;
    bool need = false;
    if (x < tw && y < th) {
        key_p = P.key[p];
        const float4 m = P.m_cur[p];
        float n = P.n, v;
        if constexpr (ADAPT) n = (float)P.counts[(size_t)((uint32_t)y >> 3) * P.tiles_x + ((uint32_t)x >> 3)];
        Mw_p = m.z;
        need = !dn_known(m.x, m.y, m.z, n, P.min_frames, v) && key_p != kNoHit && (key_p >> 24) != kGlass && dn_sv_holds(m.x, m.z);
    }
    // every pixel of the block known or excluded (most blocks of a steady orbit): nothing is staged
    if (!__syncthreads_or(need ? 1 : 0)) return;
    const int bx = (int)(blockIdx.x * 16u) - kSvRadius, by = (int)(blockIdx.y * 16u) - kSvRadius;
    for (int i = (int)threadIdx.x; i < kSvTile * kSvTile; i += 256) {
        const int cy = i / kSvTile, cx = i - cy * kSvTile;
        const int qx = bx + cx, qy = by + cy;
        uint32_t k = kDnNoTap;                                  // outside the rectangle, or moments that take no part
        float m1 = 0.0f, Mw = 0.0f;
        float4 g0 = float4{0, 0, 0, 0}, g1 = float4{0, 0, 0, 0};
        if (qx >= 0 && qx < tw && qy >= 0 && qy < th) {
            const size_t q = (size_t)qy * P.tw + (size_t)qx;
            const float4 m = P.m_cur[q];
            if (dn_sv_holds(m.x, m.z)) {
                k = P.key[q]; m1 = m.x; Mw = m.z;
                if (k != kNoHit) { g0 = P.gbuf[2 * q]; g1 = P.gbuf[2 * q + 1]; }
            }
        }
        const int c = cy * kSvPitch + cx;
        tile[dn_sv_plane(0) + c] = bits_f(k);
        tile[dn_sv_plane(1) + c] = m1;
        tile[dn_sv_plane(2) + c] = Mw;
        tile[dn_sv_plane(3) + c] = g1.x; tile[dn_sv_plane(4) + c] = g1.y; tile[dn_sv_plane(5) + c] = g1.z;
        tile[dn_sv_plane(6) + c] = g0.y; tile[dn_sv_plane(7) + c] = g0.z; tile[dn_sv_plane(8) + c] = g0.w;
    }
    __syncthreads();
    if (!need) return;
    const int c0 = ((int)(threadIdx.x >> 4) + kSvRadius) * kSvPitch + (int)(threadIdx.x & 15u) + kSvRadius;
    const auto nrm = [&](int c) { return f3{tile[dn_sv_plane(3) + c], tile[dn_sv_plane(4) + c], tile[dn_sv_plane(5) + c]}; };
    const auto pos = [&](int c) { return f3{tile[dn_sv_plane(6) + c], tile[dn_sv_plane(7) + c], tile[dn_sv_plane(8) + c]}; };
    const f3 n_p = nrm(c0), x_p = pos(c0);
    // w Mw_q of the tap at cell c, and w itself; false: the tap is not accepted
    const auto tap = [&](int c, bool centre, float &w, float &wm) {
        if (f_bits(tile[dn_sv_plane(0) + c]) != key_p) return false;
        w = centre ? 1.0f : exp_(-dn_guide_term(0.0f, nrm(c), pos(c), n_p, x_p, P.inv_n, P.inv_x));
        wm = w * tile[dn_sv_plane(2) + c];
        return true;
    };
    // Both loops are unrolled in full: the accepted taps and their w Mw_q stay in registers (a 49-bit mask, 49 floats), so
    // the second pass reads m1 alone and evaluates no weight again.
    constexpr int kSide = 2 * kSvRadius + 1;
    float A = 0.0f, B = 0.0f, C = 0.0f, S = 0.0f, w, wm, wms[kSide * kSide];
    uint64_t accepted = 0;
#pragma unroll
    for (int dy = -kSvRadius; dy <= kSvRadius; dy++)
#pragma unroll
        for (int dx = -kSvRadius; dx <= kSvRadius; dx++) {
            const int c = c0 + dy * kSvPitch + dx, i = (dy + kSvRadius) * kSide + dx + kSvRadius;
            wms[i] = 0.0f;
            if (!tap(c, dx == 0 && dy == 0, w, wm)) continue;
            accepted |= 1ull << i;
            wms[i] = wm;
            A = A + w;
            B = B + wm;
            C = C + wm * tile[dn_sv_plane(1) + c];
        }
    const float mu = C / B;
    // (a second pass, not m2 - m1^2: 6g's cancellation; the window is in LDS, so it costs no traffic)
#pragma unroll
    for (int dy = -kSvRadius; dy <= kSvRadius; dy++)
#pragma unroll
        for (int dx = -kSvRadius; dx <= kSvRadius; dx++) {
            const int c = c0 + dy * kSvPitch + dx, i = (dy + kSvRadius) * kSide + dx + kSvRadius;
            if (!((accepted >> i) & 1ull)) continue;
            const float d = tile[dn_sv_plane(1) + c] - mu;
            S = S + wms[i] * (d * d);
        }
    const float s2 = S / (A - 1.0f);
    const float g = 2.2f * exp_(-2.2f * max_(mu, 0.0f));
    const float t = P.b * ((g * g) * (s2 / Mw_p));
    const float v = A >= 4.0f && dn_finite(t) ? t : 1.0f;
    P.cv[p].w = v;
    if (P.var) P.var[p] = v;
}

#ifdef CRT_PROBE_SV_DIRECT
// The probe build of DESIGN.md 6j (EXTRA=-DCRT_PROBE_SV_DIRECT): the same estimate with every tap gathered from global
// memory, nothing staged -- what the LDS tile is measured against (timing only: no test runs it).
template <bool ADAPT>
__global__ __launch_bounds__(256) void k_dn_spatial_var_direct(const std::conditional_t<ADAPT, DnAdaptive<DnSpatialParams>, DnSpatialParams> P)
{
    const int x = dn_x16(), y = dn_y16();
    const int tw = (int)P.tw, th = (int)P.th;
    if (x >= tw || y >= th) return;
    const size_t p = (size_t)y * P.tw + (size_t)x;
    const uint32_t key_p = P.key[p];
    const float4 m = P.m_cur[p];
    float n = P.n, v0;
    if constexpr (ADAPT) n = (float)P.counts[(size_t)((uint32_t)y >> 3) * P.tiles_x + ((uint32_t)x >> 3)];
    if (dn_known(m.x, m.y, m.z, n, P.min_frames, v0) || key_p == kNoHit || (key_p >> 24) == kGlass || !dn_sv_holds(m.x, m.z)) return;
    const DnGuides g_p = dn_centre_guides(P.gbuf, p, true);
    float A = 0.0f, B = 0.0f, C = 0.0f, S = 0.0f, mu = 0.0f;
    for (int pass = 0; pass < 2; pass++) {
#pragma unroll 1
        for (int dy = -kSvRadius; dy <= kSvRadius; dy++)
#pragma unroll
            for (int dx = -kSvRadius; dx <= kSvRadius; dx++) {
                const int qx = x + dx, qy = y + dy;
                if (qx < 0 || qx >= tw || qy < 0 || qy >= th) continue;
                const size_t q = (size_t)qy * P.tw + (size_t)qx;
                if (P.key[q] != key_p) continue;
                const float4 mq = P.m_cur[q];
                if (!dn_sv_holds(mq.x, mq.z)) continue;
                const float w = dx == 0 && dy == 0 ? 1.0f : exp_(-dn_guide_term(0.0f, P.gbuf, q, g_p.n, g_p.x, P.inv_n, P.inv_x));
                const float wm = w * mq.z;
                if (pass == 0) { A = A + w; B = B + wm; C = C + wm * mq.x; }
                else { const float d = mq.x - mu; S = S + wm * (d * d); }
            }
        mu = C / B;
    }
    const float g = 2.2f * exp_(-2.2f * max_(mu, 0.0f));
    const float t = P.b * ((g * g) * ((S / (A - 1.0f)) / m.z));
    const float v = A >= 4.0f && dn_finite(t) ? t : 1.0f;
    P.cv[p].w = v;
    if (P.var) P.var[p] = v;
}
#define k_dn_spatial_var k_dn_spatial_var_direct
#endif

// ---------------------------------------------------------------- launchers (declared in crt_launch.h; DnFilter: crt_device.h)
hipError_t dn_launch_gbuffer(const DevScene &S, uint32_t x0, uint32_t y0, uint32_t tw, uint32_t th, float4 *gbuf, uint32_t *key,
                             int brute, hipStream_t stream)
{
    const uint32_t tiles_x = (tw + 7u) / 8u, tiles_y = (th + 7u) / 8u;
    if (tiles_x * tiles_y == 0) return hipSuccess;
    hipLaunchKernelGGL(k_dn_gbuffer, dim3(tiles_x * tiles_y), dim3(64), 0, stream, S, x0, y0, tw, th, tiles_x, gbuf, key, brute);
    return hipGetLastError();
}

static dim3 dn_grid16(const DnFilter &F) { return dim3((F.tw + 15u) / 16u, (F.th + 15u) / 16u); }

// (clamped to finite: 0 * inv must stay 0 for a tiny sigma)
static float dn_clamped(double v) { return (float)std::min(3.0e38, v); }

static void dn_guide_sigmas(const DnFilter &F, float &inv_n, float &inv_x)
{
    inv_n = dn_clamped(1.0 / ((double)F.sigma_normal * F.sigma_normal));
    inv_x = dn_clamped(1.0 / (double)F.sigma_plane);
}

// F.iterations passes of k_dn_atrous: the first reads `first`, each writes the buffer of F.c that it does not read
// (F.c[0] where `first` is neither), and the last also writes rgba.  Leaves the buffer that holds the result in *out.
// wave_blocks: k_dn_atrous_w64 in its place (the same bits).
static hipError_t dn_run_atrous(const DnFilter &F, float4 *first, float sigma_color, float4 **out, bool wave_blocks = false)
{
    hipError_t e = hipSuccess;
    *out = first;
    for (uint32_t i = 0; i < F.iterations && e == hipSuccess; i++) {
        DnParams P{};
        P.c_in = *out; P.c_out = F.c[*out == F.c[0] ? 1 : 0];
        P.gbuf = F.gbuf; P.key = F.key;
        P.rgba = i + 1u == F.iterations ? F.rgba : nullptr;
        P.tw = F.tw; P.th = F.th; P.step = 1u << i;
        P.inv_c = dn_clamped((double)(1u << i) / ((double)sigma_color * sigma_color));
        dn_guide_sigmas(F, P.inv_n, P.inv_x);
        if (wave_blocks) hipLaunchKernelGGL(k_dn_atrous_w64, dim3((F.tw + 7u) / 8u, (F.th + 7u) / 8u), dim3(64), 0, F.stream, P);
        else hipLaunchKernelGGL(k_dn_atrous, dn_grid16(F), dim3(256), 0, F.stream, P);
        e = hipGetLastError();
        *out = P.c_out;
    }
    return e;
}

// The two halves of the plain filter.  accum -> F.c[0] (and its rgba8 when no pass follows) ...
hipError_t dn_launch_prepare(const DnFilter &F, const float4 *accum, float n, hipStream_t stream)
{
    const size_t npix = (size_t)F.tw * F.th;
    if (npix == 0) return hipSuccess;
    hipLaunchKernelGGL(k_dn_prepare, dim3((unsigned)((npix + 255) / 256)), dim3(256), 0, stream, accum, n, F.c[0],
                       F.iterations == 0 ? F.rgba : nullptr, npix);
    return hipGetLastError();
}

// ... and the passes between F.c[0] and F.c[1], on F.stream.
hipError_t dn_launch_passes(const DnFilter &F, float sigma_color, bool wave_blocks, float4 **out)
{
    *out = F.c[0];
    if ((size_t)F.tw * F.th == 0) return hipSuccess;
    return dn_run_atrous(F, F.c[0], sigma_color, out, wave_blocks);
}

hipError_t dn_launch_filter(const DnFilter &F, const float4 *accum, float n, float sigma_color, float4 **out)
{
    *out = F.c[0];
    const hipError_t e = dn_launch_prepare(F, accum, n, F.stream);
    return e != hipSuccess ? e : dn_launch_passes(F, sigma_color, false, out);
}

// The instantiation of k_dn_reproject that P asks for: <true, *, *> where the PREVIOUS slot has a geometry snapshot,
// <*, *, true> where `counts` gives every 8x8 tile its own n (the adaptive state) in place of P.n.
template <bool MOMENTS, class Params>
static hipError_t dn_launch_reproject(const DnFilter &F, const Params &P, const uint32_t *counts)
{
    if (counts) {
        DnAdaptive<Params> A{};
        static_cast<Params &>(A) = P;
        A.counts = counts; A.tiles_x = (F.tw + 7u) / 8u;
        if (P.raw_prev) hipLaunchKernelGGL((k_dn_reproject<true, MOMENTS, true>), dn_grid16(F), dim3(256), 0, F.stream, A);
        else hipLaunchKernelGGL((k_dn_reproject<false, MOMENTS, true>), dn_grid16(F), dim3(256), 0, F.stream, A);
    } else {
        if (P.raw_prev) hipLaunchKernelGGL((k_dn_reproject<true, MOMENTS, false>), dn_grid16(F), dim3(256), 0, F.stream, P);
        else hipLaunchKernelGGL((k_dn_reproject<false, MOMENTS, false>), dn_grid16(F), dim3(256), 0, F.stream, P);
    }
    return hipGetLastError();
}

// 6l's box pass for the blend that follows: box null (option "temporal_clip_pct" off) or no PREVIOUS launches nothing and
// leaves P.box null.
template <class Params>
static hipError_t dn_launch_clip_box(const DnFilter &F, Params &P, const uint32_t *counts, float4 *box, float gamma)
{
    P.box = nullptr;
    if (!box || !P.h_prev) return hipSuccess;
    DnAdaptive<DnClipParams> A{};
    A.accum = P.accum; A.key = F.key; A.box = box;
    A.tw = F.tw; A.th = F.th; A.n = P.n; A.gamma = gamma;
    A.counts = counts; A.tiles_x = (F.tw + 7u) / 8u;
    if (counts) hipLaunchKernelGGL(k_dn_clip_box<true>, dn_grid16(F), dim3(256), 0, F.stream, A);
    else hipLaunchKernelGGL(k_dn_clip_box<false>, dn_grid16(F), dim3(256), 0, F.stream, static_cast<const DnClipParams &>(A));
    P.box = box;
    return hipGetLastError();
}

// The blend into P.h_cur, then the passes reading h_cur first and writing c[0], c[1], ... (h_cur itself stays
// unfiltered: it is the next frame's history).  counts: null, or the tile counts of the adaptive state.
// box: null, or the 2 float4 per pixel of option "temporal_clip_pct" with its factor gamma.
hipError_t dn_launch_temporal(const DnFilter &F, DnReprojParams P, const uint32_t *counts, float sigma_color, float4 *box, float gamma,
                              float4 **out)
{
    *out = P.h_cur;
    if ((size_t)F.tw * F.th == 0) return hipSuccess;
    P.rgba = F.iterations == 0 ? F.rgba : nullptr;
    hipError_t e = dn_launch_clip_box(F, P, counts, box, gamma);
    if (e == hipSuccess) e = dn_launch_reproject<false>(F, P, counts);
    return e != hipSuccess ? e : dn_run_atrous(F, P.h_cur, sigma_color, out);
}

// The film positions of P's pixels in its previous slot (P.gbuf / P.key: the slot they are asked for), tw * th float2.
hipError_t dn_launch_motion(const DnReprojParams &P, float2 *out, hipStream_t stream)
{
    if ((size_t)P.tw * P.th == 0) return hipSuccess;
    const dim3 grid((P.tw + 15u) / 16u, (P.th + 15u) / 16u);
    if (P.raw_prev) hipLaunchKernelGGL(k_dn_motion<true>, grid, dim3(256), 0, stream, P, out);
    else hipLaunchKernelGGL(k_dn_motion<false>, grid, dim3(256), 0, stream, P, out);
    return hipGetLastError();
}

// F.iterations times (k_dn_vblur into kv, k_dn_atrous_as) on the (c, v) in F.c[0], between F.c[0] and F.c[1]; the last
// launch also writes rgba and var (either may be null).  Leaves the buffer that holds the result in *out.
static hipError_t dn_run_atrous_as(const DnFilter &F, uint2 *kv, float *var, float sigma_variance, float4 **out)
{
    const uint32_t tw = F.tw, th = F.th;
    hipError_t e = hipSuccess;
    *out = F.c[0];
    for (uint32_t i = 0; i < F.iterations && e == hipSuccess; i++) {
        DnAsParams P{};
        P.c_in = F.c[i & 1u]; P.c_out = F.c[(i + 1u) & 1u];
        P.gbuf = F.gbuf; P.kv = kv;
        const bool last = i + 1u == F.iterations;
        P.rgba = last ? F.rgba : nullptr;
        P.var = last ? var : nullptr;
        P.tw = tw; P.th = th; P.step = 1u << i;
        P.sv2 = dn_clamped((double)sigma_variance * sigma_variance);
        dn_guide_sigmas(F, P.inv_n, P.inv_x);
        hipLaunchKernelGGL(k_dn_vblur, dn_grid16(F), dim3(256), 0, F.stream, P.c_in, F.key, kv, tw, th);
        e = hipGetLastError();
        if (e != hipSuccess) break;
        hipLaunchKernelGGL(k_dn_atrous_as, dn_grid16(F), dim3(256), 0, F.stream, P);
        e = hipGetLastError();
        *out = P.c_out;
    }
    return e;
}

// The adaptive state's filter: (accum, q, counts) -> c[0] with v in w, then the variance-guided passes.
hipError_t dn_launch_filter_adaptive(const DnFilter &F, const float4 *accum, const float *q, const uint32_t *counts, uint2 *kv,
                                     float *var, float sigma_variance, float4 **out)
{
    const uint32_t tw = F.tw, th = F.th;
    *out = F.c[0];
    if ((size_t)tw * th == 0) return hipSuccess;
    const bool last0 = F.iterations == 0;
    hipLaunchKernelGGL(k_dn_prepare_as, dim3((tw + 63u) / 64u, (th + 3u) / 4u), dim3(256), 0, F.stream, accum, q, counts, tw, th,
                       (tw + 7u) / 8u, F.c[0], last0 ? F.rgba : nullptr, last0 ? var : nullptr);
    const hipError_t e = hipGetLastError();
    return e != hipSuccess ? e : dn_run_atrous_as(F, kv, var, sigma_variance, out);
}

// crt_denoise_svgf: the blend into P.h_cur and the moments into P.m_cur, (c, v) into c[0], then the variance-guided passes
// (h_cur and m_cur stay unfiltered: they are the next frame's history).  counts: as dn_launch_temporal.
// spatial_b: 0, or the factor of option "svgf_spatial_pct" -- k_dn_spatial_var then rewrites the v of the pixels the moments
// do not cover before the passes read it; what stays behind in h_cur and m_cur does not depend on it.
// box, gamma: as dn_launch_temporal.
hipError_t dn_launch_svgf(const DnFilter &F, DnSvgfParams P, const uint32_t *counts, uint2 *kv, float *var, float sigma_variance,
                          float spatial_b, float4 *box, float gamma, float4 **out)
{
    *out = F.c[0];
    if ((size_t)F.tw * F.th == 0) return hipSuccess;
    const bool last0 = F.iterations == 0;
    P.rgba = last0 ? F.rgba : nullptr;
    P.var = last0 ? var : nullptr;
    P.cv = F.c[0];
    hipError_t e = dn_launch_clip_box(F, P, counts, box, gamma);
    if (e == hipSuccess) e = dn_launch_reproject<true>(F, P, counts);
    if (e == hipSuccess && spatial_b != 0.0f) {
        DnAdaptive<DnSpatialParams> A{};
        A.m_cur = P.m_cur; A.gbuf = F.gbuf; A.key = F.key;
        A.cv = P.cv; A.var = P.var;
        A.tw = F.tw; A.th = F.th;
        A.n = P.n; A.min_frames = P.min_frames; A.b = spatial_b;
        dn_guide_sigmas(F, A.inv_n, A.inv_x);
        A.counts = counts; A.tiles_x = (F.tw + 7u) / 8u;
        if (counts) hipLaunchKernelGGL(k_dn_spatial_var<true>, dn_grid16(F), dim3(256), 0, F.stream, A);
        else hipLaunchKernelGGL(k_dn_spatial_var<false>, dn_grid16(F), dim3(256), 0, F.stream, static_cast<const DnSpatialParams &>(A));
        e = hipGetLastError();
    }
    return e != hipSuccess ? e : dn_run_atrous_as(F, kv, var, sigma_variance, out);
}

}  // namespace crt
