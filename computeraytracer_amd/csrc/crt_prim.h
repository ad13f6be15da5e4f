// crt_prim.h -- per-primitive device functions shared by the GPU LBVH build (crt_lbvh.hip) and the refit
// (crt_refit.hip): the 80-byte record read, the conservative bound rule and the 48-byte leaf-ordered record.  One
// definition each, so that a refitted tree and a freshly built one cannot drift apart.
#pragma once
#include <hip/hip_runtime.h>

#include "crt_math.h"

namespace crt {

struct RawPrim { uint32_t category; f3 d1, d2, d3; uint32_t emission, reflectance, material, index; };

__device__ __forceinline__ RawPrim load_raw(const unsigned char *__restrict__ raw, size_t i)
{
    const uint4 *r = (const uint4 *)(raw + i * 80);
    const uint4 a = r[0], b = r[1], c = r[2], d = r[3], e = r[4];
    RawPrim p;
    p.category = a.x;
    p.d1 = f3{bits_f(b.x), bits_f(b.y), bits_f(b.z)};
    p.d2 = f3{bits_f(c.x), bits_f(c.y), bits_f(c.z)};
    p.d3 = f3{bits_f(d.x), bits_f(d.y), bits_f(d.z)};
    p.emission = e.x; p.reflectance = e.y; p.material = e.z; p.index = e.w;
    return p;
}

// Conservative bounds of one primitive (the rules of upload_geometry: acceptance box + 2 * hit_pad, the region a
// patch's test really accepts, a radial term for spheres; non-finite -> never culled).  Spheres read d2.x (the
// radius) only, so the leaf-ordered record (B = {r, r*r, 0, index}) gives the same box as the 80-byte one.
__device__ __forceinline__ void prim_bounds(uint32_t category, f3 d1, f3 d2, f3 d3, float pad, float l[3], float h[3])
{
    const float S = pad * 131072.0f;
    f3 cs[4];
    int nc;
    if (category == 1u) {
        const float r = abs_(d2.x);
        cs[0] = f3{d1.x - r, d1.y - r, d1.z - r}; cs[1] = f3{d1.x + r, d1.y + r, d1.z + r}; nc = 2;
    } else {
        cs[0] = d1; cs[1] = d1 + d2; cs[2] = d1 + d3; nc = 3;
        if (category == 0u) { cs[3] = cs[1] + d3; nc = 4; }
    }
    l[0] = cs[0].x; l[1] = cs[0].y; l[2] = cs[0].z; h[0] = cs[0].x; h[1] = cs[0].y; h[2] = cs[0].z;
    for (int k = 1; k < nc; k++) {
        l[0] = fminf(l[0], cs[k].x); l[1] = fminf(l[1], cs[k].y); l[2] = fminf(l[2], cs[k].z);
        h[0] = fmaxf(h[0], cs[k].x); h[1] = fmaxf(h[1], cs[k].y); h[2] = fmaxf(h[2], cs[k].z);
    }
    float g = 2.0f * pad;
    if (category == 0u) {
        const double e1[3] = {d2.x, d2.y, d2.z}, e2[3] = {d3.x, d3.y, d3.z};
        const double g11 = e1[0] * e1[0] + e1[1] * e1[1] + e1[2] * e1[2];
        const double g22 = e2[0] * e2[0] + e2[1] * e2[1] + e2[2] * e2[2];
        const double g12 = e1[0] * e2[0] + e1[1] * e2[1] + e1[2] * e2[2];
        const double det = g11 * g22 - g12 * g12;
        if (!(det > 1e-9 * g11 * g22)) {
            l[0] = l[1] = l[2] = -3.0e38f; h[0] = h[1] = h[2] = 3.0e38f;
        } else {
            const double P0[3] = {d1.x, d1.y, d1.z};
            for (int k = 0; k < 4; k++) {
                const double a = (k & 1) ? g11 : 0.0, b = (k & 2) ? g22 : 0.0;
                const double al = (a * g22 - b * g12) / det, be = (b * g11 - a * g12) / det;
                for (int ax = 0; ax < 3; ax++) {
                    const double v = P0[ax] + al * e1[ax] + be * e2[ax];
                    l[ax] = fminf(l[ax], nextafterf((float)v, -INFINITY));
                    h[ax] = fmaxf(h[ax], nextafterf((float)v, INFINITY));
                }
            }
        }
    }
    if (category == 1u) {
        const float r = fabsf(d2.x);
        g += (r > 0.0f) ? fminf(S * S * 9.5367431640625e-07f / r, S) : S;
    }
    for (int a = 0; a < 3; a++) {
        if (!(l[a] == l[a]) || !(h[a] == h[a]) || isinf(l[a]) || isinf(h[a])) { l[a] = -3.0e38f; h[a] = 3.0e38f; }
        l[a] = l[a] - g; h[a] = h[a] + g;
    }
}

// The 48-byte leaf-ordered record of a primitive (crt_device.h: A, B, C per slot) and its D vector (patches).
__device__ __forceinline__ void prim_record(const RawPrim &p, float4 &A, float4 &B, float4 &C, float4 &D)
{
    const uint32_t meta = (p.category & 3u) | ((p.material & 3u) << 2) | ((p.emission & 0x3FFFu) << 4) | ((p.reflectance & 0x3FFFu) << 18);
    A = float4{p.d1.x, p.d1.y, p.d1.z, bits_f(meta)};
    B = float4{p.d2.x, p.d2.y, p.d2.z, bits_f(p.index)};
    C = float4{p.d3.x, p.d3.y, p.d3.z, 0.0f};
    D = float4{0.0f, 0.0f, 0.0f, 0.0f};
    if (p.category == 0u) {
        const f3 nrm = normalize(cross(p.d2, p.d3));             // ComputeShader.wgsl:536
        D = float4{nrm.x, nrm.y, nrm.z, dot(p.d2, p.d2)};        // :563 denominator
        C.w = dot(p.d3, p.d3);                                   // :564 denominator
    } else if (p.category == 1u) {
        const float r = p.d2.x;                                  // :593-594
        B = float4{r, r * r, 0.0f, bits_f(p.index)};
    }
}

}  // namespace crt
