// crt_radiance.hip -- radiance queries (include/crt.h, crt_radiance_rays / crt_radiance_rays_device): "here are my rays,
// how much light arrives along them?".  The reference's path_trace (ComputeShader.wgsl:119-295) from caller rays, each
// with a key (x, y, first sample) that seeds its paths as the reference seeds a pixel's.  A kernel of its own beside the
// path tracer: it reads the scene, the lights, the spectra tables and the tree and writes the caller's planes; nothing of
// the pipeline's state is involved.  DESIGN.md 6q has the definition this follows.
//
// The path loop is k_trace's (crt_kernels.hip) RESTATED -- same operations, same draw order; a change in one is made in
// the other -- with the single-ray walks k_wf_finish and k_query use (crt_shade.h, finish_walk_*).
#include "crt_launch.h"
#include "crt_shade.h"

namespace crt {

// 64-thread blocks, k_query's LDS stack (kStackDepth x 64 entries, lane i on column i).  Ownership is static: lane g of
// the G = 64 * gridDim.x lanes owns rays g, g + G, g + 2G, ... -- no atomic, no counter in device memory, no barrier, and a
// lane touches its own rays and their outputs only, so a ray's output is a function of its record, its key and n_samples.
//
// Per ray the loops are k_trace's, nested: for samples { for (;;) path }, the path a two-state loop (extension ray, shadow
// ray) around one traversal SITE in the code.  That site is not one converged walk: a lane with a shadow ray takes
// finish_walk_shadow, a lane with an extension ray finish_walk_extension, and a wave that holds both runs the two walks one
// after the other (as k_wf_finish does).  A flat form -- one loop per lane whose states also cover "next sample, or next
// ray", so that a lane never waits for its wave's longest path -- was built first and measured 15-17 % slower than this one
// at one ray per lane: the wave re-enters the sample's set-up for any one lane at almost every trip.
//
// Termination.  A path traces at most kMaxDepthPath + 1 extension rays (the depth test ends it) and at most one shadow
// ray per extension ray; a ray has n_samples paths; a lane's ray index grows by G > 0 per ray and the lane leaves when it
// reaches n.
//
// BRUTE: CRT_ACCEL_NONE, the reference's loop over every primitive for every ray.  Without it a bounce ray that has
// become non-finite gets that loop too, in line (as k_query: a call of intersect_all would put the scene into scratch).
template <bool BRUTE>
__global__ __launch_bounds__(64) void k_radiance(const DevScene S, const RadianceParams P)
{
    __shared__ int lds_stack[BRUTE ? 64 : kStackDepth * 64];
    int *stk = lds_stack + threadIdx.x;
    const size_t G = (size_t)gridDim.x * 64u;
    const bool wide = P.wide_ok && finish_walks_wide(S);

    enum { kExt = 1, kShadow = 2 };
    for (size_t i = (size_t)blockIdx.x * 64u + threadIdx.x; i < P.n; i += G) {
    const float4 r0 = P.rays[2 * i], r1 = P.rays[2 * i + 1];
    const f3 c_o = f3{r0.x, r0.y, r0.z}, c_d = f3{r1.x, r1.y, r1.z};
    if (!finite3(c_o) || !finite3(c_d)) {                       // never walked: zeros in every plane (crt_query_rays' rule)
        if (P.xyz) P.xyz[i] = float4{0.0f, 0.0f, 0.0f, 0.0f};
        if (P.y2) P.y2[i] = 0.0f;
        if (P.rgba8) P.rgba8[i] = uchar4{0, 0, 0, 0};
        continue;
    }
    uint32_t kx = (uint32_t)i, ky = 0u, ks = 1u;
    if (P.keys) { const uint4 k = P.keys[i]; kx = k.x; ky = k.y; ks = k.z; }
    const uint32_t tea_xy = tea(kx, ky * 100u);
    f3 sum = f3{0, 0, 0};
    float qy = 0.0f;
    for (uint32_t j = 0; j < P.n_samples; j++) {
        // seeded as a pixel's sample (:98), the camera's two jitter draws made and dropped
        Rng rng = Rng{ky, kx * 100u, ks + j, tea_xy};
        (void)rnd(rng);
        (void)rnd(rng);
        uint32_t wl[4];
        {                                                        // sample_wavelengths :315-322
            float u = rnd(rng);
            uint32_t lambda = (uint32_t)(301.0f * u);
            wl[0] = lambda; wl[1] = (lambda + 4u) % kNLambda; wl[2] = (lambda + 8u) % kNLambda;
            wl[3] = (lambda + 12u) % kNLambda;
        }
        // path_trace :119-295 (k_trace's names)
        int state = kExt;
        uint32_t depth = 0;
        f4 radiance = f4{0, 0, 0, 0}, beta = f4{1, 1, 1, 1};
        float last_bounce_pdf = 1.0f;
        f3 ray_o = c_o, ray_d = c_d;
        float limit = r0.w;                                      // the extension ray's t_max: the caller's on the first segment
        uint32_t exclude = f_bits(r1.w);
        bool specular_bounce = false;
        float etaScale = 1.0f;
        bool inTransmission = false;
        f3 s_pos = f3{0, 0, 0}, s_nrm = f3{0, 0, 0}, s_ldir = f3{0, 0, 0};
        f4 s_brdf = f4{0, 0, 0, 0};
        uint32_t s_light = 0, s_index = 0;
        for (;;) {
        // ---- the ray this lane traces now: the one traversal site
        const bool shadow_mode = state == kShadow;
        const f3 o = shadow_mode ? s_pos : ray_o;
        const f3 d = shadow_mode ? s_ldir : ray_d;
        const uint32_t excl = shadow_mode ? s_index : exclude;
        float t_max = shadow_mode ? CRT_INFINITY : limit;
        uint32_t b_index = kNoHit, b_slot = kNoHit, cn = 0, cp = 0;
        bool light_seen = false;
        if (BRUTE || !finite3(o) || !finite3(d)) {
            // intersect_all's loop, in line.  (A caller ray is finite here, so a NaN or negative limit, which the literal
            // test would let through, can only meet it under BRUTE.)
            if (t_max >= 0.0f)
                for (uint32_t k = 0; k < S.nprim; k++)
                    hit_test<true>(S, S.slot_of_index[k], o, d, excl, 0.001f, t_max, b_index, b_slot);
            if (shadow_mode) light_seen = (b_slot != kNoHit && b_index == f_bits(S.lights[3 * s_light + 1].w));   // :700
        } else if (shadow_mode) {
            // shadow_intersect (:697-705) == "is the light's own primitive the closest hit?": hit the light first, then
            // ask the tree for anything that beats it (k_trace's and k_wf_finish's priming)
            const uint32_t include = f_bits(S.lights[3 * s_light + 1].w);
            if (include < S.nprim) hit_test<false>(S, S.slot_of_index[include], o, d, excl, 0.001f, t_max, b_index, b_slot);
            if (b_slot != kNoHit) {
                uint32_t how;
                light_seen = finish_walk_shadow<false>(S, stk, wide, o, d, excl, t_max, include, cn, cp, how);
            }
        } else if (t_max >= 0.0f) {                             // (a NaN or negative limit can never be beaten: a miss)
            uint32_t how;
            finish_walk_extension<false>(S, stk, wide, o, d, excl, t_max, b_index, b_slot, cn, cp, how);
        }
        limit = CRT_INFINITY;                                    // (the caller's limit bears on the first segment only)

        bool diffuse_tail = false, ended = false;
        f4 nee = f4{0, 0, 0, 0};
        f3 h_pos = s_pos, h_nrm = s_nrm;

        if (shadow_mode) {
            // ---- compute_light_radiance tail :388-407
            if (light_seen) {
                f3 lp, ln; uint32_t lmeta;
                hit_attributes(S, b_slot, o, d, t_max, lp, ln, lmeta);
                float cos_theta = max_(0.0f, dot(s_nrm, s_ldir));
                f4 spec = sample_spectrum(S, f_bits(S.lights[3 * s_light + 0].w), wl);
                f4 le = spec * cos_theta;
                float pdf_l = compute_light_pdf(S, (lmeta >> 4) & 0x3FFFu, lp, ln, o, d);
                float pdf_b = cos_theta / CRT_PI;
                float weight_l = power_heuristic(1.0f, pdf_l, 1.0f, pdf_b);
                nee = (le * weight_l) / pdf_l;
            }
            state = kExt;
            diffuse_tail = true;
        } else if (b_slot == kNoHit) {                          // :141
            ended = true;
        } else {
            f3 pos, nrm; uint32_t meta;
            hit_attributes(S, b_slot, o, d, t_max, pos, nrm, meta);
            exclude = b_index;                                   // :146
            const uint32_t material = (meta >> 2) & 3u;
            const uint32_t emission_index = (meta >> 4) & 0x3FFFu;
            const uint32_t reflectance_index = (meta >> 18) & 0x3FFFu;
            if (material == kLight) {                            // :149-164
                f4 le = sample_spectrum(S, emission_index, wl);
                if (depth == 0 || specular_bounce) {
                    radiance = radiance + beta * le;
                } else {
                    float pdf_l = compute_light_pdf(S, emission_index, pos, nrm, o, d);
                    float weight_b = power_heuristic(1.0f, last_bounce_pdf, 1.0f, pdf_l);
                    radiance = radiance + (le * weight_b) * beta;
                }
                ended = true;
            } else if (depth >= kMaxDepthPath) {                 // :167
                ended = true;
            } else {
                if (inTransmission) {                            // :173-179
                    float distance = length(o - pos);
                    f4 ext = sample_spectrum(S, S.nspectra - 1u, wl);
                    f4 att = f4{exp_(-ext.x * distance), exp_(-ext.y * distance), exp_(-ext.z * distance),
                                exp_(-ext.w * distance)};
                    beta = beta * att;
                }
                if (material == kDiffuse) {                      // :182-204, first half
                    s_brdf = sample_spectrum(S, reflectance_index, wl) / CRT_PI;
                    // sample_lights :341-347, sample_light :349-355
                    float u0 = rnd(rng);
                    uint32_t li = (uint32_t)((float)S.nlight * u0);
                    if (li >= S.nlight) li = S.nlight - 1u;
                    float u = rnd(rng);
                    float v = rnd(rng);
                    f3 l1 = xyz(S.lights[3 * li + 0]), l2 = xyz(S.lights[3 * li + 1]), l3 = xyz(S.lights[3 * li + 2]);
                    f3 pl = (l1 + l2 * u) + l3 * v;
                    s_ldir = normalize(pl - pos);
                    s_pos = pos; s_nrm = nrm; s_light = li; s_index = b_index;
                    state = kShadow;
                    continue;                                    // trace the shadow ray
                }
                if (material == kGlass) {                        // :208-276
                    const float eta1 = 1.0f, eta2 = 1.5f;
                    float eta = eta1 / eta2;
                    float cos_theta = dot(nrm, ray_d);
                    float reflected = fresnel_s(ray_d, nrm, eta1, eta2);
                    float pr = reflected;
                    float pt = 1.0f - reflected;
                    float u = rnd(rng);
                    f3 current_normal = nrm;
                    if (cos_theta > 0.0f) { eta = 1.0f / eta; current_normal = -current_normal; }
                    f3 new_direction;
                    if (u < pr / (pr + pt)) {                    // :238
                        new_direction = reflect_(ray_d, current_normal);
                    } else {
                        new_direction = normalize(refract_(ray_d, current_normal, eta));
                        beta = beta * (eta * eta);
                        etaScale = etaScale / (eta * eta);
                        inTransmission = !inTransmission;
                    }
                    ray_o = pos;
                    specular_bounce = true;
                    exclude = 0xFFFFFFFFu;
                    ray_d = new_direction;
                }
                h_pos = pos; h_nrm = nrm;
            }
        }

        if (!ended) {
            if (diffuse_tail) {                                  // :187-195
                radiance = radiance + (s_brdf * nee) * beta;
                f3 new_direction = cosine_hemisphere(rng, h_nrm, last_bounce_pdf);
                float cos_theta = abs_(dot(h_nrm, new_direction));
                beta = beta * ((s_brdf * cos_theta) / last_bounce_pdf);
                ray_o = h_pos;
                ray_d = new_direction;
                specular_bounce = false;
            }
            // Russian roulette :279-289
            f4 rbeta = beta * etaScale;
            float max_beta_component = max_(rbeta.x, max_(rbeta.y, rbeta.z));
            if (depth > 1u && max_beta_component < 1.0f) {
                float qq = max_(0.0f, 1.0f - max_beta_component);
                if (rnd(rng) < qq) ended = true;
                else beta = beta / (1.0f - qq);
            }
            depth++;
        }
        if (ended) break;
        }
        const f3 c = spectral_to_xyz(S, radiance, wl);
        sum = sum + c;                                           // :108
        qy = qy + c.y * c.y;                                     // DESIGN.md 6c's second moment
    }
    // the ray's only stores
    if (P.xyz) P.xyz[i] = float4{sum.x, sum.y, sum.z, 0.0f};
    if (P.y2) P.y2[i] = qy;
    if (P.rgba8) P.rgba8[i] = tonemap_rgba8(sum, (float)P.n_samples);
    }
}

uint32_t radiance_blocks(size_t n, uint32_t num_cu)
{
    const size_t want = (n + 63) / 64, cap = (size_t)num_cu * kRadianceWavesPerCu;
    return (uint32_t)(want < cap ? want : cap);
}

hipError_t radiance_launch(const DevScene &S, const RadianceParams &P, bool brute, uint32_t num_cu, hipStream_t stream)
{
    if (P.n == 0) return hipSuccess;
    if (P.n > 0xFFFFFFFFull || P.n_samples == 0 || num_cu == 0) return hipErrorInvalidValue;
    const dim3 grid(radiance_blocks(P.n, num_cu));
    if (brute) hipLaunchKernelGGL((k_radiance<true>), grid, dim3(64), 0, stream, S, P);
    else hipLaunchKernelGGL((k_radiance<false>), grid, dim3(64), 0, stream, S, P);
    return hipGetLastError();
}

}  // namespace crt
