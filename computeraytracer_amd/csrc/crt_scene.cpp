// crt_scene.cpp -- the scene on the device: record unpacking, the acceleration trees (host SAH or GPU LBVH build, the
// 4- and 8-wide forms), and the edits that keep a built scene alive: camera, primitives, lights, the refit.
#include "crt_ctx.h"

using namespace crt;

namespace crt {

HostPrim read_prim(const uint8_t *base, size_t i)
{
    HostPrim p;
    const uint8_t *r = base + i * 80;
    float f[9];
    uint32_t u[4];
    std::memcpy(&p.category, r, 4);
    std::memcpy(f, r + 16, 12); std::memcpy(f + 3, r + 32, 12); std::memcpy(f + 6, r + 48, 12);
    std::memcpy(u, r + 64, 16);
    p.d1 = f3{f[0], f[1], f[2]}; p.d2 = f3{f[3], f[4], f[5]}; p.d3 = f3{f[6], f[7], f[8]};
    p.emission = u[0]; p.reflectance = u[1]; p.material = u[2]; p.index = u[3];
    return p;
}

// Primitive corners for bounds / scene scale (same op order as the oracle's orc_hit_pad).
static int prim_corners(const HostPrim &p, f3 out[4])
{
    if (p.category == 1u) {
        float r = abs_(p.d2.x);
        out[0] = f3{p.d1.x - r, p.d1.y - r, p.d1.z - r};
        out[1] = f3{p.d1.x + r, p.d1.y + r, p.d1.z + r};
        return 2;
    }
    out[0] = p.d1; out[1] = p.d1 + p.d2; out[2] = p.d1 + p.d3;
    if (p.category == 0u) { out[3] = out[1] + p.d3; return 4; }
    return 3;
}

// scene_hit_pad in two steps: the primitives' part (cached as crt_ctx::s_prims; k_refit_pad on the device) and the eye's.
float prims_scale(const std::vector<HostPrim> &prims)
{
    float S = 0.0f;
    f3 c[4];
    for (const HostPrim &p : prims) {
        int nc = prim_corners(p, c);
        for (int k = 0; k < nc; k++) {
            S = max_(S, abs_(c[k].x)); S = max_(S, abs_(c[k].y)); S = max_(S, abs_(c[k].z));
        }
    }
    return S;
}

float pad_of(float S, const float cam[16])
{
    S = max_(S, abs_(cam[0])); S = max_(S, abs_(cam[1])); S = max_(S, abs_(cam[2]));
    return S * 7.62939453125e-06f;  // 2^-17
}

// The host copy of the primitives again as the device holds them, after crt_transform_primitives moved records there.
// Called before anything reads geometry from c->prims: the host builders and record packing of upload_geometry (and
// prims_scale, should a caller of it appear that runs after an edit).
static int refresh_prims(crt_ctx *c)
{
    if (!c->prims_moved) return CRT_OK;
    const size_t n = c->prims.size();
    std::vector<uint8_t> raw(n * 80);
    if (n) {
        HIPCHK(c, hipMemcpyAsync(raw.data(), c->d_raw.p, n * 80, hipMemcpyDeviceToHost, c->stream));
        HIPCHK(c, hipStreamSynchronize(c->stream));
    }
    for (size_t i = 0; i < n; i++) c->prims[i] = read_prim(raw.data(), i);
    c->prims_moved = false;
    return CRT_OK;
}

// The device rows of one light record (crt_upload_scene, crt_update_lights).
void light_rows(const HostPrim &l, float4 out[3])
{
    float light_area = length(l.d2) * length(l.d3);              // :363
    out[0] = float4{l.d1.x, l.d1.y, l.d1.z, bits_f(l.emission)};
    out[1] = float4{l.d2.x, l.d2.y, l.d2.z, bits_f(l.index)};
    out[2] = float4{l.d3.x, l.d3.y, l.d3.z, 1.0f / light_area};       // :364
}

// ComputeShader.wgsl:470-487, everything independent of the pixel.
void camera_frame(const float cam[16], float out[12])
{
    f3 eye = f3{cam[0], cam[1], cam[2]}, lookat = f3{cam[4], cam[5], cam[6]}, up = f3{cam[8], cam[9], cam[10]};
    f3 w = normalize(eye - lookat);
    f3 u = normalize(cross(up, w));
    f3 v = cross(w, u);
    float aspect_ratio = cam[11] / cam[12];
    float viewport_height = 2.0f * tan_(cam[13] / 2.0f);
    float viewport_width = aspect_ratio * viewport_height;
    f3 horizontal = u * viewport_width;
    f3 vertical = v * viewport_height;
    f3 llc = ((eye - horizontal / 2.0f) - vertical / 2.0f) - w;
    out[0] = llc.x; out[1] = llc.y; out[2] = llc.z;
    out[3] = horizontal.x; out[4] = horizontal.y; out[5] = horizontal.z;
    out[6] = vertical.x; out[7] = vertical.y; out[8] = vertical.z;
    out[9] = eye.x; out[10] = eye.y; out[11] = eye.z;
}

// crt_build_accel(CRT_ACCEL_LBVH), all on the device (crt_lbvh.hip): bounds, Morton order, hierarchy, collapse to the
// 4-wide tree, quantisation and the leaf-ordered primitive records; nothing of the tree visits the host.  Returns
// CRT_OK with *done = false when the scene cannot take this path (not quantisable): the caller builds the host way.
//
// CRT_ACCEL_PLOC takes the same route with the clustered hierarchy (crt_ploc.hip).  A PLOC build that is abandoned (deeper
// than the single-ray stacks allow, or not finished within the rounds limit) leaves a note in crt_last_error and the
// same call builds the Karras LBVH instead.
static void ploc_abandoned_note(crt_ctx *c, const PlocInfo &info)
{
    if (info.abandoned == 1)
        (void)fail(c, CRT_OK, "crt_build_accel: the PLOC hierarchy is %u levels deep, more than the %u the walk's stacks allow; built the LBVH instead",
                   info.depth, c->ploc.max_depth);
    else
        (void)fail(c, CRT_OK, "crt_build_accel: the PLOC build had not finished after %u rounds (the limit); built the LBVH instead", info.rounds);
}

static int build_accel_on_device(crt_ctx *c, bool *done)
{
    *done = false;
    const uint32_t n = (uint32_t)c->prims.size();
    if (n < 2 || !c->quantize || c->wf_width != 4 || c->d_raw.n < (size_t)n * 80) return CRT_OK;
    HIPCHK(c, c->d_prim.alloc((size_t)n * 3));
    HIPCHK(c, c->d_primD.alloc(n));
    HIPCHK(c, c->d_slot_of_index.alloc(n));
    HIPCHK(c, c->d_nodes.alloc((size_t)(n - 1) * 4));
    HIPCHK(c, c->d_nodes4q.alloc((size_t)(n - 1) * 4));
    HIPCHK(c, c->d_nodes4.alloc(8));
    LbvhDeviceResult res;
    int builder = 1;
    if (c->want_builder == 2) {
        PlocInfo info;
        const hipError_t e = build_ploc_device(c->d_raw.p, n, c->sc.hit_pad, c->ploc, c->d_prim.p, c->d_primD.p, c->d_slot_of_index.p,
                                               (float *)c->d_nodes.p, c->d_nodes4q.p, res, info, c->stream);
        if (e != hipSuccess) return fail(c, e == hipErrorOutOfMemory ? CRT_ENOMEM : CRT_EDEVICE, "crt_build_accel: GPU PLOC build: %s", hipGetErrorString(e));
        if (info.abandoned) ploc_abandoned_note(c, info);
        else builder = 2;
    }
    if (builder == 1) {
        const hipError_t e = build_lbvh_device(c->d_raw.p, n, c->sc.hit_pad, c->d_prim.p, c->d_primD.p, c->d_slot_of_index.p,
                                               (float *)c->d_nodes.p, c->d_nodes4q.p, res, c->stream);
        if (e != hipSuccess) return fail(c, e == hipErrorOutOfMemory ? CRT_ENOMEM : CRT_EDEVICE, "crt_build_accel: GPU LBVH build: %s", hipGetErrorString(e));
    }
    if (!res.quantised) return CRT_OK;
    // the host keeps the tree's statistics only
    c->bvh = Bvh(); c->bvh4 = Bvh4(); c->bvh4q = Bvh4Q(); c->bvh8q = Bvh8Q();
    c->bvh.root = 0; c->bvh.n_inner = n - 1; c->bvh.n_leaves = n; c->bvh.max_depth = res.max_depth;
    c->bvh4.root = 0; c->bvh4.n_inner = res.n_nodes4; c->bvh4.max_depth = res.depth4;
    c->bvh4q.ok = true;
    for (int a = 0; a < 3; a++) { c->bvh4q.base[a] = res.qbase[a]; c->bvh4q.scale[a] = res.qscale[a]; c->sc.qbase[a] = res.qbase[a]; c->sc.qscale[a] = res.qscale[a]; }
    c->accel_builder = builder;
    c->sc.prim = c->d_prim.p; c->sc.primD = c->d_primD.p; c->sc.slot_of_index = c->d_slot_of_index.p;
    c->sc.nodes = c->d_nodes.p; c->sc.root = 0;
    c->sc.nodes4 = c->d_nodes4.p; c->sc.root4 = 0; c->sc.n_nodes4 = res.n_nodes4;
    c->sc.nodes4q = c->d_nodes4q.p;
    c->sc.nodes8q = nullptr; c->sc.root8 = -1;
    c->sc.nprim = n;
    c->sc.npatch = 0;
    for (const HostPrim &hp_ : c->prims) c->sc.npatch += hp_.category == 0u ? 1u : 0u;
    c->accel_mode = CRT_ACCEL_BVH2;
    *done = true;
    return CRT_OK;
}

// Builds the device primitive arrays in `order` and (for BVH2) the node array.
static int upload_geometry(crt_ctx *c, int mode)
{
    const uint32_t n = (uint32_t)c->prims.size();
    const float pad = c->sc.hit_pad;
    if (mode == CRT_ACCEL_BVH2 && c->want_builder != 0) {
        bool done = false;
        int rc = build_accel_on_device(c, &done);
        if (rc || done) return rc;
    }
    CRT_TRY(refresh_prims(c));            // (the device build above reads d_raw itself)
    std::vector<uint32_t> order;
    c->bvh = Bvh();
    if (mode == CRT_ACCEL_BVH2 && n > 0) {
        // Conservative boxes: the triangle acceptance box is [corner min - pad, corner max + pad];
        // node boxes get 2*pad (covers the slab arithmetic), spheres an extra radial term.
        float S = pad * 131072.0f;
        std::vector<float> lo((size_t)n * 3), hi((size_t)n * 3);
        f3 cs[4];
        for (uint32_t i = 0; i < n; i++) {
            const HostPrim &p = c->prims[i];
            int nc = prim_corners(p, cs);
            float l[3] = {cs[0].x, cs[0].y, cs[0].z}, h[3] = {cs[0].x, cs[0].y, cs[0].z};
            for (int k = 1; k < nc; k++) {
                l[0] = std::min(l[0], cs[k].x); l[1] = std::min(l[1], cs[k].y); l[2] = std::min(l[2], cs[k].z);
                h[0] = std::max(h[0], cs[k].x); h[1] = std::max(h[1], cs[k].y); h[2] = std::max(h[2], cs[k].z);
            }
            float g = 2.0f * pad;
            if (p.category == 0u) {
                // The patch test accepts {P0+m : 0<=m.e1<=e1.e1, 0<=m.e2<=e2.e2} (ComputeShader.wgsl
                // :563-566 use projections, which only equals the corner parallelogram when e1 is
                // perpendicular to e2 -- cornell's box faces are not).  Bound THAT region.
                double e1[3] = {p.d2.x, p.d2.y, p.d2.z}, e2[3] = {p.d3.x, p.d3.y, p.d3.z};
                double g11 = e1[0] * e1[0] + e1[1] * e1[1] + e1[2] * e1[2];
                double g22 = e2[0] * e2[0] + e2[1] * e2[1] + e2[2] * e2[2];
                double g12 = e1[0] * e2[0] + e1[1] * e2[1] + e1[2] * e2[2];
                double det = g11 * g22 - g12 * g12;
                if (!(det > 1e-9 * g11 * g22)) {
                    l[0] = l[1] = l[2] = -3.0e38f; h[0] = h[1] = h[2] = 3.0e38f;   // unbounded strip
                } else {
                    double P0[3] = {p.d1.x, p.d1.y, p.d1.z};
                    for (int k = 0; k < 4; k++) {
                        double a = (k & 1) ? g11 : 0.0, b = (k & 2) ? g22 : 0.0;
                        double al = (a * g22 - b * g12) / det, be = (b * g11 - a * g12) / det;
                        for (int ax = 0; ax < 3; ax++) {
                            double v = P0[ax] + al * e1[ax] + be * e2[ax];
                            l[ax] = std::min(l[ax], (float)std::nextafter((float)v, -INFINITY));
                            h[ax] = std::max(h[ax], (float)std::nextafter((float)v, INFINITY));
                        }
                    }
                }
            }
            if (p.category == 1u) {
                float r = std::fabs(p.d2.x);
                g += (r > 0.0f) ? std::min(S * S * 9.5367431640625e-07f / r, S) : S;
            }
            for (int a = 0; a < 3; a++) {
                if (!(l[a] == l[a]) || !(h[a] == h[a]) || std::isinf(l[a]) || std::isinf(h[a])) {
                    l[a] = -3.0e38f; h[a] = 3.0e38f;      // non-finite primitive: never culled
                }
                lo[3 * i + a] = l[a] - g; hi[3 * i + a] = h[a] + g;
            }
        }
        c->accel_builder = 0;
        if (c->want_builder != 0 && n >= 2) {
            // GPU build (crt_lbvh.hip, crt_ploc.hip): same structure, so everything below is shared
            int builder = 1;
            if (c->want_builder == 2) {
                PlocInfo info;
                hipError_t e = build_ploc(lo.data(), hi.data(), n, c->ploc, c->bvh, info, c->stream);
                if (e != hipSuccess) return fail(c, e == hipErrorOutOfMemory ? CRT_ENOMEM : CRT_EDEVICE, "crt_build_accel: GPU PLOC build: %s", hipGetErrorString(e));
                if (info.abandoned) ploc_abandoned_note(c, info);
                else builder = 2;
            }
            if (builder == 1) {
                hipError_t e = build_lbvh(lo.data(), hi.data(), n, c->bvh, c->stream);
                if (e != hipSuccess) return fail(c, e == hipErrorOutOfMemory ? CRT_ENOMEM : CRT_EDEVICE, "crt_build_accel: GPU LBVH build: %s", hipGetErrorString(e));
            }
            c->accel_builder = builder;
        } else {
            build_bvh2(lo.data(), hi.data(), n, c->bvh);
        }
        order = c->bvh.order;
    } else {
        order.resize(n);
        for (uint32_t i = 0; i < n; i++) order[i] = i;
        c->bvh.root = -1;
    }

    std::vector<float4> hp((size_t)n * 3), hd(n);
    std::vector<uint32_t> slot_of(n);
    for (uint32_t slot = 0; slot < n; slot++) {
        const HostPrim &p = c->prims[order[slot]];
        slot_of[p.index] = slot;
        uint32_t meta = (p.category & 3u) | ((p.material & 3u) << 2) | ((p.emission & 0x3FFFu) << 4) |
                        ((p.reflectance & 0x3FFFu) << 18);
        float4 A = {p.d1.x, p.d1.y, p.d1.z, bits_f(meta)};
        float4 B = {p.d2.x, p.d2.y, p.d2.z, bits_f(p.index)};
        float4 C = {p.d3.x, p.d3.y, p.d3.z, 0.0f};
        float4 D = {0.0f, 0.0f, 0.0f, 0.0f};
        if (p.category == 0u) {
            f3 nrm = normalize(cross(p.d2, p.d3));               // ComputeShader.wgsl:536
            D = float4{nrm.x, nrm.y, nrm.z, dot(p.d2, p.d2)};    // :563 denominator
            C.w = dot(p.d3, p.d3);                               // :564 denominator
        } else if (p.category == 1u) {
            float r = p.d2.x;                                    // :593-594
            B = float4{r, r * r, 0.0f, bits_f(p.index)};
        }
        hp[3 * (size_t)slot + 0] = A; hp[3 * (size_t)slot + 1] = B; hp[3 * (size_t)slot + 2] = C;
        hd[slot] = D;
    }
    HIPCHK(c, c->d_prim.alloc(std::max<size_t>(hp.size(), 3)));
    HIPCHK(c, c->d_primD.alloc(std::max<size_t>(hd.size(), 1)));
    HIPCHK(c, c->d_slot_of_index.alloc(std::max<size_t>(n, 1)));
    if (n) {
        HIPCHK(c, hipMemcpy(c->d_prim.p, hp.data(), hp.size() * sizeof(float4), hipMemcpyHostToDevice));
        HIPCHK(c, hipMemcpy(c->d_primD.p, hd.data(), hd.size() * sizeof(float4), hipMemcpyHostToDevice));
        HIPCHK(c, hipMemcpy(c->d_slot_of_index.p, slot_of.data(), n * sizeof(uint32_t), hipMemcpyHostToDevice));
    }
    size_t nn = c->bvh.nodes.size() / 4;
    HIPCHK(c, c->d_nodes.alloc(std::max<size_t>(nn, 4)));
    if (nn) HIPCHK(c, hipMemcpy(c->d_nodes.p, c->bvh.nodes.data(), nn * sizeof(float4), hipMemcpyHostToDevice));
    c->sc.prim = c->d_prim.p;
    c->sc.primD = c->d_primD.p;
    c->sc.slot_of_index = c->d_slot_of_index.p;
    c->bvh4 = Bvh4();
    if (mode == CRT_ACCEL_BVH2 && n > 0) collapse_bvh4(c->bvh, c->bvh4);
    size_t nn4 = c->bvh4.nodes.size() / 4;
    HIPCHK(c, c->d_nodes4.alloc(std::max<size_t>(nn4, 8)));
    if (nn4) HIPCHK(c, hipMemcpy(c->d_nodes4.p, c->bvh4.nodes.data(), nn4 * sizeof(float4), hipMemcpyHostToDevice));
    c->sc.nodes4 = c->d_nodes4.p;
    c->sc.root4 = c->bvh4.root;
    c->sc.n_nodes4 = c->bvh4.n_inner;
    c->bvh4q = Bvh4Q();
    c->sc.nodes4q = nullptr;
    if (c->quantize && c->bvh4.n_inner) quantize_bvh4(c->bvh4, c->bvh4q);
    if (c->bvh4q.ok) {
        size_t nq = c->bvh4q.nodes.size() / 4;
        HIPCHK(c, c->d_nodes4q.alloc(nq));
        HIPCHK(c, hipMemcpy(c->d_nodes4q.p, c->bvh4q.nodes.data(), nq * sizeof(uint4), hipMemcpyHostToDevice));
        c->sc.nodes4q = c->d_nodes4q.p;
        for (int a = 0; a < 3; a++) { c->sc.qbase[a] = c->bvh4q.base[a]; c->sc.qscale[a] = c->bvh4q.scale[a]; }
    }
    c->bvh8q = Bvh8Q();
    c->sc.nodes8q = nullptr;
    c->sc.root8 = -1;
    if (c->quantize && c->wf_width == 8 && c->bvh4q.ok) build_bvh8q(c->bvh, c->bvh8q);
    if (c->bvh8q.ok) {
        const size_t nq = c->bvh8q.nodes.size() / 4;
        HIPCHK(c, c->d_nodes8q.alloc(nq));
        HIPCHK(c, hipMemcpy(c->d_nodes8q.p, c->bvh8q.nodes.data(), nq * sizeof(uint4), hipMemcpyHostToDevice));
        c->sc.nodes8q = c->d_nodes8q.p;
        c->sc.root8 = c->bvh8q.root;
        for (int a = 0; a < 3; a++) { c->sc.qbase[a] = c->bvh8q.base[a]; c->sc.qscale[a] = c->bvh8q.scale[a]; }
    }
    c->sc.nodes = c->d_nodes.p;
    c->sc.root = c->bvh.root;
    c->sc.nprim = n;
    c->sc.npatch = 0;
    for (const HostPrim &hp_ : c->prims) c->sc.npatch += hp_.category == 0u ? 1u : 0u;
    c->accel_mode = mode;
    return CRT_OK;
}

// The stacks of the wavefront walks ("Stack capacity"): a nearest-first walk holds at most
// (node width - 1) entries per inner level of the walked tree.
uint32_t wf_stack_need(const crt_ctx *c) { return (c->bvh8q.ok ? 7u : 3u) * c->wf_depth; }
// LDS stack entries per lane of the kernel wf_launch_trace picks (wf_trace_kernel: k_wf_trace2 for the quantised 4-wide tree under form 2)
uint32_t wf_stack_lds(const crt_ctx *c) { return (c->wf_trace_form == 2 && c->bvh4q.ok && !c->bvh8q.ok) ? (uint32_t)kWfStackLds2 : (uint32_t)kWfStackLds; }
uint32_t wf_overflow_levels(const crt_ctx *c)
{
    const uint32_t need = wf_stack_need(c), lds = wf_stack_lds(c);
    return std::max(kWfOverflowLevels, need > lds ? need - lds : 0u);
}

// upload_geometry plus the scene-edit bookkeeping: a new tree is fresh, its boxes made with the current hit_pad.
// Also records the depth of the tree the wavefront kernels walk, and builds the SAH tree instead of an LBVH too deep for
// a reasonable stack overflow area.
int build_tree(crt_ctx *c, int mode)
{
    c->rf_ready = false;
    c->q_built_ok = false;
    c->refits = 0;
    c->wf_depth = 0;
    int rc = upload_geometry(c, mode);
    if (rc == CRT_OK && mode == CRT_ACCEL_BVH2) {
        c->wf_depth = c->bvh8q.ok ? c->bvh8q.max_depth : c->bvh4.max_depth;
        // ("wf_trace_form" may change after the build: judged with the fewest LDS entries a kernel for this tree has)
        const uint32_t lds_min = c->bvh4q.ok && !c->bvh8q.ok ? (uint32_t)kWfStackLds2 : (uint32_t)kWfStackLds;
        if (c->accel_builder != 0 && wf_stack_need(c) > lds_min + kWfOverflowMaxLevels) {
            // a GPU-built tree this deep would need an unreasonable overflow area: the SAH builder's tree is at most 30 levels deep
            const uint32_t depth = c->wf_depth, width = c->bvh8q.ok ? 8u : 4u;
            const int wanted = c->want_builder;
            const char *made = c->accel_builder == 2 ? "PLOC tree" : "LBVH";
            c->want_builder = 0; c->accel_mode = -1;
            rc = upload_geometry(c, mode);
            c->want_builder = wanted;                            // (a rebuild by crt_refit_accel tries the GPU builder again)
            if (rc == CRT_OK) {
                c->wf_depth = c->bvh8q.ok ? c->bvh8q.max_depth : c->bvh4.max_depth;
                (void)fail(c, CRT_OK, "crt_build_accel: the %u-wide %s is %u levels deep (its walk would need %u stack entries per lane, "
                                      "more than %u + %u); built with the host SAH builder instead (%u levels)",
                           width, made, depth, (width - 1u) * depth, lds_min, kWfOverflowMaxLevels, c->wf_depth);
            }
        }
    }
    if (rc == CRT_OK) { c->accel_stale = false; c->accel_topo = false; c->tree_pad = c->sc.hit_pad; }
    return rc;
}

}  // namespace crt

extern "C" {

// ---------------------------------------------------------------- scene edits (crt_refit.hip)
// Every edit call starts as a sync point (quiesce: what is in flight finishes against the old scene) ...
// ... and ends as crt_reset does: accumulator zeroed, sample 0, frame ring emptied; the G-buffer is rebuilt on next use.
// Tile, row bands, bound outputs, stream, options and a communicator partition stay.
static int edit_end(crt_ctx *c)
{
    c->dn.valid = false; c->fdn.valid = false;
    return zero_state(c);
}

// The cost of the trees as they lie on the device (include/crt.h crt_accel_quality; crt_quality.hip): q = boxes2 prims2
// boxes4 prims4.  Zeros without an inner node; the 4-wide pair is that of the tree the wavefront kernels walk (the
// quantised one where there is one), NaN where they walk the 8-wide tree.  Two launches per tree, one readback, a sync.
// walked_only: the BVH2's pair is left 0 where there is a 4-wide tree (what the policy of crt_refit_accel compares).
// The 4-wide tree whose cost is reported and compared: 2 = the quantised one, 1 = the float one (a host build without
// quantisation), 0 = none (no inner node, or the wavefront kernels walk the 8-wide tree).
static int quality_wide_layout(const crt_ctx *c)
{
    const uint32_t n4 = c->bvh4.n_inner;
    if (c->accel_mode != CRT_ACCEL_BVH2 || n4 == 0 || c->bvh8q.ok) return 0;
    if (c->sc.nodes4q != nullptr) return 2;
    return c->bvh4.nodes.size() >= (size_t)n4 * kNode4Floats ? 1 : 0;
}

static int tree_quality(crt_ctx *c, double q[4], bool walked_only = false)
{
    q[0] = q[1] = q[2] = q[3] = 0.0;
    const uint32_t n2 = c->bvh.n_inner, n4 = c->bvh4.n_inner;
    if (c->accel_mode != CRT_ACCEL_BVH2 || n2 == 0 || c->sc.root < 0) return CRT_OK;
    const int layout4 = quality_wide_layout(c);
    const bool wide = layout4 != 0, quant = layout4 == 2;
    const size_t nb2 = (n2 + 255u) / 256u, nb4 = wide ? (n4 + 255u) / 256u : 0;
    CRT_ENSURE(c, c->q_part, nb2 + nb4);
    CRT_ENSURE(c, c->q_out, 8);
    HIPCHK(c, hipMemsetAsync(c->q_out.p, 0, 8 * sizeof(double), c->stream));
    if (!(walked_only && wide))
        HIPCHK(c, quality_launch(0, c->d_nodes.p, n2, (uint32_t)c->sc.root, c->sc.qbase, c->sc.qscale, c->q_part.p, c->q_out.p, c->stream));
    if (wide)
        HIPCHK(c, quality_launch(quant ? 2 : 1, quant ? (const void *)c->d_nodes4q.p : (const void *)c->d_nodes4.p, n4, (uint32_t)c->sc.root4,
                                 c->sc.qbase, c->sc.qscale, c->q_part.p + nb2, c->q_out.p + 4, c->stream));
    double h[8];
    HIPCHK(c, hipMemcpyAsync(h, c->q_out.p, sizeof h, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    q[0] = h[0]; q[1] = h[1];
    q[2] = c->bvh8q.ok ? (double)NAN : h[4]; q[3] = c->bvh8q.ok ? (double)NAN : h[5];
    return CRT_OK;
}

// The as-built values: from the untouched tree, at the first refit's set-up or the first crt_accel_quality after a build.
static int quality_as_built(crt_ctx *c)
{
    if (c->q_built_ok) return CRT_OK;
    CRT_TRY(tree_quality(c, c->q_built));
    c->q_built_ok = true;
    return CRT_OK;
}

// What option "refit_rebuild_pct" compares: boxes + prims of the walked tree -- the 4-wide one where there is one
// (quality_wide_layout, the predicate tree_quality computes by), else the BVH2.  NaN under the 8-wide walk, whose refit is
// a rebuild before the policy is asked.
static double walked_cost(const crt_ctx *c, const double q[4])
{
    if (c->bvh8q.ok) return (double)NAN;
    return quality_wide_layout(c) ? q[2] + q[3] : q[0] + q[1];
}

// Recompute every box of the current tree from the current primitives and hit_pad, its topology kept (BVH2, and the
// 4-wide tree: float boxes, quantised planes on a re-derived grid).  Rebuilt instead, with the builder that made the
// tree, where a refit cannot serve: an 8-wide tree, or refitted boxes that quantize_bvh4's rule refuses.  The host
// copies c->bvh / bvh4 / bvh4q keep the boxes of the build; nothing re-derives device nodes from them (every option
// that changes the tree takes effect at crt_build_accel, which builds from c->prims).
static int refit_tree(crt_ctx *c, bool *rebuilt)
{
    *rebuilt = false;
    if (c->accel_mode != CRT_ACCEL_BVH2) { c->accel_stale = false; return CRT_OK; }
    if (c->accel_topo) {                                         // records were added or removed: no topology to keep
        *rebuilt = true;
        c->accel_mode = -1;
        CRT_TRY(build_tree(c, CRT_ACCEL_BVH2));
        return quality_as_built(c);
    }
    if (c->bvh8q.ok) {
        *rebuilt = true;
        c->accel_mode = -1;
        return build_tree(c, CRT_ACCEL_BVH2);
    }
    const float pad = c->sc.hit_pad;
    const uint32_t n2 = c->bvh.n_inner, n4 = c->bvh4.n_inner;
    if (n2 == 0 || c->sc.root < 0) { c->accel_stale = false; c->tree_pad = pad; return CRT_OK; }   // one primitive: a leaf, no box
    const bool quant = c->sc.nodes4q != nullptr && n4 > 0;
    const bool wide_float = n4 > 0 && c->bvh4.nodes.size() >= (size_t)n4 * kNode4Floats;   // the host build's float 4-wide tree
    const bool wide = quant || wide_float;
    const void *refs4 = quant ? (const void *)c->d_nodes4q.p : (const void *)c->d_nodes4.p;
    if (!c->rf_ready) {                                  // once per tree: the cost of the tree as built, the level lists
        CRT_TRY(quality_as_built(c));
        HIPCHK(c, c->rf_cnt.alloc(1));
        HIPCHK(c, c->rf_lv2.alloc(n2));
        HIPCHK(c, refit_levels(c->d_nodes.p, 2, false, c->sc.root, n2, c->rf_lv2.p, c->rf_cnt.p, nullptr, c->rf_off2, c->stream));
        if (c->rf_off2.back() != n2) return fail(c, CRT_EDEVICE, "crt_refit_accel: the BVH2 has %u inner nodes, its levels list %u", n2, c->rf_off2.back());
        if (wide) {
            HIPCHK(c, c->rf_lv4.alloc(n4));
            HIPCHK(c, c->rf_nch4.alloc(n4));
            HIPCHK(c, refit_levels(refs4, 4, quant, 0, n4, c->rf_lv4.p, c->rf_cnt.p, c->rf_nch4.p, c->rf_off4, c->stream));
            if (c->rf_off4.back() != n4) return fail(c, CRT_EDEVICE, "crt_refit_accel: the 4-wide tree has %u nodes, its levels list %u", n4, c->rf_off4.back());
            if (!wide_float) HIPCHK(c, c->rf_fb.alloc((size_t)n4 * kNode4Floats));
        }
        c->rf_ready = true;
    }
    HIPCHK(c, refit_launch_bvh2(c->d_prim.p, pad, c->rf_lv2.p, c->rf_off2, (float *)c->d_nodes.p, c->stream));
    if (wide) {
        float *fb = wide_float ? (float *)c->d_nodes4.p : c->rf_fb.p;
        HIPCHK(c, refit_launch_wide(c->d_prim.p, pad, c->rf_lv4.p, c->rf_off4, refs4, quant, c->rf_nch4.p, fb, c->stream));
        if (quant) {
            // quantize_bvh4's grid: the union of every box = the union of the root's children (each box is its children's union)
            float root[kNode4Floats];
            uint32_t k = 0;
            HIPCHK(c, hipMemcpyAsync(root, fb, sizeof root, hipMemcpyDeviceToHost, c->stream));
            HIPCHK(c, hipMemcpyAsync(&k, c->rf_nch4.p, 4, hipMemcpyDeviceToHost, c->stream));
            HIPCHK(c, hipStreamSynchronize(c->stream));
            float glo[3] = {FLT_MAX, FLT_MAX, FLT_MAX}, ghi[3] = {-FLT_MAX, -FLT_MAX, -FLT_MAX}, base[3], scale[3];
            bool ok = k > 0 && k <= 4;
            for (uint32_t i = 0; ok && i < k; i++)
                for (int a = 0; a < 3; a++) {
                    const float l = root[4 * a + i], h = root[12 + 4 * a + i];
                    if (!(l > -1.0e30f) || !(h < 1.0e30f)) ok = false;     // unbounded primitive: not quantisable
                    glo[a] = std::min(glo[a], l); ghi[a] = std::max(ghi[a], h);
                }
            for (int a = 0; ok && a < 3; a++) {
                const float ext = std::max(ghi[a] - glo[a], 1.0e-3f);
                const float mag = std::max(std::fabs(glo[a]), std::fabs(ghi[a]));
                if (mag > 16.0f * ext) ok = false;                          // too far from the origin for the slack
                base[a] = glo[a]; scale[a] = ext / 65533.0f;
            }
            if (!ok) {
                *rebuilt = true;
                c->accel_mode = -1;
                return build_tree(c, CRT_ACCEL_BVH2);
            }
            const double bd[3] = {base[0], base[1], base[2]}, sd[3] = {scale[0], scale[1], scale[2]};
            HIPCHK(c, refit_launch_quant4(fb, c->rf_nch4.p, n4, c->d_nodes4q.p, bd, sd, c->stream));
            for (int a = 0; a < 3; a++) { c->sc.qbase[a] = c->bvh4q.base[a] = base[a]; c->sc.qscale[a] = c->bvh4q.scale[a] = scale[a]; }
        }
    }
    HIPCHK(c, hipStreamSynchronize(c->stream));
    c->tree_pad = pad;
    c->accel_stale = false;
    c->refits++;
    return CRT_OK;
}

int crt_set_camera(crt_ctx *c, const float camera[16])
{
    if (!c) return CRT_EINVAL;
    if (!camera) return fail(c, CRT_EINVAL, "crt_set_camera: camera is NULL");
    if (!c->have_scene) return fail(c, CRT_ESTATE, "crt_set_camera: upload a scene first");
    if (camera[11] != (float)c->W || camera[12] != (float)c->H)
        return fail(c, CRT_EINVAL, "crt_set_camera: floats 11, 12 (width, height) must stay %u x %u (a size change is crt_upload_scene's)",
                    c->W, c->H);
    CRT_TRY(quiesce(c, true));
    std::memcpy(c->camera, camera, sizeof c->camera);
    camera_frame(c->camera, c->sc.cam);
    c->sc.hit_pad = pad_of(c->s_prims, c->camera);               // = scene_hit_pad(c->prims, c->camera), no primitive scanned
    if (c->accel_mode == CRT_ACCEL_BVH2 && !c->accel_stale && c->sc.hit_pad > c->tree_pad) {
        bool rebuilt = false;                                     // a larger pad: the boxes must grow
        CRT_TRY(refit_tree(c, &rebuilt));
    }
    return edit_end(c);
}

// The two halves every primitive edit shares (crt_update_primitives, crt_transform_primitives).  Before anything changes:
// option "temporal_motion": the history stays, with the scene as its newest slot saw it.  Not retaken
// until a newer slot exists: several edits may precede one refit, and a frame that is never filtered temporally
// must not cost the older slot its geometry.
static int prims_edit_history(crt_ctx *c)
{
    crt_ctx::Denoise &d = c->dn;
    crt_ctx::DnSlot *const newest = !d.motion ? nullptr : d.cur.valid ? &d.cur : d.prev.valid ? &d.prev : nullptr;
    const bool take = newest && !newest->snap;
    const size_t nb = c->prims.size() * 80;                      // (the records: d_raw.n and snap.n are capacities)
    if (take && d.snap.n < nb) {                                 // before anything changes: CRT_ENOMEM leaves all as it was
        DevBuf<unsigned char> fresh;
        HIPCHK(c, fresh.alloc(nb));
        d.snap = std::move(fresh);
    }
    if (take) {
        if (nb) HIPCHK(c, hipMemcpyAsync(d.snap.p, c->d_raw.p, nb, hipMemcpyDeviceToDevice, c->stream));
        d.cur.snap = d.prev.snap = false;
        newest->snap = true;
    }
    if (!newest) d.drop();                                       // (nothing to keep, or the option is off)
    return CRT_OK;
}

// After d_raw (and the leaf-ordered records) changed: hit_pad exactly as a fresh upload computes it (the full scan: the
// value enters the kernels), the tree stale, the frame state reset.  scan_out: the scan's word on the device, from a
// caller that allocates everything before it changes anything.
static int prims_edit_end(crt_ctx *c, uint32_t *scan_out = nullptr)
{
    DevBuf<uint32_t> s;
    if (!scan_out) { HIPCHK(c, s.alloc(1)); scan_out = s.p; }
    HIPCHK(c, refit_launch_pad(c->d_raw.p, (uint32_t)c->prims.size(), scan_out, c->stream));
    uint32_t sb = 0;
    HIPCHK(c, hipMemcpyAsync(&sb, scan_out, 4, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    c->s_prims = bits_f(sb);
    c->sc.hit_pad = pad_of(c->s_prims, c->camera);
    if (c->accel_mode == CRT_ACCEL_BVH2) c->accel_stale = true;  // (CRT_ACCEL_NONE: no tree to go stale)
    return edit_end(c);
}

int crt_update_primitives(crt_ctx *c, uint32_t first, uint32_t count, const void *records)
{
    if (!c) return CRT_EINVAL;
    if (!records && count) return fail(c, CRT_EINVAL, "crt_update_primitives: records is NULL");
    if (!c->have_scene) return fail(c, CRT_ESTATE, "crt_update_primitives: upload a scene first");
    const size_t n = c->prims.size();
    if ((uint64_t)first + count > n)
        return fail(c, CRT_EINVAL, "crt_update_primitives: range [%u, %llu) outside the scene's %zu primitives", first,
                    (unsigned long long)first + count, n);
    std::vector<HostPrim> np(count);
    for (uint32_t k = 0; k < count; k++) {
        const uint32_t i = first + k;
        const HostPrim p = np[k] = read_prim((const uint8_t *)records, k), &o = c->prims[i];
        if (p.index != i) return fail(c, CRT_EINVAL, "crt_update_primitives: record %u: index is %u, must equal the array position %u", k, p.index, i);
        if (p.category != o.category || p.material != o.material)
            return fail(c, CRT_EINVAL, "crt_update_primitives: primitive %u: category and material cannot change (a topology edit: crt_upload_scene)", i);
        if (p.emission >= c->sc.nspectra || p.reflectance >= c->sc.nspectra)
            return fail(c, CRT_EINVAL, "crt_update_primitives: primitive %u: spectrum index out of range", i);
    }
    CRT_TRY(quiesce(c, true));
    CRT_TRY(prims_edit_history(c));
    std::copy(np.begin(), np.end(), c->prims.begin() + first);   // the host SAH builder reads these
    if (count) {
        HIPCHK(c, hipMemcpyAsync(c->d_raw.p + (size_t)first * 80, records, (size_t)count * 80, hipMemcpyHostToDevice, c->stream));   // the LBVH builder's input
        if (c->accel_mode >= 0 && !c->accel_topo)                // the leaf-ordered records, in their slots (not those of another primitive list)
            HIPCHK(c, refit_launch_prims(c->d_raw.p, first, count, c->d_slot_of_index.p, c->d_prim.p, c->d_primD.p, c->stream));
    }
    return prims_edit_end(c);
}

int crt_transform_primitives(crt_ctx *c, const crt_prim_transform *ops, uint32_t n_ops)
{
    if (!c) return CRT_EINVAL;
    if (!ops && n_ops) return fail(c, CRT_EINVAL, "crt_transform_primitives: ops is NULL");
    if (!c->have_scene) return fail(c, CRT_ESTATE, "crt_transform_primitives: upload a scene first");
    const size_t n = c->prims.size();
    std::vector<uint32_t> live;                                  // the ops that move something, in the caller's order
    for (uint32_t k = 0; k < n_ops; k++) {
        const crt_prim_transform &o = ops[k];
        if ((uint64_t)o.first + o.count > n)
            return fail(c, CRT_EINVAL, "crt_transform_primitives: op %u: range [%u, %llu) outside the scene's %zu primitives", k, o.first,
                        (unsigned long long)o.first + o.count, n);
        bool finite = std::isfinite(o.radius_scale);
        for (int a = 0; a < 12; a++) finite = finite && std::isfinite(o.m[a]);
        if (!finite) return fail(c, CRT_EINVAL, "crt_transform_primitives: op %u: a non-finite matrix entry or radius_scale", k);
        if (o.count) live.push_back(k);
    }
    std::vector<uint32_t> by_first(live);
    std::sort(by_first.begin(), by_first.end(), [&](uint32_t a, uint32_t b) { return ops[a].first < ops[b].first; });
    for (size_t j = 1; j < by_first.size(); j++) {
        const crt_prim_transform &a = ops[by_first[j - 1]], &b = ops[by_first[j]];
        if (a.first + a.count > b.first)
            return fail(c, CRT_EINVAL, "crt_transform_primitives: ops %u and %u overlap: both move primitive %u", by_first[j - 1], by_first[j], b.first);
    }
    // the device table: live.size() + 1 prefix sums (padded to whole records), then the ops
    const size_t op_dw = sizeof(crt_prim_transform) / 4, head = (live.size() + 1 + op_dw - 1) / op_dw * op_dw;
    std::vector<uint32_t> tab(head + live.size() * op_dw, 0u);
    uint32_t total = 0;                                          // <= n: the ranges are disjoint
    for (size_t j = 0; j < live.size(); j++) {
        tab[j] = total;
        total += ops[live[j]].count;
        std::memcpy(&tab[head + j * op_dw], &ops[live[j]], sizeof(crt_prim_transform));
    }
    tab[live.size()] = total;
    CRT_TRY(quiesce(c, true));
    // the table and the snapshot are allocated before anything changes, the history included: CRT_ENOMEM leaves all as it was
    if (total && c->xf_tab.n < tab.size()) HIPCHK(c, c->xf_tab.alloc(std::max(tab.size(), 2 * c->xf_tab.n)));
    CRT_TRY(prims_edit_history(c));
    if (total) {
        HIPCHK(c, hipMemcpyAsync(c->xf_tab.p, tab.data(), tab.size() * 4, hipMemcpyHostToDevice, c->stream));
        const bool built = c->accel_mode >= 0 && !c->accel_topo; // the leaf-ordered records exist: moved in the same thread
        HIPCHK(c, refit_launch_transform(c->d_raw.p, c->xf_tab.p, (const crt_prim_transform *)(c->xf_tab.p + head), (uint32_t)live.size(), total,
                                         c->d_slot_of_index.p, built ? c->d_prim.p : nullptr, built ? c->d_primD.p : nullptr, c->stream));
        c->prims_moved = true;
    }
    return prims_edit_end(c);                                    // (its sync covers the table's upload from `tab`)
}

// ---------------------------------------------------------------- topology edits (crt_remove_primitives, crt_append_primitives)
// Both calls run in the same four steps: validate (nothing touched), allocate (TopoEdit holds every new buffer until the
// commit, so CRT_ENOMEM frees them and leaves all as it was), prims_edit_history, then change records, mirror, lights and
// derived state -- nothing after the allocations can fail short of a device error.

struct TopoEdit {
    std::vector<HostPrim> lights;       // the light list after the call
    bool lights_replaced = false;       // the caller passed a list: d_lights is re-made
    bool lights_changed = false;        // ... or kept lights were renumbered: their rows are re-sent
    DevBuf<float4> d_lights;
    DevBuf<unsigned char> raw, snap;    // a new d_raw / history snapshot, where the call needs one
    DevBuf<float4> prim, primD;         // CRT_ACCEL_NONE: the packed records in array order, re-derived here
    DevBuf<uint32_t> slot, scan;        // (scan: prims_edit_end's word)
    std::vector<uint32_t> iota, tab;    // (host sources of asynchronous copies: they live until the call's last sync)
    std::vector<float4> rows;
};

// The caller's light list, if there is one, with the upload's validation.
static int topo_lights(crt_ctx *c, const char *what, const void *lights, size_t nlight, TopoEdit &e)
{
    if (!lights) {
        if (nlight) return fail(c, CRT_EINVAL, "%s: lights is NULL with nlight = %zu (NULL, 0 keeps the light list)", what, nlight);
        e.lights = c->lights;
        return CRT_OK;
    }
    if (nlight < 1) return fail(c, CRT_EINVAL, "%s: at least one light record is required", what);
    e.lights.resize(nlight);
    for (size_t i = 0; i < nlight; i++) {
        e.lights[i] = read_prim((const uint8_t *)lights, i);
        if (e.lights[i].emission >= c->sc.nspectra) return fail(c, CRT_EINVAL, "%s: light %zu: emission index out of range", what, i);
    }
    e.lights_replaced = true;
    return CRT_OK;
}

// Every allocation of the call, for a scene of n_new primitives: new_raw / new_snap bytes (0 = that buffer stays).
static int topo_alloc(crt_ctx *c, TopoEdit &e, size_t n_new, size_t new_raw, size_t new_snap, bool records_change)
{
    if (new_raw) HIPCHK(c, e.raw.alloc(new_raw));
    if (new_snap) HIPCHK(c, e.snap.alloc(new_snap));
    if (e.lights_replaced) HIPCHK(c, e.d_lights.alloc(e.lights.size() * 3));
    if (records_change && c->accel_mode == CRT_ACCEL_NONE) {
        HIPCHK(c, e.prim.alloc(std::max<size_t>(n_new * 3, 3)));
        HIPCHK(c, e.primD.alloc(std::max<size_t>(n_new, 1)));
        HIPCHK(c, e.slot.alloc(std::max<size_t>(n_new, 1)));
    }
    HIPCHK(c, e.scan.alloc(1));
    return CRT_OK;
}

// After d_raw and c->prims hold the new list: the lights, the state derived from the list as a fresh upload derives
// it, the packed records (CRT_ACCEL_NONE) or the topology-stale tree, and the end of every primitive edit.
static int topo_commit(crt_ctx *c, TopoEdit &e, bool records_change)
{
    DevScene &S = c->sc;
    const uint32_t n = (uint32_t)c->prims.size();
    if (e.lights_replaced || e.lights_changed) {
        e.rows.resize(e.lights.size() * 3);
        for (size_t i = 0; i < e.lights.size(); i++) light_rows(e.lights[i], &e.rows[3 * i]);
        if (e.lights_replaced) {
            c->d_lights = std::move(e.d_lights);
            S.lights = c->d_lights.p;
            S.nlight = (uint32_t)e.lights.size();
            S.inv_nlight = 1.0f / (float)S.nlight;
            c->dn.drop();                                        // other illumination: as crt_update_lights
        }
        c->lights.swap(e.lights);
        HIPCHK(c, hipMemcpyAsync(c->d_lights.p, e.rows.data(), e.rows.size() * sizeof(float4), hipMemcpyHostToDevice, c->stream));
    }
    if (records_change) {
        S.nf_last[0] = S.nf_last[1] = kNoHit;
        for (size_t i = n; i-- > 0 && S.nf_last[1] == kNoHit;)
            if (c->prims[i].category != 2u) (S.nf_last[0] == kNoHit ? S.nf_last[0] : S.nf_last[1]) = (uint32_t)i;
        if (c->accel_mode == CRT_ACCEL_NONE) {
            e.iota.resize(n);
            for (uint32_t i = 0; i < n; i++) e.iota[i] = i;
            HIPCHK(c, hipMemcpyAsync(e.slot.p, e.iota.data(), (size_t)n * 4, hipMemcpyHostToDevice, c->stream));
            HIPCHK(c, refit_launch_prims(c->d_raw.p, 0, n, e.slot.p, e.prim.p, e.primD.p, c->stream));
            c->d_prim = std::move(e.prim); c->d_primD = std::move(e.primD); c->d_slot_of_index = std::move(e.slot);
            S.prim = c->d_prim.p; S.primD = c->d_primD.p; S.slot_of_index = c->d_slot_of_index.p;
            S.nprim = n;
            S.npatch = 0;
            for (const HostPrim &p : c->prims) S.npatch += p.category == 0u ? 1u : 0u;
        }
        if (c->accel_mode == CRT_ACCEL_BVH2) c->accel_topo = true;   // (nprim, npatch and the packed records: the rebuild's)
    }
    return prims_edit_end(c, e.scan.p);                          // (its sync: before `e` frees what the kernels above still read)
}

int crt_remove_primitives(crt_ctx *c, const crt_prim_range *ranges, uint32_t n_ranges, const void *lights, size_t nlight)
{
    if (!c) return CRT_EINVAL;
    if (!ranges && n_ranges) return fail(c, CRT_EINVAL, "crt_remove_primitives: ranges is NULL");
    if (!c->have_scene) return fail(c, CRT_ESTATE, "crt_remove_primitives: upload a scene first");
    const size_t n = c->prims.size();
    std::vector<crt_prim_range> live;                            // the ranges that remove something, ascending
    for (uint32_t k = 0; k < n_ranges; k++) {
        if ((uint64_t)ranges[k].first + ranges[k].count > n)
            return fail(c, CRT_EINVAL, "crt_remove_primitives: range %u: [%u, %llu) outside the scene's %zu primitives", k, ranges[k].first,
                        (unsigned long long)ranges[k].first + ranges[k].count, n);
        if (ranges[k].count) live.push_back(ranges[k]);
    }
    std::sort(live.begin(), live.end(), [](const crt_prim_range &a, const crt_prim_range &b) { return a.first < b.first; });
    for (size_t j = 1; j < live.size(); j++)
        if (live[j - 1].first + live[j - 1].count > live[j].first)
            return fail(c, CRT_EINVAL, "crt_remove_primitives: two ranges overlap: both remove primitive %u", live[j].first);
    // the device table: the new index before which each range fell, then the prefix sums of the counts
    const size_t m = live.size();
    TopoEdit e;
    e.tab.assign(2 * m + 1, 0u);
    uint32_t total = 0;                                          // <= n: the ranges are disjoint
    for (size_t j = 0; j < m; j++) {
        e.tab[j] = live[j].first - total;
        total += live[j].count;
        e.tab[m + 1 + j] = total;
    }
    if (total && total == n)
        return fail(c, CRT_EINVAL, "crt_remove_primitives: the call would remove all %zu primitives (an empty scene is crt_upload_scene's)", n);
    CRT_TRY(topo_lights(c, "crt_remove_primitives", lights, nlight, e));
    if (!e.lights_replaced && total)
        for (size_t i = 0; i < e.lights.size(); i++) {
            const uint32_t x = e.lights[i].index;
            if (x >= n) continue;                                // (names no primitive: the kernels guard, as after an upload)
            size_t r = std::upper_bound(live.begin(), live.end(), x, [](uint32_t v, const crt_prim_range &a) { return v < a.first; }) - live.begin();
            if (r && x < live[r - 1].first + live[r - 1].count)
                return fail(c, CRT_EINVAL, "crt_remove_primitives: light %zu lies on primitive %u, which the call removes: pass the new light list", i, x);
            if (e.tab[m + r]) { e.lights[i].index = x - e.tab[m + r]; e.lights_changed = true; }
        }
    const size_t n_new = n - total;
    CRT_TRY(quiesce(c, true));
    crt_ctx::Denoise &d = c->dn;
    const bool keep = d.motion && (d.cur.valid || d.prev.valid);   // prims_edit_history keeps the history, with a snapshot
    CRT_TRY(topo_alloc(c, e, n_new, total ? n_new * 80 : 0, total && keep ? n_new * 80 : 0, total != 0));
    if (total && c->xf_tab.n < e.tab.size()) HIPCHK(c, c->xf_tab.alloc(std::max(e.tab.size(), 2 * c->xf_tab.n)));
    CRT_TRY(prims_edit_history(c));
    if (total) {
        HIPCHK(c, hipMemcpyAsync(c->xf_tab.p, e.tab.data(), e.tab.size() * 4, hipMemcpyHostToDevice, c->stream));
        HIPCHK(c, refit_launch_compact(c->d_raw.p, e.raw.p, c->xf_tab.p, (uint32_t)m, (uint32_t)n_new, c->stream));
        if (keep) HIPCHK(c, refit_launch_compact(d.snap.p, e.snap.p, c->xf_tab.p, (uint32_t)m, (uint32_t)n_new, c->stream));
        std::swap(c->d_raw, e.raw);                              // (the old arrays go with `e`, after the commit's sync)
        if (keep) std::swap(d.snap, e.snap);
        size_t w = 0, r = 0;                                     // the mirror: survivors close ranks, renumbered
        for (size_t j = 0; j <= m; j++) {
            const size_t stop = j < m ? live[j].first : n;
            if (w != r) std::copy(c->prims.begin() + r, c->prims.begin() + stop, c->prims.begin() + w);
            w += stop - r;
            if (j < m) r = (size_t)live[j].first + live[j].count;
        }
        c->prims.resize(n_new);
        for (size_t i = live[0].first; i < n_new; i++) c->prims[i].index = (uint32_t)i;
        matte_ids_remove(c, live.data(), m);                     // the id table: compacted alike, a survivor keeps its id
    }
    return topo_commit(c, e, total != 0);
}

int crt_append_primitives(crt_ctx *c, const void *records, uint32_t count, const void *lights, size_t nlight)
{
    if (!c) return CRT_EINVAL;
    if (!records && count) return fail(c, CRT_EINVAL, "crt_append_primitives: records is NULL");
    if (!c->have_scene) return fail(c, CRT_ESTATE, "crt_append_primitives: upload a scene first");
    const size_t n = c->prims.size(), n_new = n + count;
    if (n_new >= (1u << 28)) return fail(c, CRT_EINVAL, "crt_append_primitives: too many primitives (%zu + %u)", n, count);
    std::vector<HostPrim> np(count);
    for (uint32_t k = 0; k < count; k++) {
        const HostPrim &p = np[k] = read_prim((const uint8_t *)records, k);
        if (p.category > 2u) return fail(c, CRT_EINVAL, "crt_append_primitives: record %u: category %u not in {0,1,2}", k, p.category);
        if (p.material > 2u) return fail(c, CRT_EINVAL, "crt_append_primitives: record %u: material %u not in {0,1,2}", k, p.material);
        if (p.index != n + k)
            return fail(c, CRT_EINVAL, "crt_append_primitives: record %u: index is %u, must equal its array position %zu", k, p.index, n + k);
        if (p.emission >= c->sc.nspectra || p.reflectance >= c->sc.nspectra)
            return fail(c, CRT_EINVAL, "crt_append_primitives: record %u: spectrum index out of range", k);
    }
    TopoEdit e;
    CRT_TRY(topo_lights(c, "crt_append_primitives", lights, nlight, e));
    CRT_TRY(quiesce(c, true));
    crt_ctx::Denoise &d = c->dn;
    const bool keep = d.motion && (d.cur.valid || d.prev.valid);
    // a buffer that cannot take the records grows by half of itself at least, device to device
    const auto grown = [&](size_t have) { return have >= n_new * 80 ? (size_t)0 : std::max(n_new * 80, have + have / 2); };
    CRT_TRY(topo_alloc(c, e, n_new, count ? grown(c->d_raw.n) : 0, count && keep ? grown(d.snap.n) : 0, count != 0));
    if (c->prims.capacity() < n_new)                             // (the mirror grows as d_raw does; std::bad_alloc: nothing has changed)
        c->prims.reserve(std::max(n_new, c->prims.capacity() + c->prims.capacity() / 2));
    matte_ids_reserve(c, n_new);                                 // (and the id table beside it)
    CRT_TRY(prims_edit_history(c));
    if (count) {
        if (e.raw.p) {
            HIPCHK(c, hipMemcpyAsync(e.raw.p, c->d_raw.p, n * 80, hipMemcpyDeviceToDevice, c->stream));
            std::swap(c->d_raw, e.raw);
        }
        HIPCHK(c, hipMemcpyAsync(c->d_raw.p + n * 80, records, (size_t)count * 80, hipMemcpyHostToDevice, c->stream));
        if (keep) {                                              // the snapshot takes them too: new records compare equal
            if (e.snap.p) {
                HIPCHK(c, hipMemcpyAsync(e.snap.p, d.snap.p, n * 80, hipMemcpyDeviceToDevice, c->stream));
                std::swap(d.snap, e.snap);
            }
            HIPCHK(c, hipMemcpyAsync(d.snap.p + n * 80, records, (size_t)count * 80, hipMemcpyHostToDevice, c->stream));
        }
        c->prims.insert(c->prims.end(), np.begin(), np.end());
        matte_ids_append(c, count);                              // primitive n + k gets the id n + k
    }
    return topo_commit(c, e, count != 0);
}

int crt_read_primitives(crt_ctx *c, uint32_t first, uint32_t count, void *out)
{
    if (!c) return CRT_EINVAL;
    if (!out && count) return fail(c, CRT_EINVAL, "crt_read_primitives: out is NULL");
    if (!c->have_scene) return fail(c, CRT_ESTATE, "crt_read_primitives: upload a scene first");
    if ((uint64_t)first + count > c->prims.size())
        return fail(c, CRT_EINVAL, "crt_read_primitives: range [%u, %llu) outside the scene's %zu primitives", first,
                    (unsigned long long)first + count, c->prims.size());
    CRT_TRY(quiesce(c, true));               // (a sync point; nothing is edited)
    if (count) {
        HIPCHK(c, hipMemcpyAsync(out, c->d_raw.p + (size_t)first * 80, (size_t)count * 80, hipMemcpyDeviceToHost, c->stream));
        HIPCHK(c, hipStreamSynchronize(c->stream));
    }
    return CRT_OK;
}

int crt_update_lights(crt_ctx *c, uint32_t first, uint32_t count, const void *records)
{
    if (!c) return CRT_EINVAL;
    if (!records && count) return fail(c, CRT_EINVAL, "crt_update_lights: records is NULL");
    if (!c->have_scene) return fail(c, CRT_ESTATE, "crt_update_lights: upload a scene first");
    if ((uint64_t)first + count > c->lights.size())
        return fail(c, CRT_EINVAL, "crt_update_lights: range [%u, %llu) outside the scene's %zu lights", first,
                    (unsigned long long)first + count, c->lights.size());
    std::vector<HostPrim> nl(count);
    for (uint32_t k = 0; k < count; k++) {
        nl[k] = read_prim((const uint8_t *)records, k);
        if (nl[k].emission >= c->sc.nspectra) return fail(c, CRT_EINVAL, "crt_update_lights: light %u: emission index out of range", first + k);
    }
    CRT_TRY(quiesce(c, true));
    std::copy(nl.begin(), nl.end(), c->lights.begin() + first);
    // option "temporal_clip_pct" (DESIGN.md 6l): the history stays -- both slots, the moments, a geometry snapshot -- and the
    // blend clips what the new lighting has made stale
    if (c->dn.clip_pct == 0) c->dn.drop();
    else if (c->dn.cur.valid || c->dn.prev.valid) c->dn.relit = true;
    std::vector<float4> hl((size_t)count * 3);
    for (uint32_t k = 0; k < count; k++) light_rows(nl[k], &hl[3 * (size_t)k]);
    if (count) {
        HIPCHK(c, hipMemcpyAsync(c->d_lights.p + 3 * (size_t)first, hl.data(), hl.size() * sizeof(float4), hipMemcpyHostToDevice, c->stream));
        HIPCHK(c, hipStreamSynchronize(c->stream));
    }
    return edit_end(c);
}

int crt_refit_accel(crt_ctx *c, int *rebuilt)
{
    if (rebuilt) *rebuilt = 0;
    if (!c) return CRT_EINVAL;
    if (!c->have_scene) return fail(c, CRT_ESTATE, "crt_refit_accel: upload a scene first");
    CRT_TRY(quiesce(c, true));
    bool rb = false;
    CRT_TRY(refit_tree(c, &rb));
    if (!rb && c->refit_rebuild_pct && c->q_built_ok) {          // (no as-built values: no tree with an inner node)
        double q[4];
        CRT_TRY(tree_quality(c, q, true));
        const double now = walked_cost(c, q), built = walked_cost(c, c->q_built);
        if (std::isfinite(now) && std::isfinite(built) && now > built * (double)c->refit_rebuild_pct / 100.0) {
            rb = true;                                           // the refitted tree has decayed: a fresh one, by the builder that made it
            c->accel_mode = -1;
            CRT_TRY(build_tree(c, CRT_ACCEL_BVH2));
            CRT_TRY(quality_as_built(c));
            c->policy_rebuilds++;
        }
    }
    if (rebuilt) *rebuilt = rb ? 1 : 0;
    return edit_end(c);
}

int crt_accel_quality(crt_ctx *c, double out[12])
{
    if (!c || !out) return CRT_EINVAL;
    if (!c->have_scene || c->accel_mode < 0) return fail(c, CRT_ESTATE, "crt_accel_quality: scene + accel required");
    if (c->accel_topo) return fail(c, CRT_ESTATE, "crt_accel_quality: the tree belongs to another primitive list: call crt_refit_accel or crt_build_accel first");
    CRT_TRY(quiesce(c, true));
    if (!c->q_built_ok) {                                        // no refit since the build: the tree is as it was built
        CRT_TRY(quality_as_built(c));
        for (int k = 0; k < 4; k++) out[k] = c->q_built[k];
    } else {
        CRT_TRY(tree_quality(c, out));
    }
    for (int k = 0; k < 4; k++) out[4 + k] = c->q_built[k];
    out[8] = (double)c->refits;
    out[9] = (double)c->policy_rebuilds;
    out[10] = c->bvh8q.ok ? 0.0 : 1.0;
    out[11] = 0.0;
    return CRT_OK;
}

}  // extern "C"
