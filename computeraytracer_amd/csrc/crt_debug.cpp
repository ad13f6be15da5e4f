// crt_debug.cpp -- the debug read-outs of include/crt.h: what the tests look at that no renderer needs.
#include "crt_ctx.h"

using namespace crt;

extern "C" {

int crt_debug_intersect(crt_ctx *c, const float *rays, size_t n, float *out)
{
    if (!c || (!rays && n) || (!out && n)) return CRT_EINVAL;
    if (!c->have_scene || c->accel_mode < 0) return fail(c, CRT_ESTATE, "crt_debug_intersect: scene + accel required");
    if (c->accel_stale) return fail(c, CRT_ESTATE, "crt_debug_intersect: primitives were updated: call crt_refit_accel or crt_build_accel first");
    HIPCHK(c, hipSetDevice(c->device));
    DevBuf<float> din, dout;
    HIPCHK(c, din.alloc(n * 8));
    hipError_t e = dout.alloc(n * 8);
    if (e == hipSuccess) e = hipMemcpyAsync(din.p, rays, n * 8 * sizeof(float), hipMemcpyHostToDevice, c->stream);
    if (e == hipSuccess) e = launch_debug_intersect(c->sc, din.p, n, dout.p, c->accel_mode == CRT_ACCEL_NONE, c->stream);
    if (e == hipSuccess) e = hipMemcpyAsync(out, dout.p, n * 8 * sizeof(float), hipMemcpyDeviceToHost, c->stream);
    if (e == hipSuccess) e = hipStreamSynchronize(c->stream);
    if (e != hipSuccess) return fail(c, CRT_EDEVICE, "crt_debug_intersect: %s", hipGetErrorString(e));
    return CRT_OK;
}

// Caller-chosen rays through the traversal kernel crt_trace launches: one iteration's ray lists filled by hand (as
// k_wf_shade / k_wf_gen leave them), one wf_launch_trace with the context's scene, form, waves per CU and overflow
// area, and P.hit / P.vis read back.  The lists, the control block and the result arrays are the call's own.
int crt_debug_trace_rays(crt_ctx *c, const float *rays, size_t n, uint32_t *out, uint64_t report[8])
{
    if (!c || (!rays && n) || (!out && n)) return CRT_EINVAL;
    if (!c->have_scene || c->accel_mode < 0) return fail(c, CRT_ESTATE, "crt_debug_trace_rays: scene + accel required");
    if (c->accel_stale) return fail(c, CRT_ESTATE, "crt_debug_trace_rays: primitives were updated: call crt_refit_accel or crt_build_accel first");
    if (c->accel_mode != CRT_ACCEL_BVH2 || c->pipeline != 1)
        return fail(c, CRT_ESTATE, "crt_debug_trace_rays: no wavefront tree (CRT_ACCEL_NONE or option pipeline = 0)");
    if (n > (size_t)kWfListSlot) return fail(c, CRT_EINVAL, "crt_debug_trace_rays: too many rays");
    const uint32_t nprim = (uint32_t)c->prims.size();
    // ray i goes to shard kShardOf[i % 16] (a quarter of the shards: the waves that start on an empty one scan, the
    // listed ones hold several chunks) and, by (i / 16) & 1, to the first or the second list of its kind
    static const uint8_t kShardOf[16] = {0, 1, 2, 3, 5, 8, 13, 21, 34, 55, 63, 62, 31, 32, 33, 7};
    std::vector<uint32_t> cnt((size_t)kWfShards * 4, 0u), pos(n);
    for (size_t i = 0; i < n; i++) {
        const float *r = rays + 12 * i;
        uint32_t u[4];
        std::memcpy(u, r + 6, 16);                               // exclude, kind, t_light, light index
        for (int k = 0; k < 6; k++)
            if (!std::isfinite(r[k])) return fail(c, CRT_EINVAL, "crt_debug_trace_rays: ray %zu is not finite (crt_trace resolves such rays without a walk)", i);
        if (u[1] > 1u) return fail(c, CRT_EINVAL, "crt_debug_trace_rays: ray %zu: kind must be 0 (extension) or 1 (shadow)", i);
        if (u[1] == 1u && (!std::isfinite(r[8]) || u[3] >= nprim))
            return fail(c, CRT_EINVAL, "crt_debug_trace_rays: shadow ray %zu: t_light must be finite and the light index below %u", i, nprim);
        const uint32_t cls = (u[1] ? 2u : 0u) + (uint32_t)((i / 16) & 1u);
        pos[i] = cnt[(size_t)kShardOf[i % 16] * 4 + cls]++;
    }
    uint32_t list_cap = 64;
    for (uint32_t v : cnt) list_cap = std::max(list_cap, (v + 63u) & ~63u);
    CRT_TRY(quiesce(c, true));
    CRT_TRY(wf_ensure_overflow(c));

    WfParams W{};
    W.sc = c->sc;
    W.list_cap = list_cap;
    W.count = c->counting ? 1u : 0u;
    W.trace_form = (uint32_t)c->wf_trace_form;
    W.overflow_lanes = (uint32_t)c->num_cu * wf_waves(wf_options(c)) * 64u;
    W.stack_overflow = c->w_overflow.p;                          // pipe 0's part
    const int kernel = wf_trace_kernel(W);
    if (report) {
        report[0] = kernel == 2 ? 8 : 4;                          // node width of the walked tree
        report[1] = c->wf_depth;                                 // its inner levels
        report[2] = wf_stack_lds(c);                             // stack entries per lane in LDS
        report[3] = wf_overflow_levels(c);                       // ... and in the overflow area
        report[4] = report[2] + report[3];                       // capacity per lane
        report[5] = 0;                                           // deepest stack a lane reached (counting variant)
        report[6] = (uint64_t)kernel;
        report[7] = W.count;
    }
    if (n == 0) return CRT_OK;

    const size_t cls_stride = (size_t)list_cap * kWfShards;
    std::vector<float4> hA(4 * cls_stride, float4{0, 0, 0, 0}), hB(4 * cls_stride, float4{0, 0, 0, 0});
    std::vector<uint4> hC(4 * cls_stride, uint4{0, 0, 0, 0});
    std::vector<uint32_t> slot_of(std::max<uint32_t>(nprim, 1u)), index_of(std::max<uint32_t>(nprim, 1u));
    if (nprim) HIPCHK(c, hipMemcpy(slot_of.data(), c->d_slot_of_index.p, (size_t)nprim * 4, hipMemcpyDeviceToHost));
    for (uint32_t i = 0; i < nprim; i++) {
        if (slot_of[i] >= nprim) return fail(c, CRT_EDEVICE, "crt_debug_trace_rays: slot_of_index[%u] = %u", i, slot_of[i]);
        index_of[slot_of[i]] = i;
    }
    for (size_t i = 0; i < n; i++) {
        const float *r = rays + 12 * i;
        uint32_t u[4];
        std::memcpy(u, r + 6, 16);
        const uint32_t cls = (u[1] ? 2u : 0u) + (uint32_t)((i / 16) & 1u);
        const size_t g = (size_t)cls * cls_stride + (size_t)kShardOf[i % 16] * list_cap + pos[i];
        hA[g] = float4{r[0], r[1], r[2], bits_f(u[0])};
        if (u[1]) {
            hB[g] = float4{r[3], r[4], r[5], r[8]};
            hC[g] = uint4{(uint32_t)i, u[3], slot_of[u[3]], 0u};
        } else {
            hB[g] = float4{r[3], r[4], r[5], bits_f((uint32_t)i)};
        }
    }
    std::vector<WfCtl> hctl(1);
    std::memset(hctl.data(), 0, sizeof(WfCtl));
    for (uint32_t sh = 0; sh < kWfShards; sh++)
        for (int k = 0; k < 4; k++) hctl[0].shard[0][sh].n[k] = cnt[(size_t)sh * 4 + k];

    DevBuf<float4> dA, dB;
    DevBuf<uint4> dC;
    DevBuf<WfCtl> dctl;
    DevBuf<float2> dhit;
    DevBuf<uint32_t> dvis;
    HIPCHK(c, dA.alloc(hA.size())); HIPCHK(c, dB.alloc(hB.size())); HIPCHK(c, dC.alloc(hC.size()));
    HIPCHK(c, dctl.alloc(1)); HIPCHK(c, dhit.alloc(n)); HIPCHK(c, dvis.alloc(n));
    HIPCHK(c, hipMemcpyAsync(dA.p, hA.data(), hA.size() * sizeof(float4), hipMemcpyHostToDevice, c->stream));
    HIPCHK(c, hipMemcpyAsync(dB.p, hB.data(), hB.size() * sizeof(float4), hipMemcpyHostToDevice, c->stream));
    HIPCHK(c, hipMemcpyAsync(dC.p, hC.data(), hC.size() * sizeof(uint4), hipMemcpyHostToDevice, c->stream));
    HIPCHK(c, hipMemcpyAsync(dctl.p, hctl.data(), sizeof(WfCtl), hipMemcpyHostToDevice, c->stream));
    HIPCHK(c, hipMemsetAsync(dhit.p, 0xEE, n * sizeof(float2), c->stream));     // "never written": no slot, no visibility bit
    HIPCHK(c, hipMemsetAsync(dvis.p, 0xEE, n * sizeof(uint32_t), c->stream));
    W.recA = dA.p; W.recB = dB.p; W.recC = dC.p; W.ctl = dctl.p; W.hit = dhit.p; W.vis = dvis.p;
    HIPCHK(c, wf_launch_trace(W, 0u, (uint32_t)c->num_cu * wf_waves(wf_options(c)), c->stream));   // iteration 0: list parity 0, shard ring 0
    std::vector<float2> hhit(n);
    std::vector<uint32_t> hvis(n);
    HIPCHK(c, hipMemcpyAsync(hhit.data(), dhit.p, n * sizeof(float2), hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipMemcpyAsync(hvis.data(), dvis.p, n * sizeof(uint32_t), hipMemcpyDeviceToHost, c->stream));
    if (W.count) HIPCHK(c, hipMemcpyAsync(hctl[0].max_sp, dctl.p->max_sp, sizeof hctl[0].max_sp, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    if (report && W.count)
        for (uint32_t sh = 0; sh < kWfShards; sh++) report[5] = std::max<uint64_t>(report[5], hctl[0].max_sp[sh]);
    for (size_t i = 0; i < n; i++) {
        uint32_t kind;
        std::memcpy(&kind, rays + 12 * i + 7, 4);
        if (kind) {
            if (hvis[i] > 1u) return fail(c, CRT_EDEVICE, "crt_debug_trace_rays: shadow ray %zu was not resolved (vis = 0x%08x)", i, hvis[i]);
            out[2 * i] = hvis[i]; out[2 * i + 1] = 0u;
        } else {
            const uint32_t slot = f_bits(hhit[i].y);
            if (slot != kNoHit && slot >= nprim) return fail(c, CRT_EDEVICE, "crt_debug_trace_rays: ray %zu was not resolved (slot = 0x%08x)", i, slot);
            out[2 * i] = f_bits(hhit[i].x); out[2 * i + 1] = slot == kNoHit ? kNoHit : index_of[slot];
        }
    }
    return CRT_OK;
}

// Caller-chosen rays through the single-ray walks (k_debug_walk_rays: the call patterns of crt_shade.h that k_wf_finish
// and k_trace use), one lane per ray.  The buffers are the call's own.
int crt_debug_walk_rays(crt_ctx *c, int walk, const float *rays, size_t n, uint32_t *out, uint64_t report[8])
{
    if (!c || (!rays && n) || (!out && n)) return CRT_EINVAL;
    if (!c->have_scene || c->accel_mode < 0) return fail(c, CRT_ESTATE, "crt_debug_walk_rays: scene + accel required");
    if (c->accel_stale) return fail(c, CRT_ESTATE, "crt_debug_walk_rays: primitives were updated: call crt_refit_accel or crt_build_accel first");
    if (c->accel_mode != CRT_ACCEL_BVH2) return fail(c, CRT_ESTATE, "crt_debug_walk_rays: no tree (CRT_ACCEL_NONE)");
    if (walk != 0 && walk != 1) return fail(c, CRT_EINVAL, "crt_debug_walk_rays: walk must be 0 (as k_wf_finish) or 1 (as the pipeline = 0 kernel)");
    const uint32_t nprim = (uint32_t)c->prims.size();
    for (size_t i = 0; i < n; i++) {
        const float *r = rays + 12 * i;
        uint32_t u[4];
        std::memcpy(u, r + 6, 16);                               // exclude, kind, t_light, light index
        for (int k = 0; k < 6; k++)
            if (!std::isfinite(r[k])) return fail(c, CRT_EINVAL, "crt_debug_walk_rays: ray %zu is not finite (crt_trace resolves such rays without a walk)", i);
        if (u[1] > 1u) return fail(c, CRT_EINVAL, "crt_debug_walk_rays: ray %zu: kind must be 0 (extension) or 1 (shadow)", i);
        if (u[1] == 1u && (!std::isfinite(r[8]) || u[3] >= nprim))
            return fail(c, CRT_EINVAL, "crt_debug_walk_rays: shadow ray %zu: t_light must be finite and the light index below %u", i, nprim);
    }
    CRT_TRY(quiesce(c, true));
    const bool wide = c->sc.nodes4q != nullptr && c->sc.nodes8q == nullptr;     // finish_walks_wide (crt_shade.h)
    if (report) {
        report[0] = report[1] = 0;                               // rays that walked the 4-wide tree / that fell back to the BVH2
        report[2] = (uint64_t)kStackDepth;                       // stack entries per lane
        report[3] = c->bvh4.max_depth;                           // inner levels of the 4-wide tree
        report[4] = c->bvh.max_depth;                            // recorded depth of the BVH2
        report[5] = wide ? 1 : 0;
        report[6] = report[7] = 0;
    }
    if (n == 0) return CRT_OK;
    DevBuf<float> din;
    DevBuf<uint32_t> dout;
    HIPCHK(c, din.alloc(n * 12)); HIPCHK(c, dout.alloc(n * 4));
    HIPCHK(c, hipMemcpyAsync(din.p, rays, n * 12 * sizeof(float), hipMemcpyHostToDevice, c->stream));
    HIPCHK(c, hipMemsetAsync(dout.p, 0xEE, n * 4 * sizeof(uint32_t), c->stream));     // "never written"
    HIPCHK(c, launch_debug_walk_rays(c->sc, walk, din.p, n, dout.p, c->stream));
    HIPCHK(c, hipMemcpyAsync(out, dout.p, n * 4 * sizeof(uint32_t), hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    for (size_t i = 0; i < n; i++) {
        if (out[4 * i + 2] > (kWalk4q | kWalkFellBack)) return fail(c, CRT_EDEVICE, "crt_debug_walk_rays: ray %zu was not resolved (flags = 0x%08x)", i, out[4 * i + 2]);
        if (report) { report[0] += out[4 * i + 2] & kWalk4q ? 1 : 0; report[1] += out[4 * i + 2] & kWalkFellBack ? 1 : 0; }
    }
    return CRT_OK;
}

// The current structure as it lies on the device, part by part (include/crt.h): device-to-host copies only.
int crt_debug_read_accel(crt_ctx *c, int what, void *out, size_t capacity, size_t *bytes)
{
    if (!c) return CRT_EINVAL;
    if (bytes) *bytes = 0;
    if (!c->have_scene || c->accel_mode < 0) return fail(c, CRT_ESTATE, "crt_debug_read_accel: scene + accel required");
    if (c->accel_topo) return fail(c, CRT_ESTATE, "crt_debug_read_accel: the tree belongs to another primitive list: call crt_refit_accel or crt_build_accel first");
    if (what < CRT_ACCEL_PART_HEADER || what > CRT_ACCEL_PART_SLOT_OF_INDEX) return fail(c, CRT_EINVAL, "crt_debug_read_accel: unknown part %d", what);
    CRT_TRY(quiesce(c, true));
    const bool tree = c->accel_mode == CRT_ACCEL_BVH2;
    const size_t n = c->prims.size(), n2 = tree ? c->bvh.n_inner : 0, n4 = tree ? c->bvh4.n_inner : 0, n8 = tree && c->bvh8q.ok ? c->bvh8q.n_inner : 0;
    const bool device_route = tree && n4 > 0 && c->bvh4.nodes.size() < n4 * (size_t)kNode4Floats;
    const bool live4 = tree && n4 > 0 && !device_route, live4q = tree && n4 > 0 && c->sc.nodes4q != nullptr, live8q = n8 > 0 && c->sc.nodes8q != nullptr;
    double hdr[CRT_ACCEL_HEADER_N] = {0};
    const void *src = nullptr;
    size_t need = 0;
    switch (what) {
    case CRT_ACCEL_PART_HEADER: {
        const size_t lanes = (size_t)c->num_cu * wf_waves(wf_options(c)) * 64u * (size_t)std::max(1, c->wf_pipes);
        hdr[0] = c->accel_mode; hdr[1] = c->accel_builder; hdr[2] = (double)n;
        hdr[3] = tree ? c->sc.root : -1; hdr[4] = tree ? c->sc.root4 : -1; hdr[5] = live8q ? c->sc.root8 : -1;
        hdr[6] = (double)n2; hdr[7] = (double)n4; hdr[8] = (double)n8;
        hdr[9] = live4; hdr[10] = live4q; hdr[11] = live8q;
        for (int a = 0; a < 3; a++) { hdr[12 + a] = c->sc.qbase[a]; hdr[15 + a] = c->sc.qscale[a]; }
        hdr[18] = c->sc.hit_pad; hdr[19] = c->tree_pad;
        hdr[20] = c->bvh.max_depth; hdr[21] = c->bvh4.max_depth; hdr[22] = c->bvh8q.max_depth; hdr[23] = c->wf_depth;
        hdr[24] = wf_stack_need(c); hdr[25] = wf_stack_lds(c); hdr[26] = wf_overflow_levels(c);
        hdr[27] = lanes ? (double)(c->w_overflow.n / lanes) : 0.0;
        hdr[28] = c->accel_stale; hdr[29] = device_route;
        need = sizeof hdr;
        break;
    }
    case CRT_ACCEL_PART_NODES2: src = c->d_nodes.p; need = n2 * kNodeFloats * sizeof(float); break;
    case CRT_ACCEL_PART_NODES4: src = c->d_nodes4.p; need = live4 ? n4 * kNode4Floats * sizeof(float) : 0; break;
    case CRT_ACCEL_PART_NODES4Q: src = c->d_nodes4q.p; need = live4q ? n4 * 16 * sizeof(uint32_t) : 0; break;
    case CRT_ACCEL_PART_NODES8Q: src = c->d_nodes8q.p; need = live8q ? n8 * 32 * sizeof(uint32_t) : 0; break;
    case CRT_ACCEL_PART_PRIM: src = c->d_prim.p; need = n * 3 * sizeof(float4); break;
    case CRT_ACCEL_PART_PRIMD: src = c->d_primD.p; need = tree ? n * sizeof(float4) : 0; break;
    default: src = c->d_slot_of_index.p; need = n * sizeof(uint32_t); break;
    }
    if (bytes) *bytes = need;
    if (!out) return CRT_OK;
    if (capacity < need) return fail(c, CRT_EINVAL, "crt_debug_read_accel: part %d holds %zu bytes, the buffer %zu", what, need, capacity);
    if (what == CRT_ACCEL_PART_HEADER) std::memcpy(out, hdr, need);
    else if (need) HIPCHK(c, hipMemcpy(out, src, need, hipMemcpyDeviceToHost));
    return CRT_OK;
}

int crt_debug_math(crt_ctx *c, int fn, const float *a, const float *b, float *out, size_t n)
{
    if (!c || !a || !b || !out) return CRT_EINVAL;
    HIPCHK(c, hipSetDevice(c->device));
    DevBuf<float> da, db, dout;
    hipError_t e = da.alloc(n);
    if (e == hipSuccess) e = db.alloc(n);
    if (e == hipSuccess) e = dout.alloc(n);
    if (e == hipSuccess && n) e = hipMemcpyAsync(da.p, a, n * sizeof(float), hipMemcpyHostToDevice, c->stream);
    if (e == hipSuccess && n) e = hipMemcpyAsync(db.p, b, n * sizeof(float), hipMemcpyHostToDevice, c->stream);
    if (e == hipSuccess) e = launch_debug_math(fn, da.p, db.p, dout.p, n, c->stream);
    if (e == hipSuccess && n) e = hipMemcpyAsync(out, dout.p, n * sizeof(float), hipMemcpyDeviceToHost, c->stream);
    if (e == hipSuccess) e = hipStreamSynchronize(c->stream);
    if (e != hipSuccess) return fail(c, CRT_EDEVICE, "crt_debug_math: %s", hipGetErrorString(e));
    return CRT_OK;
}

int crt_debug_read_moments(crt_ctx *c, float *out)
{
    if (!c || !out) return CRT_EINVAL;
    CRT_TRY(dn_begin(c, "crt_debug_read_moments", 0, nullptr, 0, "", DN_TEMPORAL));
    if (!c->dn.cur.valid || c->dn.cur.frame != c->frame_id || !c->dn.cur.has_m)
        return fail(c, CRT_ESTATE, "crt_debug_read_moments: no crt_denoise_svgf in this frame yet, or a crt_denoise_temporal after it "
                                   "(the CURRENT slot carries no moments)");
    const size_t n = (size_t)c->tw * c->th;
    if (n) HIPCHK(c, hipMemcpyAsync(out, c->dn.cur.m.p, n * sizeof(float4), hipMemcpyDeviceToHost, c->stream));
    return dn_finish(c, n, nullptr, nullptr, nullptr);
}

int crt_debug_read_clip_box(crt_ctx *c, float *out)
{
    if (!c || !out) return CRT_EINVAL;
    CRT_TRY(dn_begin(c, "crt_debug_read_clip_box", 0, nullptr, 0, "", DN_TEMPORAL));
    if (!c->dn.cur.valid || c->dn.cur.frame != c->frame_id || !c->dn.box_ran || c->dn.clip_pct == 0)
        return fail(c, CRT_ESTATE, "crt_debug_read_clip_box: the last temporal call of this frame ran no box pass (option "
                                   "\"temporal_clip_pct\" off, no usable PREVIOUS slot, or no call in this frame yet)");
    const size_t n = (size_t)c->tw * c->th;
    if (n) HIPCHK(c, hipMemcpyAsync(out, c->dn.box.p, 2 * n * sizeof(float4), hipMemcpyDeviceToHost, c->stream));
    return dn_finish(c, n, nullptr, nullptr, nullptr);
}

// The tile classes of the context's current camera, tile rectangle and root node: the inputs of the next
// run, or of the one the flush below ends.  A run's set-up makes its table from the same inputs with the same launch.
static int tile_class_inputs(crt_ctx *c, const char *what, size_t n_tiles, WfParams &W)
{
    if (!c->have_scene || c->accel_mode < 0) return fail(c, CRT_ESTATE, "%s: scene + accel required", what);
    if (c->accel_stale) return fail(c, CRT_ESTATE, "%s: primitives were updated: call crt_refit_accel or crt_build_accel first", what);
    CRT_TRY(quiesce(c, true));
    W = WfParams{};
    W.sc = c->sc;
    W.x0 = c->x0; W.y0 = c->y0; W.tw = c->tw; W.th = c->th; W.band = c->band; W.stride = c->stride; W.phase = c->phase;
    W.tiles_x = (c->tw + 7u) / 8u; W.tiles_y = (c->th + 7u) / 8u;
    if (c->accel_mode != CRT_ACCEL_BVH2 || c->pipeline != 1 || !W.sc.nodes4q || W.sc.root4 < 0 || W.sc.root4 == 0x7FFFFFFF)
        return fail(c, CRT_ESTATE, "%s: no quantised 4-wide tree with an inner root", what);
    if (n_tiles != (size_t)W.tiles_x * W.tiles_y) return fail(c, CRT_EINVAL, "%s: the tile rectangle has %zu tiles of 8x8, not %zu", what, (size_t)W.tiles_x * W.tiles_y, n_tiles);
    return CRT_OK;
}

int crt_debug_tile_classes(crt_ctx *c, uint8_t *out, size_t n_tiles)
{
    if (!c || (!out && n_tiles)) return CRT_EINVAL;
    WfParams W;
    CRT_TRY(tile_class_inputs(c, "crt_debug_tile_classes", n_tiles, W));
    if (n_tiles == 0) return CRT_OK;
    const size_t words = (n_tiles + 15u) / 16u;
    CRT_ENSURE(c, c->w_tile_cls, words);
    std::vector<uint32_t> h(words);
    HIPCHK(c, wf_launch_tile_classes(W, c->w_tile_cls.p, c->stream));
    HIPCHK(c, hipMemcpyAsync(h.data(), c->w_tile_cls.p, words * sizeof(uint32_t), hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    for (size_t t = 0; t < n_tiles; t++) out[t] = (uint8_t)((h[t >> 4] >> (2u * (t & 15u))) & 3u);
    return CRT_OK;
}

int crt_debug_tile_classes_host(crt_ctx *c, uint8_t *out, size_t n_tiles)
{
    if (!c || (!out && n_tiles)) return CRT_EINVAL;
    WfParams W;
    CRT_TRY(tile_class_inputs(c, "crt_debug_tile_classes_host", n_tiles, W));
    TcRoot R;
    HIPCHK(c, hipMemcpy(R.q, W.sc.nodes4q + 4 * (size_t)W.sc.root4, sizeof R.q, hipMemcpyDeviceToHost));
    R.qscale = f3{W.sc.qscale[0], W.sc.qscale[1], W.sc.qscale[2]}; R.qbase = f3{W.sc.qbase[0], W.sc.qbase[1], W.sc.qbase[2]};
    const TcCam C = tc_cam(W.sc.cam, W.sc.W, W.sc.H);
    const TcTiles T{W.x0, W.y0, W.tw, W.th, W.band, W.stride, W.phase, W.tiles_x};
    for (size_t t = 0; t < n_tiles; t++) out[t] = (uint8_t)tc_tile_class(C, R, T, (uint32_t)t);
    return CRT_OK;
}

int crt_debug_tile_class_setups(crt_ctx *c, uint64_t *out)
{
    if (!c || !out) return CRT_EINVAL;
    *out = c->tile_cls_setups;
    return CRT_OK;
}

int crt_debug_mapped_gen_launches(crt_ctx *c, uint64_t *out)
{
    if (!c || !out) return CRT_EINVAL;
    *out = c->mapped_gen_launches;
    return CRT_OK;
}

int crt_debug_hit_pad(crt_ctx *c, float *out)
{
    if (!c || !out) return CRT_EINVAL;
    if (!c->have_scene) return fail(c, CRT_ESTATE, "crt_debug_hit_pad: no scene");
    *out = c->sc.hit_pad;
    return CRT_OK;
}

}  // extern "C"
