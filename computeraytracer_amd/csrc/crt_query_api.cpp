// crt_query_api.cpp -- the entry points of the ray queries (crt_query.hip): crt_query_rays and crt_pick
// (host pointers, the context's own query stream and staging) and crt_query_rays_device (device pointers, the caller's
// stream).  None of them flushes: they read the scene, the tree and the id table, which only sync points change.
#include "crt_ctx.h"

using namespace crt;

namespace {

bool aligned16(const void *p) { return ((uintptr_t)p & 15u) == 0; }

// The refusals the three calls share, in the header's order.  Nothing here touches the device.
int query_check(crt_ctx *c, const char *what, const void *in, const char *in_name, bool in_rays, size_t n, int mode,
                const crt_query_planes *out)
{
    if (!out) return fail(c, CRT_EINVAL, "%s: out is NULL", what);
    if (mode != CRT_QUERY_CLOSEST && mode != CRT_QUERY_ANY) return fail(c, CRT_EINVAL, "%s: unknown mode %d", what, mode);
    const bool others = out->prim || out->id || out->t || out->position || out->normal || out->uv;
    if (!out->hit && !others) return fail(c, CRT_EINVAL, "%s: every plane is NULL", what);
    if (mode == CRT_QUERY_ANY && others)
        return fail(c, CRT_EINVAL, "%s: CRT_QUERY_ANY reports `hit` alone (which primitive ends the walk depends on the tree): every other plane must be NULL", what);
    if (!in && n) return fail(c, CRT_EINVAL, "%s: %s is NULL with n = %zu", what, in_name, n);
    if (in_rays && !aligned16(in)) return fail(c, CRT_EINVAL, "%s: %s must be 16-byte aligned", what, in_name);
    if (!aligned16(out->position) || !aligned16(out->normal))
        return fail(c, CRT_EINVAL, "%s: the position and normal planes must be 16-byte aligned", what);
    if (n >= ((unsigned long long)1 << 32)) return fail(c, CRT_EINVAL, "%s: n = %zu, must be below 2^32", what, n);
    if (!c->have_scene || c->accel_mode < 0) return fail(c, CRT_ESTATE, "%s: scene + accel required", what);
    if (c->accel_stale) return fail(c, CRT_ESTATE, "%s: primitives were updated: call crt_refit_accel or crt_build_accel first", what);
    return CRT_OK;
}

// Grow a staging buffer to n elements, by at least half (DevBuf::alloc frees the old one first: hipFree waits for the device).
template <typename T>
hipError_t stage(DevBuf<T> &b, size_t n)
{
    if (b.n >= n) return hipSuccess;
    return b.alloc(std::max(n, b.n + b.n / 2));
}

QueryParams query_params(crt_ctx *c, size_t n, const crt_query_planes &p)
{
    QueryParams P{};
    P.table = p.id ? c->d_prim_ids.p : nullptr;
    P.hit = p.hit; P.prim = p.prim; P.id = p.id; P.t = p.t;
    P.position = (float4 *)p.position; P.normal = (float4 *)p.normal; P.uv = (float2 *)p.uv;
    P.n = n;
    P.wide_ok = c->pipeline == 1;
    return P;
}

// The host forms: `in` is n crt_ray records, or with pick n pixel pairs.  Every allocation first; then the upload, the
// launch and the planes' copies on the query stream, and a wait for that stream alone.
int query_host(crt_ctx *c, const char *what, const void *in, size_t n, int mode, bool pick, const crt_query_planes *out)
{
    HIPCHK(c, hipSetDevice(c->device));
    crt_ctx::Query &q = c->query;
    if (!q.stream) HIPCHK(c, q.stream.create(hipStreamNonBlocking));
    if (pick) HIPCHK(c, stage(q.xy, n)); else HIPCHK(c, stage(q.rays, 2 * n));
    crt_query_planes dev{};
    if (out->hit) { HIPCHK(c, stage(q.hit, n)); dev.hit = q.hit.p; }
    if (out->prim) { HIPCHK(c, stage(q.prim, n)); dev.prim = q.prim.p; }
    if (out->id) { HIPCHK(c, stage(q.id, n)); dev.id = q.id.p; }
    if (out->t) { HIPCHK(c, stage(q.t, n)); dev.t = q.t.p; }
    if (out->position) { HIPCHK(c, stage(q.position, n)); dev.position = (float *)q.position.p; }
    if (out->normal) { HIPCHK(c, stage(q.normal, n)); dev.normal = (float *)q.normal.p; }
    if (out->uv) { HIPCHK(c, stage(q.uv, n)); dev.uv = (float *)q.uv.p; }
    if (out->id) CRT_TRY(matte_ids_device(c));
    QueryParams P = query_params(c, n, dev);
    const hipStream_t s = q.stream;
    hipError_t e;
    if (pick) { P.xy = q.xy.p; e = hipMemcpyAsync(q.xy.p, in, n * sizeof(uint2), hipMemcpyHostToDevice, s); }
    else { P.rays = q.rays.p; e = hipMemcpyAsync(q.rays.p, in, n * sizeof(crt_ray), hipMemcpyHostToDevice, s); }
    if (e == hipSuccess) e = query_launch(c->sc, P, mode, pick, c->accel_mode == CRT_ACCEL_NONE, s);
#define CRT_QUERY_BACK(plane, bytes) \
    if (e == hipSuccess && out->plane) e = hipMemcpyAsync(out->plane, dev.plane, n * (bytes), hipMemcpyDeviceToHost, s);
    CRT_QUERY_BACK(hit, 4) CRT_QUERY_BACK(prim, 4) CRT_QUERY_BACK(id, 4) CRT_QUERY_BACK(t, 4)
    CRT_QUERY_BACK(position, 16) CRT_QUERY_BACK(normal, 16) CRT_QUERY_BACK(uv, 8)
#undef CRT_QUERY_BACK
    const hipError_t es = hipStreamSynchronize(s);               // (also after a failure: the staging is idle when the call returns)
    if (e == hipSuccess) e = es;
    if (e != hipSuccess) return fail(c, CRT_EDEVICE, "%s: %s", what, hipGetErrorString(e));
    return CRT_OK;
}

}  // namespace

extern "C" {

int crt_query_rays(crt_ctx *c, const crt_ray *rays, size_t n, int mode, const crt_query_planes *out)
{
    const char *what = "crt_query_rays";
    if (!c) return CRT_EINVAL;
    CRT_TRY(query_check(c, what, rays, "rays", true, n, mode, out));
    if (n == 0) return CRT_OK;
    return query_host(c, what, rays, n, mode, false, out);
}

int crt_query_rays_device(crt_ctx *c, const crt_ray *rays_dev, size_t n, int mode, const crt_query_planes *out_dev, void *hip_stream)
{
    const char *what = "crt_query_rays_device";
    if (!c) return CRT_EINVAL;
    CRT_TRY(query_check(c, what, rays_dev, "rays_dev", true, n, mode, out_dev));
    if (n == 0) return CRT_OK;
    HIPCHK(c, hipSetDevice(c->device));
    if (out_dev->id) CRT_TRY(matte_ids_device(c));
    QueryParams P = query_params(c, n, *out_dev);
    P.rays = (const float4 *)rays_dev;
    HIPCHK(c, query_launch(c->sc, P, mode, false, c->accel_mode == CRT_ACCEL_NONE, (hipStream_t)hip_stream));
    return CRT_OK;
}

int crt_pick(crt_ctx *c, const uint32_t *xy, size_t n, const crt_query_planes *out)
{
    const char *what = "crt_pick";
    if (!c) return CRT_EINVAL;
    CRT_TRY(query_check(c, what, xy, "xy", false, n, CRT_QUERY_CLOSEST, out));
    for (size_t i = 0; i < n; i++)
        if (xy[2 * i] >= c->W || xy[2 * i + 1] >= c->H)
            return fail(c, CRT_EINVAL, "%s: pixel %zu is (%u, %u), outside the %u x %u image (coordinates are global: crt_set_tile does not move them)",
                        what, i, xy[2 * i], xy[2 * i + 1], c->W, c->H);
    if (n == 0) return CRT_OK;
    return query_host(c, what, xy, n, CRT_QUERY_CLOSEST, true, out);
}

}  // extern "C"
