// crt_radiance_api.cpp -- the entry points of the radiance queries (crt_radiance.hip): crt_radiance_rays
// (host pointers, the context's query stream and staging) and crt_radiance_rays_device (device pointers, the caller's
// stream).  Neither flushes: they read the scene, the lights, the spectra tables and the tree, which only sync points change.
#include "crt_ctx.h"

using namespace crt;

namespace {

bool aligned16(const void *p) { return ((uintptr_t)p & 15u) == 0; }

// The refusals the two calls share, in the header's order.  Nothing here touches the device.
int radiance_check(crt_ctx *c, const char *what, const crt_ray *rays, const crt_path_key *keys, size_t n, uint32_t n_samples,
                   const crt_radiance_planes *out)
{
    if (!out) return fail(c, CRT_EINVAL, "%s: out is NULL", what);
    if (!out->xyz && !out->y2 && !out->rgba8) return fail(c, CRT_EINVAL, "%s: every plane is NULL", what);
    if (!rays && n) return fail(c, CRT_EINVAL, "%s: rays is NULL with n = %zu", what, n);
    if (!aligned16(rays) || !aligned16(keys) || !aligned16(out->xyz))
        return fail(c, CRT_EINVAL, "%s: rays, keys and the xyz plane must be 16-byte aligned", what);
    if (n >= ((unsigned long long)1 << 32)) return fail(c, CRT_EINVAL, "%s: n = %zu, must be below 2^32", what, n);
    if (n_samples == 0) return fail(c, CRT_EINVAL, "%s: n_samples is 0", what);
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

// The compute units of the context's device (they size the persistent grid): asked once.
int radiance_num_cu(crt_ctx *c)
{
    if (c->num_cu == 0) {
        hipDeviceProp_t prop;
        HIPCHK(c, hipGetDeviceProperties(&prop, c->device));
        c->num_cu = prop.multiProcessorCount > 0 ? prop.multiProcessorCount : 256;
    }
    return CRT_OK;
}

RadianceParams radiance_params(crt_ctx *c, size_t n, uint32_t n_samples, const crt_radiance_planes &p)
{
    RadianceParams P{};
    P.xyz = (float4 *)p.xyz; P.y2 = p.y2; P.rgba8 = (uchar4 *)p.rgba8;
    P.n = n;
    P.n_samples = n_samples;
    P.wide_ok = c->pipeline == 1;
    return P;
}

}  // namespace

extern "C" {

// Every allocation first; then the uploads, the launch and the planes' copies on the query stream, and a wait for that
// stream alone.
int crt_radiance_rays(crt_ctx *c, const crt_ray *rays, const crt_path_key *keys, size_t n, uint32_t n_samples,
                      const crt_radiance_planes *out)
{
    const char *what = "crt_radiance_rays";
    if (!c) return CRT_EINVAL;
    CRT_TRY(radiance_check(c, what, rays, keys, n, n_samples, out));
    if (n == 0) return CRT_OK;
    HIPCHK(c, hipSetDevice(c->device));
    CRT_TRY(radiance_num_cu(c));
    crt_ctx::Query &q = c->query;
    if (!q.stream) HIPCHK(c, q.stream.create(hipStreamNonBlocking));
    HIPCHK(c, stage(q.rays, 2 * n));
    if (keys) HIPCHK(c, stage(q.keys, n));
    crt_radiance_planes dev{};
    if (out->xyz) { HIPCHK(c, stage(q.rad_xyz, n)); dev.xyz = (float *)q.rad_xyz.p; }
    if (out->y2) { HIPCHK(c, stage(q.rad_y2, n)); dev.y2 = q.rad_y2.p; }
    if (out->rgba8) { HIPCHK(c, stage(q.rad_rgba8, n)); dev.rgba8 = (uint8_t *)q.rad_rgba8.p; }
    RadianceParams P = radiance_params(c, n, n_samples, dev);
    P.rays = q.rays.p;
    P.keys = keys ? q.keys.p : nullptr;
    const hipStream_t s = q.stream;
    hipError_t e = hipMemcpyAsync(q.rays.p, rays, n * sizeof(crt_ray), hipMemcpyHostToDevice, s);
    if (e == hipSuccess && keys) e = hipMemcpyAsync(q.keys.p, keys, n * sizeof(crt_path_key), hipMemcpyHostToDevice, s);
    if (e == hipSuccess) e = radiance_launch(c->sc, P, c->accel_mode == CRT_ACCEL_NONE, (uint32_t)c->num_cu, s);
    if (e == hipSuccess && out->xyz) e = hipMemcpyAsync(out->xyz, dev.xyz, n * 16, hipMemcpyDeviceToHost, s);
    if (e == hipSuccess && out->y2) e = hipMemcpyAsync(out->y2, dev.y2, n * 4, hipMemcpyDeviceToHost, s);
    if (e == hipSuccess && out->rgba8) e = hipMemcpyAsync(out->rgba8, dev.rgba8, n * 4, hipMemcpyDeviceToHost, s);
    const hipError_t es = hipStreamSynchronize(s);               // (also after a failure: the staging is idle when the call returns)
    if (e == hipSuccess) e = es;
    if (e != hipSuccess) return fail(c, CRT_EDEVICE, "%s: %s", what, hipGetErrorString(e));
    return CRT_OK;
}

int crt_radiance_rays_device(crt_ctx *c, const crt_ray *rays_dev, const crt_path_key *keys_dev, size_t n, uint32_t n_samples,
                             const crt_radiance_planes *out_dev, void *hip_stream)
{
    const char *what = "crt_radiance_rays_device";
    if (!c) return CRT_EINVAL;
    CRT_TRY(radiance_check(c, what, rays_dev, keys_dev, n, n_samples, out_dev));
    if (n == 0) return CRT_OK;
    HIPCHK(c, hipSetDevice(c->device));
    CRT_TRY(radiance_num_cu(c));
    RadianceParams P = radiance_params(c, n, n_samples, *out_dev);
    P.rays = (const float4 *)rays_dev;
    P.keys = (const uint4 *)keys_dev;
    HIPCHK(c, radiance_launch(c->sc, P, c->accel_mode == CRT_ACCEL_NONE, (uint32_t)c->num_cu, (hipStream_t)hip_stream));
    return CRT_OK;
}

int crt_debug_radiance_lanes(crt_ctx *c, size_t n, uint64_t *out)
{
    if (!c || !out) return CRT_EINVAL;
    HIPCHK(c, hipSetDevice(c->device));
    CRT_TRY(radiance_num_cu(c));
    *out = (uint64_t)radiance_blocks(n, (uint32_t)c->num_cu) * 64u;
    return CRT_OK;
}

}  // extern "C"
