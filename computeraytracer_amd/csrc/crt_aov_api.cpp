// crt_aov_api.cpp -- the entry points of the feature planes (crt_aov.hip): crt_render_aovs, the albedo
// table it reads (crt_read_albedo_table) and the definition of one row of that table (crt_spectrum_rgb).
#include "crt_ctx.h"

using namespace crt;

extern "C" {

// The reflectance of one spectra row under an equal-energy illuminant, white Y = 1, as linear sRGB: binary64 sums with k
// ascending, the matrix of xyz_to_linear_rgb (crt_shade.h) in doubles, each result rounded once to float.
int crt_spectrum_rgb(const float *spectrum, const float *cie, float out[3])
{
    if (!spectrum || !cie || !out) return CRT_EINVAL;
    const float *cx = cie, *cy = cie + kNCie, *cz = cie + 2 * kNCie;
    double X = 0.0, Y = 0.0, Z = 0.0, N = 0.0;
    for (uint32_t k = 0; k < kNLambda; k++) {
        const double r = (double)spectrum[k];
        X += r * (double)cx[k + 40];
        Y += r * (double)cy[k + 40];
        Z += r * (double)cz[k + 40];
        N += (double)cy[k + 40];
    }
    const double x = X / N, y = Y / N, z = Z / N;
    out[0] = (float)((3.2404542 * x + -1.5371385 * y) + -0.4985314 * z);
    out[1] = (float)((-0.9692660 * x + 1.8760108 * y) + 0.0415560 * z);
    out[2] = (float)((0.0556434 * x + -0.2040259 * y) + 1.0572252 * z);
    return CRT_OK;
}

}  // extern "C"

namespace crt {

// crt_upload_scene: one crt_spectrum_rgb per spectra row, on the host.  The device copy is made by the first
// crt_render_aovs after the upload.
void aov_rebuild_albedo(crt_ctx *c, const float *spectra, size_t nspectra, const float *cie)
{
    c->albedo.assign(nspectra * 3, 0.0f);
    for (size_t i = 0; i < nspectra; i++) (void)crt_spectrum_rgb(spectra + i * kNLambda, cie, &c->albedo[3 * i]);
    c->d_albedo.release();
}

}  // namespace crt

extern "C" {

int crt_read_albedo_table(crt_ctx *c, float *out)
{
    if (!c || !out) return CRT_EINVAL;
    if (!c->have_scene) return fail(c, CRT_ESTATE, "crt_read_albedo_table: upload a scene first");
    std::memcpy(out, c->albedo.data(), c->albedo.size() * sizeof(float));
    return CRT_OK;
}

int crt_render_aovs(crt_ctx *c, uint32_t n_samples, const crt_aov_planes *out)
{
    const char *what = "crt_render_aovs";
    if (!c) return CRT_EINVAL;
    if (!out) return fail(c, CRT_EINVAL, "%s: out is NULL", what);
    // crt_read_gbuffer's refusals but the one at sample 0: an explicit n needs no sample in the accumulator
    CRT_TRY(dn_check_state(c, what, true));
    const bool per_tile = n_samples == 0 && c->as_on;
    if (per_tile && c->as_broken) return as_refuse_broken(c, what);
    if (n_samples == 0 && !c->as_on && c->sample == 0)
        return fail(c, CRT_ESTATE, "%s: n_samples = 0 means the samples the accumulator holds, and it holds none", what);
    const unsigned long long n_max = n_samples ? n_samples : per_tile ? c->as_requested : c->sample;
    if ((unsigned long long)c->sample_offset + n_max > 0xFFFFFFFFull)
        return fail(c, CRT_EINVAL, "%s: sample offset %u + %llu samples pass 2^32 - 1", what, c->sample_offset, n_max);
    CRT_TRY(quiesce(c, false));
    const size_t n = (size_t)c->tw * c->th;
    if (n) {
        // every allocation before the first launch: a failed one leaves nothing enqueued
        crt_ctx::Aov &a = c->aov;
        if (out->hits) CRT_ENSURE(c, a.hits, n);
        if (out->alpha) CRT_ENSURE(c, a.alpha, n);
        if (out->depth) CRT_ENSURE(c, a.depth, n);
        if (out->normal) CRT_ENSURE(c, a.normal, n);
        if (out->albedo) CRT_ENSURE(c, a.albedo, n);
        if (c->d_albedo.n < c->albedo.size()) {
            HIPCHK(c, c->d_albedo.alloc(c->albedo.size()));
            const hipError_t e = hipMemcpy(c->d_albedo.p, c->albedo.data(), c->albedo.size() * sizeof(float), hipMemcpyHostToDevice);
            if (e != hipSuccess) c->d_albedo.release();
            HIPCHK(c, e);
        }
        AovParams P{};
        P.albedo = c->d_albedo.p;
        P.counts = per_tile ? c->as_counts.p : nullptr;
        P.hits = out->hits ? a.hits.p : nullptr;
        P.alpha = out->alpha ? a.alpha.p : nullptr;
        P.depth = out->depth ? a.depth.p : nullptr;
        P.normal = out->normal ? a.normal.p : nullptr;
        P.albedo_out = out->albedo ? a.albedo.p : nullptr;
        P.x0 = c->x0; P.y0 = c->y0; P.tw = c->tw; P.th = c->th; P.tiles_x = (c->tw + 7) / 8;
        P.first = c->sample_offset;
        P.n = n_samples ? n_samples : c->sample;
        P.brute = c->accel_mode == CRT_ACCEL_NONE;
        HIPCHK(c, aov_launch(c->sc, P, c->stream));
        if (out->hits) HIPCHK(c, hipMemcpyAsync(out->hits, a.hits.p, n * sizeof(uint32_t), hipMemcpyDeviceToHost, c->stream));
        if (out->alpha) HIPCHK(c, hipMemcpyAsync(out->alpha, a.alpha.p, n * sizeof(float), hipMemcpyDeviceToHost, c->stream));
        if (out->depth) HIPCHK(c, hipMemcpyAsync(out->depth, a.depth.p, n * sizeof(float), hipMemcpyDeviceToHost, c->stream));
        if (out->normal) HIPCHK(c, hipMemcpyAsync(out->normal, a.normal.p, n * sizeof(float4), hipMemcpyDeviceToHost, c->stream));
        if (out->albedo) HIPCHK(c, hipMemcpyAsync(out->albedo, a.albedo.p, n * sizeof(float4), hipMemcpyDeviceToHost, c->stream));
    }
    return dn_finish(c, n, nullptr, nullptr, nullptr);
}

}  // extern "C"
