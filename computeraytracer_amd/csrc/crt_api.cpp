// crt_api.cpp -- the C ABI of include/crt.h on top of the gfx950 kernels: the context's life, the tile, crt_trace and
// crt_sync, the adaptive calls, reads / writes / binds, counters, timers and options.  (The other host units: crt_ctx.h.)
//
// Host-side responsibilities (the reference does these in src/main.js):
//   upload   main.js:147-393  -> crt_upload_scene (80-byte records -> device layout)
//   state    main.js:298-311  -> accumulator + sample counter owned by the context
//   dispatch main.js:597-611  -> crt_trace(n) == n x {sample++ ; trace}
#include "crt_ctx.h"

using namespace crt;

extern "C" void crt_comm_on_destroy(crt_ctx *c);                 // crt_comm.cpp: the context's communicator goes with it
extern "C" int crt_internal_comm_partitioned(crt_ctx *c);

namespace crt {

long long g_fail_alloc_in = 0;

namespace {
std::string g_create_error;
}

int fail(crt_ctx *c, int code, const char *fmt, ...)
{
    char buf[2048];
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(buf, sizeof buf, fmt, ap);
    va_end(ap);
    if (c) c->err = buf; else g_create_error = buf;
    return code;
}

int quiesce(crt_ctx *c, bool sync)
{
    HIPCHK(c, hipSetDevice(c->device));
    CRT_TRY(wf_flush(c));
    if (sync) HIPCHK(c, hipStreamSynchronize(c->stream));
    return CRT_OK;
}

// (the frame ring alone: option "frame_ring" changes it without touching the accumulator)
int alloc_frames(crt_ctx *c)
{
    const size_t n = (size_t)c->tw * c->th;
    if (c->frame_ring) HIPCHK(c, c->d_frames.alloc(n * c->frame_ring)); else c->d_frames.release();
    c->frame_batch.assign(c->frame_ring, 0);
    if (c->frame_ring && !c->read_stream) HIPCHK(c, c->read_stream.create(hipStreamNonBlocking));
    return CRT_OK;
}

int alloc_tile(crt_ctx *c)
{
    c->as_on = false; c->as_broken = false;                      // (the adaptive buffers are the tile's: next use sizes them)
    c->as_counts.release(); c->as_errors.release(); c->as_flags.release(); c->as_active.release(); c->as_q.release();
    size_t n = (size_t)c->tw * c->th;
    HIPCHK(c, c->d_accum.alloc(n));
    HIPCHK(c, c->d_rgba.alloc(n));
    return alloc_frames(c);
}

int zero_state(crt_ctx *c)
{
    size_t n = (size_t)c->tw * c->th;
    if (n) {
        HIPCHK(c, hipMemsetAsync(accum_ptr(c), 0, n * sizeof(float4), c->stream));
        HIPCHK(c, hipMemsetAsync(rgba_ptr(c), 0, n * sizeof(uchar4), c->stream));
    }
    c->sample = 0; c->published = 0; c->pending = 0; c->resolved_upto = 0; c->ring_from = 1;
    c->as_on = false; c->as_broken = false;
    c->frame_id++;
    return CRT_OK;
}

// The calls that assume one sample count for the whole tile refuse the adaptive state.
int as_refuse(crt_ctx *c, const char *what)
{
    return fail(c, CRT_ESTATE, "%s: the context is in the adaptive state (per-tile sample counts: crt_read_adaptive; crt_reset "
                               "returns to uniform sampling)", what);
}

int as_refuse_broken(crt_ctx *c, const char *what)
{
    return fail(c, CRT_ESTATE, "%s: an earlier crt_trace_adaptive failed part way (the tile counts lag the accumulator): "
                               "crt_reset first", what);
}

}  // namespace crt

namespace {

// What a new tile (crt_set_tile, crt_set_row_bands) ends with: the denoise state dropped, the outputs unbound and
// allocated, the frame state zeroed.
int retile(crt_ctx *c)
{
    c->dn.valid = false; c->fdn.valid = false;
    c->dn.drop();
    c->accum_bound = nullptr; c->rgba_bound = nullptr;
    CRT_TRY(alloc_tile(c));
    return zero_state(c);
}

// The single-kernel form's parameters (crt_trace, crt_trace_adaptive without the wavefront pipeline).
TraceParams trace_params(crt_ctx *c)
{
    TraceParams P{};
    P.sc = c->sc;
    P.x0 = c->x0; P.y0 = c->y0; P.tw = c->tw; P.th = c->th;
    P.band = c->band; P.stride = c->stride; P.phase = c->phase;
    P.accum = accum_ptr(c); P.rgba = rgba_ptr(c);
    P.counters = c->counting ? c->d_counters.p : nullptr;
    P.tiles_x = (c->tw + 7) / 8; P.tiles_y = (c->th + 7) / 8;        // main.js:606-610
    return P;
}

// What the two timers wait for first: everything of the last crt_trace, its closing event included.
int last_timed(crt_ctx *c, const char *what)
{
    if (!c->last_timed) return fail(c, CRT_ESTATE, "%s: no crt_trace yet", what);
    CRT_TRY(quiesce(c, false));
    HIPCHK(c, hipEventSynchronize(c->ev1));
    return CRT_OK;
}

}  // namespace

extern "C" {

int crt_abi_version(void) { return CRT_ABI_VERSION; }

// (for crt_comm.cpp, which is written against the public ABI: an error with the context's message)
int crt_internal_fail(crt_ctx *c, int code, const char *msg) { return fail(c, code, "%s", msg); }

int crt_get_device(crt_ctx *c, int *out)
{
    if (!c || !out) return CRT_EINVAL;
    *out = c->device;
    return CRT_OK;
}

int crt_get_stream(crt_ctx *c, void **out)
{
    if (!c || !out) return CRT_EINVAL;
    *out = (void *)c->stream;
    return CRT_OK;
}

int crt_image_size(crt_ctx *c, uint32_t out[2])
{
    if (!c || !out) return CRT_EINVAL;
    if (!c->have_scene) return fail(c, CRT_ESTATE, "crt_image_size: upload a scene first");
    out[0] = c->W; out[1] = c->H;
    return CRT_OK;
}

const char *crt_last_error(crt_ctx *ctx) { return ctx ? ctx->err.c_str() : g_create_error.c_str(); }

int crt_create(crt_ctx **out, int device_ordinal)
{
    if (!out) return fail(nullptr, CRT_EINVAL, "crt_create: out is NULL");
    *out = nullptr;
    int ndev = 0;
    hipError_t e = hipGetDeviceCount(&ndev);
    if (e != hipSuccess || ndev <= 0)
        return fail(nullptr, CRT_EDEVICE, "crt_create: no HIP device (%s); there is no CPU fallback",
                    e != hipSuccess ? hipGetErrorString(e) : "device count 0");
    if (device_ordinal < 0 || device_ordinal >= ndev)
        return fail(nullptr, CRT_EINVAL, "crt_create: device %d out of range (0..%d)", device_ordinal, ndev - 1);
    crt_ctx *c = new crt_ctx();
    c->device = device_ordinal;
    if ((e = hipSetDevice(device_ordinal)) != hipSuccess ||
        (e = c->own_stream.create(hipStreamNonBlocking)) != hipSuccess ||
        (e = c->ev0.create()) != hipSuccess || (e = c->ev1.create()) != hipSuccess ||
        (e = c->d_counters.alloc(CRT_NCOUNTERS)) != hipSuccess ||
        (e = hipMemset(c->d_counters.p, 0, CRT_NCOUNTERS * sizeof(unsigned long long))) != hipSuccess) {
        int rc = fail(nullptr, CRT_EDEVICE, "crt_create: %s", hipGetErrorString(e));
        crt_destroy(c);
        return rc;
    }
    c->stream = c->own_stream;
    *out = c;
    return CRT_OK;
}

void crt_destroy(crt_ctx *c)
{
    if (!c) return;
    crt_comm_on_destroy(c);
    (void)hipSetDevice(c->device);
    // parked work is abandoned, but every stream must have drained before the buffers go (they go with the context)
    if (c->stream) (void)hipStreamSynchronize(c->stream);       // (ours, or an adopted one: that one is only drained)
    c->own_stream.sync();
    for (const Stream &s : c->pipe_stream) s.sync();
    c->pub_stream.sync();
    for (const Stream &s : c->fin_stream) s.sync();
    c->read_stream.sync();
    c->query.stream.sync();
    delete c;
}

int crt_upload_scene(crt_ctx *c, const void *primitives, size_t nprim, const void *lights, size_t nlight,
                     const float *spectra, size_t nspectra, const float *cie, const float camera[16])
{
    if (!c) return CRT_EINVAL;
    if ((!primitives && nprim) || !lights || !spectra || !cie || !camera)
        return fail(c, CRT_EINVAL, "crt_upload_scene: NULL buffer");
    if (nlight < 1) return fail(c, CRT_EINVAL, "crt_upload_scene: at least one light record is required");
    if (nspectra < 1 || nspectra > 0x3FFF) return fail(c, CRT_EINVAL, "crt_upload_scene: nspectra must be 1..16383");
    if (nprim >= (1u << 28)) return fail(c, CRT_EINVAL, "crt_upload_scene: too many primitives");
    if (!(camera[11] >= 1.0f && camera[12] >= 1.0f && camera[11] <= 65536.0f && camera[12] <= 65536.0f))
        return fail(c, CRT_EINVAL, "crt_upload_scene: camera width/height (floats 11,12) must be 1..65536");
    CRT_TRY(quiesce(c, true));

    std::vector<HostPrim> prims(nprim), lts(nlight);
    for (size_t i = 0; i < nprim; i++) {
        prims[i] = read_prim((const uint8_t *)primitives, i);
        const HostPrim &p = prims[i];
        if (p.category > 2u) return fail(c, CRT_EINVAL, "primitive %zu: category %u not in {0,1,2}", i, p.category);
        if (p.material > 2u) return fail(c, CRT_EINVAL, "primitive %zu: material %u not in {0,1,2}", i, p.material);
        if (p.index != (uint32_t)i)
            return fail(c, CRT_EINVAL, "primitive %zu: data4.w (index) is %u, must equal the array position "
                                       "(src/main.js:124,133)", i, p.index);
        if (p.emission >= nspectra || p.reflectance >= nspectra)
            return fail(c, CRT_EINVAL, "primitive %zu: spectrum index out of range", i);
    }
    for (size_t i = 0; i < nlight; i++) {
        lts[i] = read_prim((const uint8_t *)lights, i);
        if (lts[i].emission >= nspectra) return fail(c, CRT_EINVAL, "light %zu: emission index out of range", i);
    }
    // from here on the old scene is gone: a failure below must not leave a context that can still trace
    c->have_scene = false;
    c->accel_mode = -1;
    c->dn.valid = false; c->fdn.valid = false;
    c->sample_offset = 0;
    c->dn.drop();
    c->prims.swap(prims);
    c->prims_moved = false;
    matte_ids_identity(c);                                       // (host only: DESIGN.md 6o)
    c->query.release();                                          // (the ray queries' staging: DESIGN.md 6p)
    c->lights.swap(lts);
    std::memcpy(c->camera, camera, sizeof c->camera);
    c->W = (uint32_t)camera[11];                                 // ComputeShader.wgsl:85
    c->H = (uint32_t)camera[12];

    DevScene &S = c->sc;
    S = DevScene{};
    S.W = c->W; S.H = c->H;
    S.nspectra = (uint32_t)nspectra;
    S.nlight = (uint32_t)nlight;
    S.inv_nlight = 1.0f / (float)S.nlight;                       // :372-373
    c->s_prims = prims_scale(c->prims);
    S.hit_pad = pad_of(c->s_prims, c->camera);                  // = scene_hit_pad(c->prims, c->camera)
    c->accel_stale = false; c->accel_topo = false;
    c->rf_ready = false;
    S.nf_last[0] = S.nf_last[1] = kNoHit;
    for (size_t i = c->prims.size(); i-- > 0 && S.nf_last[1] == kNoHit;)
        if (c->prims[i].category != 2u) (S.nf_last[0] == kNoHit ? S.nf_last[0] : S.nf_last[1]) = (uint32_t)i;
    camera_frame(c->camera, S.cam);

    HIPCHK(c, c->d_raw.alloc(std::max<size_t>(nprim * 80, 16)));
    if (nprim) HIPCHK(c, hipMemcpy(c->d_raw.p, primitives, nprim * 80, hipMemcpyHostToDevice));
    HIPCHK(c, c->d_spectra.alloc(nspectra * kNLambda));
    HIPCHK(c, hipMemcpy(c->d_spectra.p, spectra, nspectra * kNLambda * sizeof(float), hipMemcpyHostToDevice));
    HIPCHK(c, c->d_cie.alloc(3 * kNCie));
    HIPCHK(c, hipMemcpy(c->d_cie.p, cie, 3 * kNCie * sizeof(float), hipMemcpyHostToDevice));
    c->cie_zero = tc_culled_is_zero(cie);                        // (what k_wf_gen stores for a MISS tile's chunk: DESIGN.md 5.9)
    aov_rebuild_albedo(c, spectra, nspectra, cie);               // (host only: DESIGN.md 6n)
    std::vector<float4> hl(nlight * 3);
    for (size_t i = 0; i < nlight; i++) light_rows(c->lights[i], &hl[3 * i]);
    HIPCHK(c, c->d_lights.alloc(hl.size()));
    HIPCHK(c, hipMemcpy(c->d_lights.p, hl.data(), hl.size() * sizeof(float4), hipMemcpyHostToDevice));
    S.spectra = c->d_spectra.p; S.cie = c->d_cie.p; S.lights = c->d_lights.p;

    c->x0 = 0; c->y0 = 0; c->tw = c->W; c->th = c->H;
    c->band = 0x40000000u; c->stride = 1; c->phase = 0;
    c->accum_bound = nullptr; c->rgba_bound = nullptr;
    c->have_scene = true;                                        // (alloc_tile / zero_state below need it for the error paths of others)
    int rc = alloc_tile(c);
    if (rc == CRT_OK) rc = zero_state(c);
    if (rc) c->have_scene = false;
    return rc;
}

int crt_set_tile(crt_ctx *c, uint32_t x0, uint32_t y0, uint32_t x1, uint32_t y1)
{
    if (!c) return CRT_EINVAL;
    if (!c->have_scene) return fail(c, CRT_ESTATE, "crt_set_tile: upload a scene first");
    if (x0 > x1 || y0 > y1 || x1 > c->W || y1 > c->H)
        return fail(c, CRT_EINVAL, "crt_set_tile: rectangle [%u,%u)x[%u,%u) outside %ux%u", x0, x1, y0, y1, c->W, c->H);
    CRT_TRY(quiesce(c, true));
    c->x0 = x0; c->y0 = y0; c->tw = x1 - x0; c->th = y1 - y0;
    c->band = 0x40000000u; c->stride = 1; c->phase = 0;
    return retile(c);
}

int crt_set_row_bands(crt_ctx *c, uint32_t band_rows, uint32_t parts, uint32_t part)
{
    if (!c) return CRT_EINVAL;
    if (!c->have_scene) return fail(c, CRT_ESTATE, "crt_set_row_bands: upload a scene first");
    if (band_rows == 0 || parts == 0 || part >= parts || band_rows > 65536u)
        return fail(c, CRT_EINVAL, "crt_set_row_bands: need band_rows >= 1 and part < parts");
    CRT_TRY(quiesce(c, true));
    uint32_t rows = 0;                                   // rows y of the frame with (y / band) % parts == part
    for (uint32_t b = part; (unsigned long long)b * band_rows < c->H; b += parts)
        rows += std::min<uint32_t>(band_rows, c->H - b * band_rows);
    c->x0 = 0; c->y0 = 0; c->tw = c->W; c->th = rows;
    c->band = band_rows; c->stride = parts; c->phase = part;
    return retile(c);
}

int crt_build_accel(crt_ctx *c, int mode)
{
    if (!c) return CRT_EINVAL;
    if (!c->have_scene) return fail(c, CRT_ESTATE, "crt_build_accel: upload a scene first");
    if (mode != CRT_ACCEL_NONE && mode != CRT_ACCEL_BVH2 && mode != CRT_ACCEL_LBVH && mode != CRT_ACCEL_PLOC)
        return fail(c, CRT_EINVAL, "crt_build_accel: unknown mode %d", mode);
    c->want_builder = mode == CRT_ACCEL_LBVH ? 1 : mode == CRT_ACCEL_PLOC ? 2 : 0;
    if (c->want_builder) mode = CRT_ACCEL_BVH2;                 // same structure, same kernels
    CRT_TRY(quiesce(c, true));
    // The build releases the scene's device arrays before it allocates the new ones: until it has succeeded there is
    // no structure to trace against (upload_geometry / build_accel_on_device set accel_mode on success only).
    c->accel_mode = -1;
    c->dn.valid = false; c->fdn.valid = false;
    return build_tree(c, mode);
}

int crt_reset(crt_ctx *c)
{
    if (!c) return CRT_EINVAL;
    if (!c->have_scene) return fail(c, CRT_ESTATE, "crt_reset: upload a scene first");
    CRT_TRY(quiesce(c, false));
    return zero_state(c);
}

int crt_trace(crt_ctx *c, uint32_t n_samples)
{
    if (!c) return CRT_EINVAL;
    if (c->as_on) return as_refuse(c, "crt_trace");
    if (!c->have_scene) return fail(c, CRT_ESTATE, "crt_trace: upload a scene first");
    if (c->accel_mode < 0) return fail(c, CRT_ESTATE, "crt_trace: call crt_build_accel first");
    if (c->accel_stale) return fail(c, CRT_ESTATE, "crt_trace: primitives were updated: call crt_refit_accel or crt_build_accel first");
    if (c->sample_offset) {
        if (!(c->pipeline == 1 && c->accel_mode == CRT_ACCEL_BVH2))
            return fail(c, CRT_ESTATE, "crt_trace: a sample offset needs the wavefront pipeline (\"pipeline\" = 1 and a tree): "
                                       "crt_set_sample_offset(ctx, 0) first");
        if ((unsigned long long)c->sample_offset + c->sample + n_samples > 0xFFFFFFFFull)
            return fail(c, CRT_EINVAL, "crt_trace: sample offset %u + %u samples so far + %u pass 2^32 - 1", c->sample_offset, c->sample, n_samples);
    }
    HIPCHK(c, hipSetDevice(c->device));
    if ((size_t)c->tw * c->th != 0 && (!accum_ptr(c) || !rgba_ptr(c)))
        return fail(c, CRT_ENOMEM, "crt_trace: the tile's output buffers are not allocated (an earlier crt_set_tile / crt_set_row_bands failed)");
    TraceParams P = trace_params(c);
    c->last_launches = 0;
    c->last_timed = true;
    c->last_iterations = 0;
    HIPCHK(c, hipEventRecord(c->ev0, c->stream));
    uint32_t left = n_samples;
    if (c->pipeline == 1 && c->accel_mode == CRT_ACCEL_BVH2) {
        c->sample += n_samples; c->pending += n_samples;
        CRT_TRY(wf_tick(c));
        CRT_TRY(wf_publish_pending(c, false));                   // (what was not published is not part of the frame)
    } else {
        CRT_TRY(wf_flush(c));
        uint32_t chunk = c->spp_per_launch ? c->spp_per_launch : 8u;
        while (left) {
            uint32_t n = std::min(left, chunk);
            P.first_sample = c->published + 1;                            // UpdateVariables.wgsl: sample++ first
            P.n_samples = n;
            HIPCHK(c, launch_trace(P, c->counting, c->accel_mode == CRT_ACCEL_NONE, c->stream));
            c->published += n; c->sample += n; c->resolved_upto = c->published;
            left -= n;
            c->last_launches++;
        }
    }
    HIPCHK(c, hipEventRecord(c->ev1, c->stream));
    return CRT_OK;
}

int crt_sync(crt_ctx *c)
{
    if (!c) return CRT_EINVAL;
    CRT_TRY(quiesce(c, true));
    return wf_check_dropped(c);
}

// ---------------------------------------------------------------- adaptive sampling (crt_adaptive.hip)
static AsParams as_params(crt_ctx *c, const crt_adaptive_params &p)
{
    AsParams A{};
    A.accum = accum_ptr(c); A.q = c->as_q.p; A.counts = c->as_counts.p; A.errors = c->as_errors.p; A.flags = c->as_flags.p;
    A.active = c->as_active.p; A.n_active = c->as_n.p;
    A.tw = c->tw; A.th = c->th; A.tiles_x = (c->tw + 7) / 8; A.tiles_y = (c->th + 7) / 8;
    A.min_samples = p.min_samples; A.max_samples = p.max_samples; A.threshold = p.threshold;
    return A;
}

// Enter the adaptive state: every tile at 0 samples, Q = 0 (the accumulator is at sample 0 already).
static int as_begin(crt_ctx *c)
{
    const size_t ntiles = std::max<size_t>((size_t)((c->tw + 7) / 8) * ((c->th + 7) / 8), 1);
    const size_t npix = std::max<size_t>((size_t)c->tw * c->th, 1);
    CRT_ENSURE(c, c->as_counts, ntiles);
    CRT_ENSURE(c, c->as_errors, ntiles);
    CRT_ENSURE(c, c->as_flags, ntiles);
    CRT_ENSURE(c, c->as_active, ntiles);
    CRT_ENSURE(c, c->as_n, 1);
    CRT_ENSURE(c, c->as_q, npix);
    HIPCHK(c, hipMemsetAsync(c->as_counts.p, 0, ntiles * sizeof(uint32_t), c->stream));
    HIPCHK(c, hipMemsetAsync(c->as_q.p, 0, npix * sizeof(float), c->stream));
    c->as_on = true;
    c->as_requested = 0;
    return CRT_OK;
}

// The defaults (tools/adaptive_bench.py): rounds of 64 samples reach tau in 0.60 / 0.62 of the wall time of
// rounds of 16 on S2 / the Cornell box at 1080p for 1.07 / 1.03 times the pixel-samples (each round flushes, selects and
// reads back); min_samples guards tiles whose first samples miss a rare path; max_samples bounds the tiles that do not
// reach tau = 0.01 (0.9 % of S2's tiles at 4096 samples).
static const crt_adaptive_params kAsDefaults = {64u, 32u, 4096u, 0.01f};

int crt_adaptive_defaults(crt_adaptive_params *out)
{
    if (!out) return CRT_EINVAL;
    *out = kAsDefaults;
    return CRT_OK;
}

// E' of every tile from the variance plane the adaptive filter left, in E's place.
static AsVarParams as_var_params(crt_ctx *c, const crt_adaptive_params &p, const float *var)
{
    const AsParams A = as_params(c, p);
    return AsVarParams{var, A.counts, A.errors, A.flags, A.tw, A.th, A.tiles_x, A.tiles_y, A.min_samples, A.max_samples, A.threshold};
}

// crt_trace_adaptive and crt_trace_adaptive_filtered (`filter` set; `what` names the call): they differ in the selection.
static int as_trace(crt_ctx *c, const char *what, const crt_adaptive_params *params, const crt_denoise_adaptive_params *filter,
                    bool filtered, uint32_t *active_tiles)
{
    if (!c) return CRT_EINVAL;
    const crt_adaptive_params p = params ? *params : kAsDefaults;
    if (p.samples == 0) return fail(c, CRT_EINVAL, "%s: samples must be >= 1", what);
    if (!(p.threshold >= 0.0f && p.threshold <= FLT_MAX)) return fail(c, CRT_EINVAL, "%s: threshold must be finite and >= 0", what);
    crt_denoise_adaptive_params dp{};
    if (filtered) CRT_TRY(dn_adaptive_params(c, what, filter, &dp));
    if (p.max_samples != 0 && p.max_samples < p.min_samples)
        return fail(c, CRT_EINVAL, "%s: max_samples %u < min_samples %u", what, p.max_samples, p.min_samples);
    if (!c->have_scene) return fail(c, CRT_ESTATE, "crt_trace: upload a scene first");
    if (c->accel_mode < 0) return fail(c, CRT_ESTATE, "crt_trace: call crt_build_accel first");
    if (c->accel_stale) return fail(c, CRT_ESTATE, "crt_trace: primitives were updated: call crt_refit_accel or crt_build_accel first");
    // (a band partition of a multiple of 8 rows: every local 8x8 tile is one of the frame's)
    if (crt_internal_comm_partitioned(c) == 1)
        return fail(c, CRT_ESTATE, "%s: not under this crt_comm_partition: its 8x8 tiles are not the frame's "
                                   "(a band partition with band_rows a multiple of 8 is what works)", what);
    if (c->as_broken) return as_refuse_broken(c, what);
    if (filtered) CRT_TRY(dn_check_state(c, what, true));         // (where crt_denoise_adaptive refuses: row bands)
    if (c->sample_offset && !c->adaptive_temporal)
        return fail(c, CRT_ESTATE, "%s: not with a sample offset (%u): crt_set_sample_offset(ctx, 0) first "
                                   "(or option \"adaptive_temporal\" = 1)", what, c->sample_offset);
    if (!c->as_on && c->sample > 0)
        return fail(c, CRT_ESTATE, "%s: the context holds %u uniform samples whose second moment was not kept: crt_reset first", what, c->sample);
    // (no tile holds more than the calls of this adaptive state have asked for: what bounds every tile's last index)
    const unsigned long long requested = c->as_on ? c->as_requested : 0ull;
    if (c->sample_offset) {
        if (!(c->pipeline == 1 && c->accel_mode == CRT_ACCEL_BVH2))
            return fail(c, CRT_ESTATE, "%s: a sample offset needs the wavefront pipeline (\"pipeline\" = 1 and a tree): "
                                       "crt_set_sample_offset(ctx, 0) first", what);
        if ((unsigned long long)c->sample_offset + requested + p.samples > 0xFFFFFFFFull)
            return fail(c, CRT_EINVAL, "%s: sample offset %u + %llu samples requested so far + %u pass 2^32 - 1",
                        what, c->sample_offset, requested, p.samples);
    }
    HIPCHK(c, hipSetDevice(c->device));
    if ((size_t)c->tw * c->th != 0 && (!accum_ptr(c) || !rgba_ptr(c)))
        return fail(c, CRT_ENOMEM, "%s: the tile's output buffers are not allocated (an earlier crt_set_tile / crt_set_row_bands failed)", what);
    CRT_TRY(wf_flush(c));                 // (the selection reads the accumulator)
    const bool entering = !c->as_on;
    if (entering) CRT_TRY(as_begin(c));
    const uint32_t tiles_x = (c->tw + 7) / 8, tiles_y = (c->th + 7) / 8;
    uint32_t n_active = 0;
    if (tiles_x * tiles_y) {
        if (filtered && !entering) {
            // the filter's own launches, then E' from the variance they leave; every allocation comes before the first launch
            float4 *res = nullptr;
            const float *var = nullptr;
            CRT_TRY(dn_adaptive_run(c, dp, false, true, &res, &var));
            const AsParams A = as_params(c, p);
            HIPCHK(c, as_launch_select_var(as_var_params(c, p, var), &A, c->stream));
        } else {
            // (entering the state every count is 0 and every tile active under either rule: no filter, no G-buffer)
            HIPCHK(c, as_launch_select(as_params(c, p), true, c->stream));
        }
        HIPCHK(c, hipMemcpyAsync(&n_active, c->as_n.p, sizeof n_active, hipMemcpyDeviceToHost, c->stream));
        HIPCHK(c, hipStreamSynchronize(c->stream));
        CRT_TRY(wf_check_dropped(c));
    }
    if (active_tiles) *active_tiles = n_active;
    if (n_active == 0) return CRT_OK;
    c->as_requested = requested + p.samples;
    c->last_launches = 0;
    c->last_timed = true;
    c->last_iterations = 0;
    HIPCHK(c, hipEventRecord(c->ev0, c->stream));
    if (c->pipeline == 1 && c->accel_mode == CRT_ACCEL_BVH2) {
        const uint32_t cap = wf_batch_cap(wf_options(c));
        for (uint32_t off = 0; off < p.samples;) {
            const uint32_t take = std::min(p.samples - off, cap);
            const AsBatch ab{off, n_active, off + take == p.samples ? p.samples : 0u};
            int rc = wf_trace_batch(c, take, &ab);
            if (rc) { c->as_broken = true; return rc; }              // (samples of this call may be in the accumulator already)
            off += take;
        }
    } else {
        TraceParams P = trace_params(c);
        const AsTiles A{c->as_active.p, c->as_counts.p, c->as_q.p, n_active};
        const uint32_t chunk = c->spp_per_launch ? c->spp_per_launch : 8u;
        for (uint32_t off = 0; off < p.samples;) {
            const uint32_t n = std::min(p.samples - off, chunk);
            P.first_sample = off + 1u;                           // + the tile's count (k_trace)
            P.n_samples = n;
            const hipError_t e = launch_trace_adaptive(P, A, c->counting, c->accel_mode == CRT_ACCEL_NONE, c->stream);
            if (e != hipSuccess) { c->as_broken = true; HIPCHK(c, e); }
            c->last_launches++;
            off += n;
        }
        const hipError_t e = as_launch_commit(c->as_counts.p, c->as_active.p, n_active, p.samples, c->stream);
        if (e != hipSuccess) { c->as_broken = true; HIPCHK(c, e); }
    }
    HIPCHK(c, hipEventRecord(c->ev1, c->stream));
    return CRT_OK;
}

int crt_trace_adaptive(crt_ctx *c, const crt_adaptive_params *params, uint32_t *active_tiles)
{
    return as_trace(c, "crt_trace_adaptive", params, nullptr, false, active_tiles);
}

int crt_trace_adaptive_filtered(crt_ctx *c, const crt_adaptive_params *params, const crt_denoise_adaptive_params *filter,
                                uint32_t *active_tiles)
{
    return as_trace(c, "crt_trace_adaptive_filtered", params, filter, true, active_tiles);
}

int crt_read_adaptive(crt_ctx *c, uint32_t *counts, float *errors)
{
    if (!c) return CRT_EINVAL;
    if (!c->as_on) return fail(c, CRT_ESTATE, "crt_read_adaptive: the context is in the uniform state (crt_trace_adaptive first)");
    if (c->as_broken) return as_refuse_broken(c, "crt_read_adaptive");
    CRT_TRY(quiesce(c, false));
    const size_t ntiles = (size_t)((c->tw + 7) / 8) * ((c->th + 7) / 8);
    if (ntiles) {
        // (the selection's thresholds do not enter E: any will do; the active list is left alone)
        HIPCHK(c, as_launch_select(as_params(c, crt_adaptive_params{1u, 0u, 0u, 0.0f}), false, c->stream));
        if (counts) HIPCHK(c, hipMemcpyAsync(counts, c->as_counts.p, ntiles * sizeof(uint32_t), hipMemcpyDeviceToHost, c->stream));
        if (errors) HIPCHK(c, hipMemcpyAsync(errors, c->as_errors.p, ntiles * sizeof(float), hipMemcpyDeviceToHost, c->stream));
    }
    HIPCHK(c, hipStreamSynchronize(c->stream));
    return wf_check_dropped(c);
}

int crt_read_adaptive_filtered(crt_ctx *c, const crt_denoise_adaptive_params *filter, uint32_t *counts, float *errors)
{
    if (!c) return CRT_EINVAL;
    const char *what = "crt_read_adaptive_filtered";
    crt_denoise_adaptive_params dp{};
    CRT_TRY(dn_adaptive_params(c, what, filter, &dp));
    if (!c->as_on) return fail(c, CRT_ESTATE, "%s: the context is in the uniform state (crt_trace_adaptive_filtered first)", what);
    if (c->as_broken) return as_refuse_broken(c, what);
    CRT_TRY(dn_check_state(c, what, true));
    CRT_TRY(quiesce(c, false));
    const size_t ntiles = (size_t)((c->tw + 7) / 8) * ((c->th + 7) / 8);
    if (ntiles) {
        float4 *res = nullptr;
        const float *var = nullptr;
        CRT_TRY(dn_adaptive_run(c, dp, false, true, &res, &var));
        // (as in crt_read_adaptive the thresholds do not enter E', and the active list is left alone)
        HIPCHK(c, as_launch_select_var(as_var_params(c, crt_adaptive_params{1u, 0u, 0u, 0.0f}, var), nullptr, c->stream));
        if (counts) HIPCHK(c, hipMemcpyAsync(counts, c->as_counts.p, ntiles * sizeof(uint32_t), hipMemcpyDeviceToHost, c->stream));
        if (errors) HIPCHK(c, hipMemcpyAsync(errors, c->as_errors.p, ntiles * sizeof(float), hipMemcpyDeviceToHost, c->stream));
    }
    HIPCHK(c, hipStreamSynchronize(c->stream));
    return wf_check_dropped(c);
}

// crt_comm.cpp (CRT_GATHER_PREVIEW and the frame-level calls): the context's frame state.  out[0] = 0 uniform, 1 adaptive;
// out[1] = the uniform sample count; out[2] = the epoch of the frame state (what zero_state and crt_write_accum bump).
// With `finish`, a sync point first, as crt_read_adaptive is one: everything in flight is finished.  q_dev / counts_dev
// (may be NULL) receive the adaptive state's device buffers: Q per tile pixel, the count per 8x8 tile.
int crt_internal_frame_state(crt_ctx *c, int finish, const char *who, uint32_t out[3], void **q_dev, void **counts_dev)
{
    if (!c || !out) return CRT_EINVAL;
    if (c->as_on && c->as_broken) return as_refuse_broken(c, who);
    if (finish) CRT_TRY(quiesce(c, false));
    out[0] = c->as_on ? 1u : 0u; out[1] = c->as_on ? 0u : c->sample; out[2] = c->frame_id;
    if (q_dev) *q_dev = c->as_on ? c->as_q.p : nullptr;
    if (counts_dev) *counts_dev = c->as_on ? c->as_counts.p : nullptr;
    return CRT_OK;
}

int crt_sample_count(crt_ctx *c, uint32_t *out)
{
    if (!c || !out) return CRT_EINVAL;
    if (c->as_on) return as_refuse(c, "crt_sample_count");
    *out = c->sample;
    return CRT_OK;
}

int crt_tile(crt_ctx *c, uint32_t out[4])
{
    if (!c || !out) return CRT_EINVAL;
    out[0] = c->x0; out[1] = c->y0; out[2] = c->tw; out[3] = c->th;
    return CRT_OK;
}

int crt_read_accum(crt_ctx *c, float *out)
{
    if (!c || !out) return CRT_EINVAL;
    if (!c->have_scene) return fail(c, CRT_ESTATE, "crt_read_accum: no scene");
    CRT_TRY(quiesce(c, false));
    size_t n = (size_t)c->tw * c->th;
    if (n) HIPCHK(c, hipMemcpyAsync(out, accum_ptr(c), n * sizeof(float4), hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    return wf_check_dropped(c);
}

int crt_read_rgba8(crt_ctx *c, uint8_t *out)
{
    if (!c || !out) return CRT_EINVAL;
    if (!c->have_scene) return fail(c, CRT_ESTATE, "crt_read_rgba8: no scene");
    CRT_TRY(quiesce(c, false));
    size_t n = (size_t)c->tw * c->th;
    if (n) HIPCHK(c, hipMemcpyAsync(out, rgba_ptr(c), n * sizeof(uchar4), hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    return wf_check_dropped(c);
}

// Page-lock caller memory so that readbacks into it run at PCIe speed (an 8 MB 1080p frame: 0.15 ms instead of 1.5-2.5 ms
// through the runtime's staging of pageable memory) -- what a display loop that shows every frame wants for its frame buffer.
int crt_pin_host(void *ptr, size_t bytes)
{
    if (!ptr || !bytes) return CRT_EINVAL;
    const hipError_t e = hipHostRegister(ptr, bytes, hipHostRegisterDefault);
    if (e != hipSuccess) { (void)hipGetLastError(); return fail(nullptr, CRT_EDEVICE, "crt_pin_host: %s", hipGetErrorString(e)); }
    return CRT_OK;
}

int crt_unpin_host(void *ptr)
{
    if (!ptr) return CRT_EINVAL;
    const hipError_t e = hipHostUnregister(ptr);
    if (e != hipSuccess) { (void)hipGetLastError(); return fail(nullptr, CRT_EDEVICE, "crt_unpin_host: %s", hipGetErrorString(e)); }
    return CRT_OK;
}

int crt_latest_sample(crt_ctx *c, uint32_t *out)
{
    if (!c || !out) return CRT_EINVAL;
    if (c->as_on) return as_refuse(c, "crt_latest_sample");
    if (c->run && c->run->live) { HIPCHK(c, hipSetDevice(c->device)); CRT_TRY(wf_tick(c)); }   // (retire what has finished meanwhile)
    *out = c->resolved_upto;
    return CRT_OK;
}

int crt_read_latest_rgba8(crt_ctx *c, uint8_t *out, uint32_t *sample)
{
    if (!c || !out) return CRT_EINVAL;
    if (!c->have_scene) return fail(c, CRT_ESTATE, "crt_read_latest_rgba8: no scene");
    if (c->as_on) return as_refuse(c, "crt_read_latest_rgba8");
    HIPCHK(c, hipSetDevice(c->device));
    if (c->run && c->run->live) CRT_TRY(wf_tick(c));
    // No flush: in stream order the framebuffer holds the complete frame of the newest batch whose resolve pass has been
    // enqueued (crt_trace's contract for bound outputs); the copy is queued behind it.
    const uint32_t s = c->resolved_upto;
    const size_t n = (size_t)c->tw * c->th;
    if (n) HIPCHK(c, hipMemcpyAsync(out, rgba_ptr(c), n * sizeof(uchar4), hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    if (sample) *sample = s;
    return CRT_OK;
}

int crt_read_sample_rgba8(crt_ctx *c, uint32_t sample, uint8_t *out)
{
    if (!c || !out) return CRT_EINVAL;
    if (!c->have_scene) return fail(c, CRT_ESTATE, "crt_read_sample_rgba8: no scene");
    if (c->as_on) return as_refuse(c, "crt_read_sample_rgba8");
    if (!c->frame_ring || !c->d_frames.p) return fail(c, CRT_ESTATE, "crt_read_sample_rgba8: set option frame_ring first (frames kept per sample)");
    if (sample == 0 || sample > c->sample) return fail(c, CRT_EINVAL, "crt_read_sample_rgba8: sample %u has not been requested (1..%u)", sample, c->sample);
    if (sample < c->ring_from) return fail(c, CRT_EINVAL, "crt_read_sample_rgba8: sample %u was not traced by this context since its last reset / crt_write_accum (frames from %u on)", sample, c->ring_from);
    if (c->sample - sample >= c->frame_ring) return fail(c, CRT_EINVAL, "crt_read_sample_rgba8: sample %u has left the ring of %u frames (%u requested)", sample, c->frame_ring, c->sample);
    if (c->pipeline != 1 || c->accel_mode != CRT_ACCEL_BVH2) return fail(c, CRT_ESTATE, "crt_read_sample_rgba8: frames are kept by the wavefront pipeline only");
    HIPCHK(c, hipSetDevice(c->device));
    CRT_TRY(wf_wait_sample(c, sample));
    // The copy waits for the resolve pass that wrote this frame (the batch id's event: a later re-recording of it only
    // orders more), on a stream of its own -- not for the finish / resolve work of later batches queued on the context's.
    const size_t n = (size_t)c->tw * c->th;
    const uint32_t slot = (sample - 1u) % c->frame_ring;
    if (c->run && c->run->resolved_recorded[c->frame_batch[slot]]) HIPCHK(c, hipStreamWaitEvent(c->read_stream, c->ev_resolved[c->frame_batch[slot]], 0));
    else HIPCHK(c, hipStreamSynchronize(c->stream));
    if (n) HIPCHK(c, hipMemcpyAsync(out, c->d_frames.p + (size_t)slot * n, n * sizeof(uchar4), hipMemcpyDeviceToHost, c->read_stream));
    HIPCHK(c, hipStreamSynchronize(c->read_stream));
    return CRT_OK;
}

int crt_write_accum(crt_ctx *c, const float *in, uint32_t sample)
{
    if (!c || !in) return CRT_EINVAL;
    if (!c->have_scene) return fail(c, CRT_ESTATE, "crt_write_accum: no scene");
    CRT_TRY(quiesce(c, false));
    size_t n = (size_t)c->tw * c->th;
    if (n) HIPCHK(c, hipMemcpyAsync(accum_ptr(c), in, n * sizeof(float4), hipMemcpyHostToDevice, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    c->sample = sample; c->published = sample; c->pending = 0; c->resolved_upto = sample; c->ring_from = sample + 1u;
    c->as_on = false; c->as_broken = false;                      // (the restored accumulator is a uniform one)
    c->frame_id++;
    c->dn.drop();
    return CRT_OK;
}

int crt_device_buffers(crt_ctx *c, void **accum_dev, void **rgba8_dev)
{
    if (!c) return CRT_EINVAL;
    if (accum_dev) *accum_dev = accum_ptr(c);
    if (rgba8_dev) *rgba8_dev = rgba_ptr(c);
    return CRT_OK;
}

int crt_bind_output(crt_ctx *c, void *accum_dev, void *rgba8_dev)
{
    if (!c) return CRT_EINVAL;
    if (!c->have_scene) return fail(c, CRT_ESTATE, "crt_bind_output: upload a scene first");
    if (((uintptr_t)accum_dev & 15u) || ((uintptr_t)rgba8_dev & 3u))
        return fail(c, CRT_EINVAL, "crt_bind_output: accum must be 16-byte and rgba8 4-byte aligned");
    CRT_TRY(quiesce(c, true));
    c->accum_bound = (float4 *)accum_dev;
    c->rgba_bound = (uchar4 *)rgba8_dev;
    return CRT_OK;
}

int crt_set_stream(crt_ctx *c, void *hip_stream)
{
    if (!c) return CRT_EINVAL;
    CRT_TRY(quiesce(c, true));
    c->stream = hip_stream ? (hipStream_t)hip_stream : c->own_stream.s;
    return CRT_OK;
}

int crt_enable_counters(crt_ctx *c, int on)
{
    if (!c) return CRT_EINVAL;
    CRT_TRY(wf_flush(c));
    c->counting = on != 0;
    return CRT_OK;
}

int crt_debug_probes(crt_ctx *c, uint64_t out[8])
{
    if (!c || !out) return CRT_EINVAL;
    for (int k = 0; k < 8; k++) out[k] = c->probes[k];
    return CRT_OK;
}

int crt_reset_counters(crt_ctx *c)
{
    if (!c) return CRT_EINVAL;
    for (int k = 0; k < 8; k++) c->probes[k] = 0;
    HIPCHK(c, hipSetDevice(c->device));
    HIPCHK(c, hipMemsetAsync(c->d_counters.p, 0, CRT_NCOUNTERS * sizeof(unsigned long long), c->stream));
    // (k_wf_gen's own count lives in the pipes' control blocks; every run's pipes start behind the context's stream)
    for (int p = 0; p < crt_ctx::kMaxPipes; p++)
        if (c->w_ctl[p].p) {
            HIPCHK(c, hipMemsetAsync(&c->w_ctl[p].p->gen_culled[0], 0, sizeof(unsigned long long) * kWfShards, c->stream));
            HIPCHK(c, hipMemsetAsync(&c->w_ctl[p].p->deferred_nee[0], 0, sizeof(unsigned long long) * kWfShards, c->stream));
        }
    return CRT_OK;
}

int crt_debug_gen_culled(crt_ctx *c, uint64_t *out)
{
    if (!c || !out) return CRT_EINVAL;
    CRT_TRY(quiesce(c, true));
    uint64_t n = 0;
    for (int p = 0; p < crt_ctx::kMaxPipes; p++) {
        if (!c->w_ctl[p].p) continue;
        unsigned long long sh[kWfShards];
        HIPCHK(c, hipMemcpy(sh, &c->w_ctl[p].p->gen_culled[0], sizeof sh, hipMemcpyDeviceToHost));
        for (uint32_t s_ = 0; s_ < kWfShards; s_++) n += sh[s_];
    }
    *out = n;
    return CRT_OK;
}

int crt_debug_deferred_nee(crt_ctx *c, uint64_t *out)
{
    if (!c || !out) return CRT_EINVAL;
    CRT_TRY(quiesce(c, true));
    uint64_t n = 0;
    for (int p = 0; p < crt_ctx::kMaxPipes; p++) {
        if (!c->w_ctl[p].p) continue;
        unsigned long long sh[kWfShards];
        HIPCHK(c, hipMemcpy(sh, &c->w_ctl[p].p->deferred_nee[0], sizeof sh, hipMemcpyDeviceToHost));
        for (uint32_t s_ = 0; s_ < kWfShards; s_++) n += sh[s_];
    }
    *out = n;
    return CRT_OK;
}

int crt_counters(crt_ctx *c, uint64_t out[CRT_NCOUNTERS])
{
    if (!c || !out) return CRT_EINVAL;
    CRT_TRY(quiesce(c, false));
    HIPCHK(c, hipMemcpyAsync(out, c->d_counters.p, CRT_NCOUNTERS * sizeof(uint64_t), hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    return CRT_OK;
}

int crt_last_trace_ms(crt_ctx *c, float *ms, uint32_t *launches)
{
    if (!c) return CRT_EINVAL;
    CRT_TRY(last_timed(c, "crt_last_trace_ms"));
    float t = 0.0f;
    HIPCHK(c, hipEventElapsedTime(&t, c->ev0, c->ev1));
    c->last_ms = t;
    if (ms) *ms = t;
    if (launches) *launches = c->last_launches;
    return CRT_OK;
}

int crt_last_kernel_ms(crt_ctx *c, float *ms, uint32_t *launches)
{
    if (!c) return CRT_EINVAL;
    CRT_TRY(last_timed(c, "crt_last_kernel_ms"));
    float total = 0.0f;
    uint32_t n = 0;
    if (c->pipeline == 1 && c->accel_mode == CRT_ACCEL_BVH2) {
        if (!c->time_kernels) return fail(c, CRT_ESTATE, "crt_last_kernel_ms: set option time_kernels=1 before crt_trace");
        HIPCHK(c, hipStreamSynchronize(c->stream));
        n = c->last_trace_kernel_launches;
        for (uint32_t i = 0; i < n; i++) {
            float t = 0.0f;
            HIPCHK(c, hipEventElapsedTime(&t, c->kev[2 * (size_t)i], c->kev[2 * (size_t)i + 1]));
            total += t;
        }
        c->last_trace_kernel_launches = 0;               // the next query starts a new interval
    } else {
        HIPCHK(c, hipEventElapsedTime(&total, c->ev0, c->ev1));
        n = c->last_launches;
    }
    if (ms) *ms = total;
    if (launches) *launches = n;
    return CRT_OK;
}

int crt_accel_stats(crt_ctx *c, uint64_t out[8])
{
    if (!c || !out) return CRT_EINVAL;
    if (c->accel_topo) return fail(c, CRT_ESTATE, "crt_accel_stats: the tree belongs to another primitive list: call crt_refit_accel or crt_build_accel first");
    const bool wide = c->pipeline == 1 && c->accel_mode == CRT_ACCEL_BVH2 && c->bvh4.n_inner > 0;
    const bool wide8 = wide && c->bvh8q.ok;
    out[4] = wide ? (c->bvh4q.ok ? 16 : 32) : 32;      // bytes of node data per child box tested
    out[5] = wide8 ? 8 : wide ? 4 : 2;                  // node width used by crt_trace
    out[6] = wide8 ? c->bvh8q.n_inner : wide ? c->bvh4.n_inner : c->bvh.n_inner;   // inner nodes of that tree
    out[7] = (uint64_t)c->accel_builder;               // 0: host binned SAH, 1: GPU LBVH, 2: GPU PLOC
    out[0] = c->bvh.n_inner; out[1] = c->bvh.n_leaves; out[2] = c->bvh.max_depth;
    out[3] = (uint64_t)c->bvh.n_inner * 64u + (uint64_t)c->bvh4.n_inner * 128u + (uint64_t)c->prims.size() * 48u;
    return CRT_OK;
}

int crt_set_option(crt_ctx *c, const char *name, int64_t value)
{
    if (!c || !name) return CRT_EINVAL;
    CRT_TRY(wf_flush(c));
    if (!std::strcmp(name, "debug_fail_alloc")) { g_fail_alloc_in = value; return CRT_OK; }
    if (!std::strcmp(name, "ploc_radius")) {                 // takes effect at crt_build_accel
        if (value < 1 || value > 32) return fail(c, CRT_EINVAL, "crt_set_option: ploc_radius is 1..32");
        c->ploc.radius = (uint32_t)value;
        return CRT_OK;
    }
    if (!std::strcmp(name, "refit_rebuild_pct")) {           // crt_refit_accel's rebuild policy (include/crt.h crt_accel_quality)
        if (value != 0 && (value < 100 || value > 100000)) return fail(c, CRT_EINVAL, "crt_set_option: refit_rebuild_pct is 0 (off) or 100..100000");
        c->refit_rebuild_pct = (int)value;
        return CRT_OK;
    }
    if (!std::strcmp(name, "debug_ploc_max_depth")) {       // test hooks: a PLOC build past these is abandoned for the LBVH
        if (value < 1 || value > 62) return fail(c, CRT_EINVAL, "crt_set_option: debug_ploc_max_depth is 1..62");
        c->ploc.max_depth = (uint32_t)value;
        return CRT_OK;
    }
    if (!std::strcmp(name, "debug_ploc_max_rounds")) {
        if (value < 1) return fail(c, CRT_EINVAL, "crt_set_option: debug_ploc_max_rounds is >= 1");
        c->ploc.max_rounds = (uint32_t)std::min<int64_t>(value, 1 << 30);
        return CRT_OK;
    }
    if (!std::strcmp(name, "wf_defer")) { c->wf_defer = value != 0; return CRT_OK; }
    if (!std::strcmp(name, "spp_per_launch")) { c->spp_per_launch = (uint32_t)std::max<int64_t>(0, value); return CRT_OK; }
    if (!std::strcmp(name, "pipeline")) { c->pipeline = value ? 1 : 0; return CRT_OK; }
    if (!std::strcmp(name, "quantize")) { c->quantize = value ? 1 : 0; return CRT_OK; }   // takes effect at crt_build_accel
    if (!std::strcmp(name, "wf_width")) { c->wf_width = value == 4 ? 4 : 8; return CRT_OK; }   // takes effect at crt_build_accel
    if (!std::strcmp(name, "wf_finish_at")) { c->wf_finish_at = (uint32_t)std::max<int64_t>(0, value); return CRT_OK; }
    if (!std::strcmp(name, "wf_flush_at")) { c->wf_flush_at = (uint32_t)std::max<int64_t>(0, value); return CRT_OK; }
    if (!std::strcmp(name, "wf_side_ppw")) { c->wf_side_ppw = (uint32_t)std::min<int64_t>(64, std::max<int64_t>(1, value)); return CRT_OK; }
    if (!std::strcmp(name, "wf_flush_ppw")) { c->wf_flush_ppw = (uint32_t)std::min<int64_t>(64, std::max<int64_t>(1, value)); return CRT_OK; }
    if (!std::strcmp(name, "wf_ring")) { c->wf_ring = (int)std::min<int64_t>((int64_t)kWfRing, std::max<int64_t>(2, value)); return CRT_OK; }
    if (!std::strcmp(name, "wf_chunk")) { c->wf_chunk = (int)std::min<int64_t>(16, std::max<int64_t>(1, value)); return CRT_OK; }
    if (!std::strcmp(name, "wf_cohort")) { c->wf_cohort = (int)std::min<int64_t>(256, std::max<int64_t>(1, value)); return CRT_OK; }
    if (!std::strcmp(name, "wf_ahead")) { c->wf_ahead = (int)std::min<int64_t>(32, std::max<int64_t>(2, value)); return CRT_OK; }
    if (!std::strcmp(name, "wf_pool_spp")) { c->wf_pool_spp = (int)std::min<int64_t>(64, std::max<int64_t>(1, value)); return CRT_OK; }
    if (!std::strcmp(name, "wf_feed_pct")) { c->wf_feed = (double)std::min<int64_t>(400, std::max<int64_t>(10, value)) / 100.0; return CRT_OK; }
    if (!std::strcmp(name, "wf_tail_walk")) { c->wf_tail_walk = value != 0; return CRT_OK; }
    if (!std::strcmp(name, "temporal_motion")) {
        if (value != 0 && value != 1) return fail(c, CRT_EINVAL, "crt_set_option: temporal_motion is 0 or 1");
        if (!value && (c->dn.cur.snap || c->dn.prev.snap)) c->dn.drop();    // (history across an edit is this option's)
        if (!value) c->dn.snap.release();
        c->dn.motion = value != 0;
        return CRT_OK;
    }
    if (!std::strcmp(name, "adaptive_temporal")) {          // (nothing is dropped either way)
        if (value != 0 && value != 1) return fail(c, CRT_EINVAL, "crt_set_option: adaptive_temporal is 0 or 1");
        c->adaptive_temporal = value != 0;
        return CRT_OK;
    }
    if (!std::strcmp(name, "svgf_spatial_pct")) {           // (nothing is dropped: history does not depend on it)
        if (value != 0 && (value < 25 || value > 10000)) return fail(c, CRT_EINVAL, "crt_set_option: svgf_spatial_pct is 0 (off) or 25..10000");
        c->svgf_spatial_pct = (int)value;
        return CRT_OK;
    }
    if (!std::strcmp(name, "denoise_latest_wave_blocks")) {  // 
        if (value != 0 && value != 1) return fail(c, CRT_EINVAL, "crt_set_option: denoise_latest_wave_blocks is 0 or 1");
        c->dn.wave_blocks = value != 0;
        return CRT_OK;
    }
    if (!std::strcmp(name, "temporal_clip_pct")) {          // 
        if (value != 0 && (value < 25 || value > 10000)) return fail(c, CRT_EINVAL, "crt_set_option: temporal_clip_pct is 0 (off) or 25..10000");
        if (!value && c->dn.relit) c->dn.drop();               // (history across a light edit is this option's)
        if (!value) { c->dn.box.release(); c->dn.box_ran = false; }
        c->dn.clip_pct = (int)value;
        return CRT_OK;
    }
    if (!std::strcmp(name, "frame_ring")) {
        c->frame_ring = (uint32_t)std::min<int64_t>(256, std::max<int64_t>(0, value));
        c->ring_from = c->sample + 1u;                          // (a new ring starts empty)
        if (c->have_scene) { HIPCHK(c, hipSetDevice(c->device)); HIPCHK(c, hipStreamSynchronize(c->stream)); return alloc_frames(c); }
        return CRT_OK;
    }
    if (!std::strcmp(name, "wf_gen_blocks")) { c->wf_gen_blocks = (int)std::min<int64_t>(4096, std::max<int64_t>(1, value)); return CRT_OK; }
    if (!std::strcmp(name, "wf_trace_form")) { c->wf_trace_form = value == 1 ? 1 : 2; return CRT_OK; }
    if (!std::strcmp(name, "wf_cull_miss")) { c->wf_cull_miss = value != 0; return CRT_OK; }
    if (!std::strcmp(name, "wf_cull_classes")) { c->wf_cull_classes = value != 0; return CRT_OK; }
    if (!std::strcmp(name, "wf_defer_nee")) { c->wf_defer_nee = value != 0; return CRT_OK; }
    if (!std::strcmp(name, "wf_affinity")) { c->wf_affinity = value != 0; return CRT_OK; }   // read when a batch is published
    if (!std::strcmp(name, "wf_pipes")) { c->wf_pipes = (int)std::min<int64_t>(crt_ctx::kMaxPipes, std::max<int64_t>(1, value)); return CRT_OK; }
    if (!std::strcmp(name, "wf_pool")) { c->wf_pool = (uint32_t)std::max<int64_t>(0, value); return CRT_OK; }
    if (!std::strcmp(name, "wf_waves_per_cu")) { c->wf_waves_per_cu = (uint32_t)std::min<int64_t>(32, std::max<int64_t>(0, value)); return CRT_OK; }
    if (!std::strcmp(name, "time_kernels")) {
        // value > 1 also creates the event pairs for that many launches now (event creation costs ~10 us apiece,
        // which would otherwise land in the region being timed)
        c->time_kernels = value != 0; c->last_trace_kernel_launches = 0;
        HIPCHK(c, hipSetDevice(c->device));
        while (value > 1 && c->kev.size() < 2 * (size_t)std::min<int64_t>(value, 1 << 20)) {
            Event e;
            HIPCHK(c, e.create());
            c->kev.push_back(std::move(e));
        }
        return CRT_OK;
    }
    return fail(c, CRT_EINVAL, "crt_set_option: unknown option '%s'", name);
}

}  // extern "C"
