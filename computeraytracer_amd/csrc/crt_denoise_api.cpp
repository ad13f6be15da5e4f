// crt_denoise_api.cpp -- the entry points of the preview filters (crt_denoise.hip): the tile's G-buffer, the four
// filters, the temporal history and its read-outs.
#include "crt_ctx.h"

using namespace crt;

namespace crt {

int dn_check_state(crt_ctx *c, const char *what, bool adaptive)   // adaptive: the counts are per tile, >= 1
{
    if (!c->have_scene || c->accel_mode < 0) return fail(c, CRT_ESTATE, "%s: scene + accel required", what);
    if (c->accel_stale) return fail(c, CRT_ESTATE, "%s: primitives were updated: call crt_refit_accel or crt_build_accel first", what);
    if (!adaptive && c->sample == 0) return fail(c, CRT_ESTATE, "%s: no sample traced yet", what);
    if (c->band != 0x40000000u)
        return fail(c, CRT_ESTATE, "%s: not under a row-band partition (neighbouring local rows are not neighbouring image rows)", what);
    if ((size_t)c->tw * c->th != 0 && !accum_ptr(c))
        return fail(c, CRT_ENOMEM, "%s: the tile's buffers are not allocated (an earlier crt_set_tile failed)", what);
    return CRT_OK;
}


// What the four entry points below do first: the checks, then the context's device and everything in flight finished.
// `values` must be positive and finite; `which` names them in the refusal.
static int dn_check_params(crt_ctx *c, const char *what, uint32_t iterations, const float *values, int count, const char *which)
{
    if (iterations > 10u) return fail(c, CRT_EINVAL, "%s: iterations %u > 10", what, iterations);
    for (int k = 0; k < count; k++)
        if (!(values[k] > 0.0f && values[k] <= 3.40282347e38f)) return fail(c, CRT_EINVAL, "%s: %s must be positive and finite", what, which);
    return CRT_OK;
}

int dn_begin(crt_ctx *c, const char *what, uint32_t iterations, const float *values, int count, const char *which, DnState state)
{
    if (!c) return CRT_EINVAL;
    CRT_TRY(dn_check_params(c, what, iterations, values, count, which));
    if (state == DN_TEMPORAL) state = c->as_on && c->adaptive_temporal ? DN_ADAPTIVE : DN_UNIFORM;
    if (state == DN_UNIFORM && c->as_on) return as_refuse(c, what);
    if (state == DN_ADAPTIVE && !c->as_on)
        return fail(c, CRT_ESTATE, "%s: the context is in the uniform state (crt_denoise filters a uniform render; "
                                   "crt_trace_adaptive with min_samples == max_samples gives this filter one)", what);
    if (state == DN_ADAPTIVE && c->as_broken) return as_refuse_broken(c, what);
    CRT_TRY(dn_check_state(c, what, state == DN_ADAPTIVE));
    return quiesce(c, false);
}

// ... and what they do last: the readbacks (plane: the filter's own float per pixel), the one synchronise, the dropped-path check.
int dn_finish(crt_ctx *c, size_t n, const float4 *res, float *rgb_out, uint8_t *rgba8_out, const float *plane, float *plane_out)
{
    if (n && rgb_out) HIPCHK(c, hipMemcpyAsync(rgb_out, res, n * sizeof(float4), hipMemcpyDeviceToHost, c->stream));
    if (n && rgba8_out) HIPCHK(c, hipMemcpyAsync(rgba8_out, c->dn.rgba.p, n * sizeof(uchar4), hipMemcpyDeviceToHost, c->stream));
    if (n && plane_out) HIPCHK(c, hipMemcpyAsync(plane_out, plane, n * sizeof(float), hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    return wf_check_dropped(c);
}

}  // namespace crt

extern "C" {

// The G-buffer of the tile, built once per scene / accel structure / tile.  Enqueued on the context's stream.  A rebuild
// goes into a set that no history slot names, the first such from the current one on (so in place if it can), but an
// allocated one before an unallocated one: nothing is allocated while a free set has buffers, and with three sets and
// two slots there always is a free one.  `dying` is a slot the caller is about to overwrite or let go: its set counts
// as free, and the slot is cleared once the allocations have succeeded, before its guides are overwritten.
// Its two halves: the set chosen and allocated (*set: -1 while the G-buffer is valid), then the launch on `stream`.
static int dn_gbuffer_alloc(crt_ctx *c, crt_ctx::DnSlot *dying, int *set_out)
{
    crt_ctx::Denoise &d = c->dn;
    *set_out = -1;
    if (d.valid) return CRT_OK;
    int set = -1;
    for (int k = 0; k < 3; k++) {
        const int s = (d.set + k) % 3;
        if ((&d.cur != dying && d.cur.guides == s) || (&d.prev != dying && d.prev.guides == s)) continue;
        if (set < 0 || (!d.sets[set].gbuf.p && d.sets[s].gbuf.p)) set = s;
    }
    const size_t n = (size_t)c->tw * c->th;
    CRT_ENSURE(c, c->dn.sets[set].gbuf, 2 * n);
    CRT_ENSURE(c, c->dn.sets[set].key, n);
    *set_out = set;
    return CRT_OK;
}

static int dn_gbuffer_build(crt_ctx *c, int set, hipStream_t stream)
{
    crt_ctx::Denoise &d = c->dn;
    if (set < 0) return CRT_OK;
    HIPCHK(c, dn_launch_gbuffer(c->sc, c->x0, c->y0, c->tw, c->th, d.sets[set].gbuf.p, d.sets[set].key.p, c->accel_mode == CRT_ACCEL_NONE, stream));
    d.set = set;
    d.valid = true;
    return CRT_OK;
}

static int dn_ensure_gbuffer(crt_ctx *c, crt_ctx::DnSlot *dying = nullptr)
{
    int set = -1;
    CRT_TRY(dn_gbuffer_alloc(c, dying, &set));
    if (set < 0) return CRT_OK;
    if (dying) dying->clear();
    return dn_gbuffer_build(c, set, c->stream);
}

// The colour buffers and the rgba8 of every filter, and what its launchers share (once the G-buffer is there).
static int dn_ensure_buffers(crt_ctx *c, size_t n)
{
    CRT_ENSURE(c, c->dn.c[0], n);
    CRT_ENSURE(c, c->dn.c[1], n);
    CRT_ENSURE(c, c->dn.rgba, n);
    return CRT_OK;
}

static DnFilter dn_filter(crt_ctx *c, uint32_t iterations, float sigma_normal, float sigma_plane, bool rgba)
{
    const crt_ctx::DnGuideSet &g = c->dn.sets[c->dn.set];
    return DnFilter{g.gbuf.p, g.key.p, {c->dn.c[0].p, c->dn.c[1].p}, rgba ? c->dn.rgba.p : nullptr, c->tw, c->th, iterations,
                    sigma_normal, sigma_plane, c->stream};
}

static const crt_denoise_params kDnDefaults = {5u, 1.0f, 0.5f, 0.3f};

int crt_denoise(crt_ctx *c, const crt_denoise_params *params, float *rgb_out, uint8_t *rgba8_out)
{
    const crt_denoise_params dp = params ? *params : kDnDefaults;
    const float sig[3] = {dp.sigma_color, dp.sigma_normal, dp.sigma_plane};
    CRT_TRY(dn_begin(c, "crt_denoise", dp.iterations, sig, 3, "every sigma", DN_UNIFORM));
    const size_t n = (size_t)c->tw * c->th;
    float4 *res = nullptr;
    if (n) {
        CRT_TRY(dn_ensure_gbuffer(c));
        CRT_TRY(dn_ensure_buffers(c, n));
        const DnFilter F = dn_filter(c, dp.iterations, dp.sigma_normal, dp.sigma_plane, rgba8_out != nullptr);
        HIPCHK(c, dn_launch_filter(F, accum_ptr(c), (float)c->sample, dp.sigma_color, &res));
    }
    return dn_finish(c, n, res, rgb_out, rgba8_out);
}

// What crt_denoise_latest puts on read_stream, behind the snapshot: the G-buffer if it is not there, the passes, the
// copies to the caller.  The caller synchronises read_stream whatever this returns.
static int dn_latest_passes(crt_ctx *c, const DnFilter &F, int set, float sigma_color, size_t n, float *rgb_out, uint8_t *rgba8_out)
{
    CRT_TRY(dn_gbuffer_build(c, set, F.stream));
    float4 *res = nullptr;
    HIPCHK(c, dn_launch_passes(F, sigma_color, c->dn.wave_blocks, &res));
    if (rgb_out) HIPCHK(c, hipMemcpyAsync(rgb_out, res, n * sizeof(float4), hipMemcpyDeviceToHost, F.stream));
    if (rgba8_out) HIPCHK(c, hipMemcpyAsync(rgba8_out, c->dn.rgba.p, n * sizeof(uchar4), hipMemcpyDeviceToHost, F.stream));
    return CRT_OK;
}

// crt_denoise of the newest complete frame, without a flush.  In stream order the accumulator holds the
// complete frame of sample resolved_upto (wf_resolve_batch sets it where it enqueues the resolve pass), so a snapshot
// enqueued on the context's stream now is that frame's average whatever the pool does meanwhile, and everything after the
// snapshot runs on read_stream: it waits for nothing the pipeline enqueues later, and the pipeline waits for that one pass of it.
int crt_denoise_latest(crt_ctx *c, const crt_denoise_params *params, float *rgb_out, uint8_t *rgba8_out, uint32_t *sample)
{
    if (!c) return CRT_EINVAL;
    const char *what = "crt_denoise_latest";
    const crt_denoise_params dp = params ? *params : kDnDefaults;
    const float sig[3] = {dp.sigma_color, dp.sigma_normal, dp.sigma_plane};
    CRT_TRY(dn_check_params(c, what, dp.iterations, sig, 3, "every sigma"));
    if (c->as_on) return as_refuse(c, what);
    CRT_TRY(dn_check_state(c, what, true));                      // (true: "no sample traced yet" is decided by s below)
    HIPCHK(c, hipSetDevice(c->device));
    CRT_TRY(wf_tick(c));
    const uint32_t s = c->resolved_upto;                         // after the tick: it may have enqueued a resolve pass
    if (s == 0) {
        if (sample) *sample = 0;
        return fail(c, CRT_ESTATE, "%s: no complete frame yet (%u samples requested): try again later", what, c->sample);
    }
    const size_t n = (size_t)c->tw * c->th;
    if (n) {
        // every allocation before the first launch: a failed one leaves nothing enqueued
        int set = -1;
        CRT_TRY(dn_gbuffer_alloc(c, nullptr, &set));
        CRT_TRY(dn_ensure_buffers(c, n));
        if (!c->read_stream) HIPCHK(c, c->read_stream.create(hipStreamNonBlocking));
        if (!c->dn.ev_snap) HIPCHK(c, c->dn.ev_snap.create(hipEventDisableTiming));
        DnFilter F = dn_filter(c, dp.iterations, dp.sigma_normal, dp.sigma_plane, rgba8_out != nullptr);
        const crt_ctx::DnGuideSet &g = c->dn.sets[set >= 0 ? set : c->dn.set];
        F.gbuf = g.gbuf.p; F.key = g.key.p;
        F.stream = c->read_stream;
        // the snapshot: behind the resolve pass of s, ahead of any resolve pass enqueued later
        HIPCHK(c, dn_launch_prepare(F, accum_ptr(c), (float)s, c->stream));
        HIPCHK(c, hipEventRecord(c->dn.ev_snap, c->stream));
        HIPCHK(c, hipStreamWaitEvent(c->read_stream, c->dn.ev_snap, 0));
        // read_stream is idle again before this call returns, also where a launch failed: c->dn's buffers and a G-buffer
        // marked valid are never in use on two streams (every other filter runs on the context's stream and ends idle)
        const int rc = dn_latest_passes(c, F, set, dp.sigma_color, n, rgb_out, rgba8_out);
        if (rc) { (void)hipStreamSynchronize(c->read_stream); return rc; }
        HIPCHK(c, hipStreamSynchronize(c->read_stream));
    }
    if (sample) *sample = s;
    return CRT_OK;
}

// The variance-guided filter of the adaptive state.  sigma_variance 8: the best of 1..24 at 16 and 32
// samples per pixel on the Cornell box and within 5 % of the best at 64.
static const crt_denoise_adaptive_params kDnAsDefaults = {5u, 8.0f, 0.5f, 0.3f};

int crt_denoise_adaptive_defaults(crt_denoise_adaptive_params *out)
{
    if (!out) return CRT_EINVAL;
    *out = kDnAsDefaults;
    return CRT_OK;
}

}  // extern "C"

namespace crt {

// The filter parameters of a call that takes them (NULL = the defaults), checked as crt_denoise_adaptive checks them.
int dn_adaptive_params(crt_ctx *c, const char *what, const crt_denoise_adaptive_params *params, crt_denoise_adaptive_params *out)
{
    *out = params ? *params : kDnAsDefaults;
    const float sig[3] = {out->sigma_variance, out->sigma_normal, out->sigma_plane};
    return dn_check_params(c, what, out->iterations, sig, 3, "every sigma");
}

// The adaptive filter of the context's tile on its stream, everything in flight already finished: what crt_denoise_adaptive
// and the selection of crt_trace_adaptive_filtered (crt_api.cpp) both run.  Every allocation comes before
// the first launch.  *res: the buffer that holds the colours; with `var`, *var_dev: the plane of v'.
int dn_adaptive_run(crt_ctx *c, const crt_denoise_adaptive_params &dp, bool rgba, bool var, float4 **res, const float **var_dev)
{
    const size_t n = (size_t)c->tw * c->th;
    *res = nullptr;
    if (var_dev) *var_dev = nullptr;
    if (!n) return CRT_OK;
    CRT_TRY(dn_ensure_buffers(c, n));
    CRT_ENSURE(c, c->dn.kv, n);
    CRT_ENSURE(c, c->dn.var, n);
    CRT_TRY(dn_ensure_gbuffer(c));
    const DnFilter F = dn_filter(c, dp.iterations, dp.sigma_normal, dp.sigma_plane, rgba);
    HIPCHK(c, dn_launch_filter_adaptive(F, accum_ptr(c), c->as_q.p, c->as_counts.p, c->dn.kv.p, var ? c->dn.var.p : nullptr,
                                        dp.sigma_variance, res));
    if (var_dev) *var_dev = c->dn.var.p;
    return CRT_OK;
}

}  // namespace crt

extern "C" {

int crt_denoise_adaptive(crt_ctx *c, const crt_denoise_adaptive_params *params, float *rgb_out, uint8_t *rgba8_out, float *var_out)
{
    if (!c) return CRT_EINVAL;
    crt_denoise_adaptive_params dp;
    CRT_TRY(dn_adaptive_params(c, "crt_denoise_adaptive", params, &dp));
    CRT_TRY(dn_begin(c, "crt_denoise_adaptive", 0, nullptr, 0, "", DN_ADAPTIVE));
    float4 *res = nullptr;
    CRT_TRY(dn_adaptive_run(c, dp, rgba8_out != nullptr, var_out != nullptr, &res, nullptr));
    return dn_finish(c, (size_t)c->tw * c->th, res, rgb_out, rgba8_out, c->dn.var.p, var_out);
}

// ---------------------------------------------------------------- temporal reuse
int crt_set_sample_offset(crt_ctx *c, uint32_t offset)
{
    if (!c) return CRT_EINVAL;
    if (c->as_on) return as_refuse(c, "crt_set_sample_offset");
    if (c->sample != 0)
        return fail(c, CRT_ESTATE, "crt_set_sample_offset: the context holds %u samples: the offset is set at sample 0 (crt_reset first)", c->sample);
    c->sample_offset = offset;
    return CRT_OK;
}

int crt_sample_offset(crt_ctx *c, uint32_t *out)
{
    if (!c || !out) return CRT_EINVAL;
    *out = c->sample_offset;
    return CRT_OK;
}

// max_history 64, normal_tol 0.5, plane_tol 2: DESIGN.md 6e has the sweep they were chosen by.
static const crt_denoise_temporal_params kDnTpDefaults = {5u, 1.0f, 0.5f, 0.3f, 64.0f, 0.5f, 2.0f};

int crt_denoise_temporal_defaults(crt_denoise_temporal_params *out)
{
    if (!out) return CRT_EINVAL;
    *out = kDnTpDefaults;
    return CRT_OK;
}

int crt_denoise_temporal_reset(crt_ctx *c)
{
    if (!c) return CRT_EINVAL;
    c->dn.drop();
    return CRT_OK;
}

// kappa of a camera frame: the pixel's footprint per unit distance, (|hor| / W) / |llc + hor/2 + ver/2 - eye|, in double.
static double th_kappa(const float cam[12], uint32_t W)
{
    double hor = 0.0, ax = 0.0;
    for (int k = 0; k < 3; k++) {
        hor += (double)cam[3 + k] * cam[3 + k];
        const double a = (double)cam[k] + 0.5 * cam[3 + k] + 0.5 * cam[6 + k] - cam[9 + k];
        ax += a * a;
    }
    return (std::sqrt(hor) / (double)W) / std::sqrt(ax);
}

// What the blend and crt_read_motion share: the frame's guides, the PREVIOUS slot with its own and its camera, and the
// records the map of 6f reads.  h_prev stays null without a usable PREVIOUS.
static DnReprojParams th_reproj_params(crt_ctx *c, const crt_ctx::DnGuideSet &guides)
{
    const crt_ctx::DnSlot &prev = c->dn.prev;
    DnReprojParams P{};
    P.gbuf = guides.gbuf.p; P.key = guides.key.p;
    P.tw = c->tw; P.th = c->th;
    if (prev.valid) {
        // M' = [hor' ver' (llc' - eye')]^-1 by cofactors, in double
        const float *q = prev.cam;
        double A[3][3], inv[3][3];
        for (int k = 0; k < 3; k++) { A[k][0] = q[3 + k]; A[k][1] = q[6 + k]; A[k][2] = (double)q[k] - (double)q[9 + k]; }
        const double det = A[0][0] * (A[1][1] * A[2][2] - A[1][2] * A[2][1]) - A[0][1] * (A[1][0] * A[2][2] - A[1][2] * A[2][0]) +
                           A[0][2] * (A[1][0] * A[2][1] - A[1][1] * A[2][0]);
        for (int i = 0; i < 3; i++)
            for (int j = 0; j < 3; j++) {
                const int r0 = (j + 1) % 3, r1 = (j + 2) % 3, c0 = (i + 1) % 3, c1 = (i + 2) % 3;
                inv[i][j] = (A[r0][c0] * A[r1][c1] - A[r0][c1] * A[r1][c0]) / det;
            }
        bool ok = std::isfinite(det) && det != 0.0;
        for (int i = 0; i < 3; i++) for (int j = 0; j < 3; j++) { P.m[3 * i + j] = inv[i][j]; ok = ok && std::isfinite(inv[i][j]); }
        if (ok) {                                                // (a degenerate previous camera: nothing is reused)
            P.h_prev = prev.c.p; P.gbuf_prev = c->dn.sets[prev.guides].gbuf.p; P.key_prev = c->dn.sets[prev.guides].key.p;
        }
        for (int k = 0; k < 3; k++) { P.eye_prev[k] = q[9 + k]; P.eye[k] = c->sc.cam[9 + k]; }
        P.kappa_prev = (float)th_kappa(q, c->W); P.kappa = (float)th_kappa(c->sc.cam, c->W);
        if (prev.snap) {                                         // PREVIOUS saw another pose of the scene: k_dn_reproject<true>
            P.raw = c->d_raw.p; P.raw_prev = c->dn.snap.p; P.nprim = (uint32_t)c->prims.size();
        }
    }
    P.W = (double)c->W; P.H = (double)c->H; P.x0 = (double)c->x0; P.y0 = (double)c->y0;
    return P;
}

// What crt_denoise_temporal and crt_denoise_svgf share once dn_begin has passed: the buffers, the promotion of CURRENT, the
// G-buffer, the blend and the passes after it.  svgf: also the moments and the variance-guided passes.
struct ThCall {
    uint32_t iterations;
    float sigma_normal, sigma_plane, max_history, normal_tol, plane_tol;
    bool svgf;
    float sigma_color;                  // !svgf
    float sigma_variance, min_frames;   // svgf
    float spatial_b;                    // svgf: 0, or the factor of option "svgf_spatial_pct" 
    float gamma;                        // 0, or the factor of option "temporal_clip_pct" 
};

static int th_blend_and_filter(crt_ctx *c, const ThCall &t, bool rgba, bool hist, bool var, float4 **res)
{
    const size_t n = (size_t)c->tw * c->th;
    crt_ctx::DnSlot &cur = c->dn.cur, &prev = c->dn.prev;
    const bool promote = cur.valid && cur.frame != c->frame_id;  // the first call of a new frame
    // Every buffer first: a failed allocation leaves the slots as they were.  dn_ensure_gbuffer comes last because it also
    // clears a slot and moves dn.set once its own two allocations are through: no allocation may follow it.
    CRT_ENSURE(c, c->dn.cur.c, n);
    CRT_ENSURE(c, c->dn.prev.c, n);
    CRT_TRY(dn_ensure_buffers(c, n));
    CRT_ENSURE(c, c->dn.hist, n);
    if (t.svgf) {
        CRT_ENSURE(c, c->dn.cur.m, n);
        CRT_ENSURE(c, c->dn.prev.m, n);
        CRT_ENSURE(c, c->dn.kv, n);
        CRT_ENSURE(c, c->dn.var, n);
    }
    if (t.gamma != 0.0f) CRT_ENSURE(c, c->dn.box, 2 * n);
    CRT_TRY(dn_ensure_gbuffer(c, promote ? &prev : &cur));
    // CURRENT becomes PREVIOUS, with its guides and its snapshot flag; the slot that was PREVIOUS ends here, as CURRENT
    // does when this frame is filtered again
    if (promote) std::swap(prev, cur);
    cur.clear();
    DnSvgfParams P{};
    static_cast<DnReprojParams &>(P) = th_reproj_params(c, c->dn.sets[c->dn.set]);
    P.accum = accum_ptr(c);
    P.h_cur = cur.c.p;
    P.hist = hist ? c->dn.hist.p : nullptr;
    P.n = (float)c->sample;
    const uint32_t *counts = c->as_on ? c->as_counts.p : nullptr;    // (dn_begin let the adaptive state in: every tile has its own n)
    P.max_history = t.max_history;
    P.normal_tol2 = (float)std::min(3.0e38, (double)t.normal_tol * t.normal_tol);
    P.plane_tol = t.plane_tol;
    const DnFilter F = dn_filter(c, t.iterations, t.sigma_normal, t.sigma_plane, rgba);
    float4 *box = t.gamma != 0.0f ? c->dn.box.p : nullptr;
    c->dn.box_ran = false;
    if (t.svgf) {
        P.m_prev = P.h_prev && prev.has_m ? prev.m.p : nullptr;
        P.m_cur = cur.m.p;
        P.min_frames = t.min_frames;
        HIPCHK(c, dn_launch_svgf(F, P, counts, c->dn.kv.p, var ? c->dn.var.p : nullptr, t.sigma_variance, t.spatial_b, box, t.gamma, res));
    } else {
        HIPCHK(c, dn_launch_temporal(F, P, counts, t.sigma_color, box, t.gamma, res));
    }
    c->dn.box_ran = box && P.h_prev;                             // (what the launchers ask before the box pass)
    std::memcpy(cur.cam, c->sc.cam, sizeof cur.cam);
    cur.guides = c->dn.set; cur.frame = c->frame_id;
    cur.valid = true; cur.has_m = t.svgf;
    return CRT_OK;
}

int crt_denoise_temporal(crt_ctx *c, const crt_denoise_temporal_params *params, float *rgb_out, uint8_t *rgba8_out, float *history_out)
{
    const crt_denoise_temporal_params dp = params ? *params : kDnTpDefaults;
    const float pos[6] = {dp.sigma_color, dp.sigma_normal, dp.sigma_plane, dp.max_history, dp.normal_tol, dp.plane_tol};
    CRT_TRY(dn_begin(c, "crt_denoise_temporal", dp.iterations, pos, 6, "every sigma, tolerance and max_history", DN_TEMPORAL));
    const size_t n = (size_t)c->tw * c->th;
    float4 *res = nullptr;
    std::vector<float> hw;                                       // (rgb_out's channel 3 is Hw: the filter passes leave it 0)
    if (rgb_out && dp.iterations > 0 && !history_out) hw.resize(n);
    float *hw_host = history_out ? history_out : hw.empty() ? nullptr : hw.data();
    if (n) {
        const ThCall t{dp.iterations, dp.sigma_normal, dp.sigma_plane, dp.max_history, dp.normal_tol, dp.plane_tol, false,
                       dp.sigma_color, 0.0f, 0.0f, 0.0f, (float)c->dn.clip_pct / 100.0f};
        CRT_TRY(th_blend_and_filter(c, t, rgba8_out != nullptr, history_out || rgb_out, false, &res));
    }
    const int rc = dn_finish(c, n, res, rgb_out, rgba8_out, c->dn.hist.p, hw_host);
    if (rgb_out && dp.iterations > 0)
        for (size_t i = 0; i < n; i++) rgb_out[4 * i + 3] = hw_host[i];
    return rc;
}

// sigma_variance 4, min_frames 4: DESIGN.md 6g has the sweep they were chosen by.
static const crt_denoise_svgf_params kDnSvgfDefaults = {5u, 4.0f, 0.5f, 0.3f, 64.0f, 0.5f, 2.0f, 4.0f};

int crt_denoise_svgf_defaults(crt_denoise_svgf_params *out)
{
    if (!out) return CRT_EINVAL;
    *out = kDnSvgfDefaults;
    return CRT_OK;
}

int crt_denoise_svgf(crt_ctx *c, const crt_denoise_svgf_params *params, float *rgb_out, uint8_t *rgba8_out, float *history_out,
                     float *var_out)
{
    const crt_denoise_svgf_params dp = params ? *params : kDnSvgfDefaults;
    const float pos[6] = {dp.sigma_variance, dp.sigma_normal, dp.sigma_plane, dp.max_history, dp.normal_tol, dp.plane_tol};
    if (c && !(dp.min_frames >= 2.0f && dp.min_frames <= 3.40282347e38f))
        return fail(c, CRT_EINVAL, "crt_denoise_svgf: min_frames must be >= 2 and finite");
    CRT_TRY(dn_begin(c, "crt_denoise_svgf", dp.iterations, pos, 6, "every sigma, tolerance and max_history", DN_TEMPORAL));
    const size_t n = (size_t)c->tw * c->th;
    float4 *res = nullptr;
    if (n) {
        const ThCall t{dp.iterations, dp.sigma_normal, dp.sigma_plane, dp.max_history, dp.normal_tol, dp.plane_tol, true,
                       0.0f, dp.sigma_variance, dp.min_frames, (float)c->svgf_spatial_pct / 100.0f,
                       (float)c->dn.clip_pct / 100.0f};
        CRT_TRY(th_blend_and_filter(c, t, rgba8_out != nullptr, history_out != nullptr, var_out != nullptr, &res));
        if (var_out) HIPCHK(c, hipMemcpyAsync(var_out, c->dn.var.p, n * sizeof(float), hipMemcpyDeviceToHost, c->stream));
    }
    return dn_finish(c, n, res, rgb_out, rgba8_out, c->dn.hist.p, history_out);
}

int crt_read_motion(crt_ctx *c, float *out)
{
    if (!c || !out) return CRT_EINVAL;
    CRT_TRY(dn_begin(c, "crt_read_motion", 0, nullptr, 0, "", DN_TEMPORAL));
    if (!c->dn.cur.valid || c->dn.cur.frame != c->frame_id)
        return fail(c, CRT_ESTATE, "crt_read_motion: no crt_denoise_temporal in this frame yet (it reports where that call's blend looked)");
    const size_t n = (size_t)c->tw * c->th;
    if (n) {
        CRT_ENSURE(c, c->dn.uv, n);
        const DnReprojParams P = th_reproj_params(c, c->dn.sets[c->dn.cur.guides]);      // CURRENT's own guides
        HIPCHK(c, dn_launch_motion(P, c->dn.uv.p, c->stream));
        HIPCHK(c, hipMemcpyAsync(out, c->dn.uv.p, n * sizeof(float2), hipMemcpyDeviceToHost, c->stream));
    }
    return dn_finish(c, n, nullptr, nullptr, nullptr);
}

int crt_read_gbuffer(crt_ctx *c, float *out)
{
    if (!c || !out) return CRT_EINVAL;
    CRT_TRY(dn_begin(c, "crt_read_gbuffer", 0, nullptr, 0, "", DN_EITHER));
    const size_t n = (size_t)c->tw * c->th;
    if (n) {
        CRT_TRY(dn_ensure_gbuffer(c));
        HIPCHK(c, hipMemcpyAsync(out, c->dn.sets[c->dn.set].gbuf.p, n * 2 * sizeof(float4), hipMemcpyDeviceToHost, c->stream));
    }
    return dn_finish(c, n, nullptr, nullptr, nullptr);
}

// ---------------------------------------------------------------- the frame of a partition
// crt_comm.cpp: the assembled planes of the latest CRT_GATHER_PREVIEW (accumulator, Q, tile counts) and W, H, n -- or the refusal.
int crt_internal_comm_frame_view(crt_ctx *c, const char *who, int adaptive, int assemble_now, const void *planes[3], uint32_t dims[3]);

namespace {

struct FrameView {
    const float4 *accum = nullptr;
    const float *q = nullptr;
    const uint32_t *counts = nullptr;
    uint32_t W = 0, H = 0, n = 0;
};

// How the three frame-level calls open: every refusal that needs no allocation, with nothing enqueued; then a sync point.
int fr_begin(crt_ctx *c, const char *what, bool adaptive, FrameView &v)
{
    if (!c->have_scene || c->accel_mode < 0) return fail(c, CRT_ESTATE, "%s: scene + accel required", what);
    if (c->accel_stale) return fail(c, CRT_ESTATE, "%s: primitives were updated: call crt_refit_accel or crt_build_accel first", what);
    const void *planes[3] = {nullptr, nullptr, nullptr};
    uint32_t dims[3] = {0, 0, 0};
    CRT_TRY(crt_internal_comm_frame_view(c, what, adaptive ? 1 : 0, 0, planes, dims));
    v.accum = (const float4 *)planes[0]; v.q = (const float *)planes[1]; v.counts = (const uint32_t *)planes[2];
    v.W = dims[0]; v.H = dims[1]; v.n = dims[2];
    return quiesce(c, false);
}

// ... and how they go on once their buffers exist: the planes in image order, on the context's stream.
int fr_assemble(crt_ctx *c, const char *what, bool adaptive)
{
    const void *planes[3];
    uint32_t dims[3];
    return crt_internal_comm_frame_view(c, what, adaptive ? 1 : 0, 1, planes, dims);
}

// The filters' buffers (kv: the adaptive filter's) and the frame's G-buffer: one camera ray per pixel of the whole image
// against this rank's replica of the scene.  Allocations first; a failed one leaves complete buffers or none.
int fr_ensure(crt_ctx *c, const char *what, bool adaptive, const FrameView &v)
{
    crt_ctx::FrameDenoise &f = c->fdn;
    const size_t n = (size_t)v.W * v.H;
    if (f.guides.gbuf.n < 2 * n || f.guides.key.n < n) f.valid = false;
    CRT_ENSURE(c, f.guides.gbuf, 2 * n);
    CRT_ENSURE(c, f.guides.key, n);
    CRT_ENSURE(c, f.c[0], n);
    CRT_ENSURE(c, f.c[1], n);
    CRT_ENSURE(c, f.rgba, n);
    if (adaptive) {
        CRT_ENSURE(c, f.kv, n);
        CRT_ENSURE(c, f.var, n);
    }
    CRT_TRY(fr_assemble(c, what, adaptive));
    if (!f.valid) {
        HIPCHK(c, dn_launch_gbuffer(c->sc, 0, 0, v.W, v.H, f.guides.gbuf.p, f.guides.key.p, c->accel_mode == CRT_ACCEL_NONE, c->stream));
        f.valid = true;
    }
    return CRT_OK;
}

DnFilter fr_filter(crt_ctx *c, const FrameView &v, uint32_t iterations, float sigma_normal, float sigma_plane, bool rgba)
{
    crt_ctx::FrameDenoise &f = c->fdn;
    return DnFilter{f.guides.gbuf.p, f.guides.key.p, {f.c[0].p, f.c[1].p}, rgba ? f.rgba.p : nullptr, v.W, v.H, iterations,
                    sigma_normal, sigma_plane, c->stream};
}

int fr_finish(crt_ctx *c, size_t n, const float4 *res, float *rgb_out, uint8_t *rgba8_out, float *var_out)
{
    if (n && rgb_out) HIPCHK(c, hipMemcpyAsync(rgb_out, res, n * sizeof(float4), hipMemcpyDeviceToHost, c->stream));
    if (n && rgba8_out) HIPCHK(c, hipMemcpyAsync(rgba8_out, c->fdn.rgba.p, n * sizeof(uchar4), hipMemcpyDeviceToHost, c->stream));
    if (n && var_out) HIPCHK(c, hipMemcpyAsync(var_out, c->fdn.var.p, n * sizeof(float), hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    return wf_check_dropped(c);
}

}  // namespace

int crt_denoise_frame(crt_ctx *c, const crt_denoise_params *params, float *rgb_out, uint8_t *rgba8_out)
{
    if (!c) return CRT_EINVAL;
    const crt_denoise_params dp = params ? *params : kDnDefaults;
    const float sig[3] = {dp.sigma_color, dp.sigma_normal, dp.sigma_plane};
    CRT_TRY(dn_check_params(c, "crt_denoise_frame", dp.iterations, sig, 3, "every sigma"));
    FrameView v;
    CRT_TRY(fr_begin(c, "crt_denoise_frame", false, v));
    if (v.n == 0) return fail(c, CRT_ESTATE, "crt_denoise_frame: no sample traced at the PREVIEW gather");
    const size_t n = (size_t)v.W * v.H;
    float4 *res = nullptr;
    if (n) {
        CRT_TRY(fr_ensure(c, "crt_denoise_frame", false, v));
        const DnFilter F = fr_filter(c, v, dp.iterations, dp.sigma_normal, dp.sigma_plane, rgba8_out != nullptr);
        HIPCHK(c, dn_launch_filter(F, v.accum, (float)v.n, dp.sigma_color, &res));
    }
    return fr_finish(c, n, res, rgb_out, rgba8_out, nullptr);
}

int crt_denoise_adaptive_frame(crt_ctx *c, const crt_denoise_adaptive_params *params, float *rgb_out, uint8_t *rgba8_out, float *var_out)
{
    if (!c) return CRT_EINVAL;
    const crt_denoise_adaptive_params dp = params ? *params : kDnAsDefaults;
    const float sig[3] = {dp.sigma_variance, dp.sigma_normal, dp.sigma_plane};
    CRT_TRY(dn_check_params(c, "crt_denoise_adaptive_frame", dp.iterations, sig, 3, "every sigma"));
    FrameView v;
    CRT_TRY(fr_begin(c, "crt_denoise_adaptive_frame", true, v));
    const size_t n = (size_t)v.W * v.H;
    float4 *res = nullptr;
    if (n) {
        CRT_TRY(fr_ensure(c, "crt_denoise_adaptive_frame", true, v));
        const DnFilter F = fr_filter(c, v, dp.iterations, dp.sigma_normal, dp.sigma_plane, rgba8_out != nullptr);
        HIPCHK(c, dn_launch_filter_adaptive(F, v.accum, v.q, v.counts, c->fdn.kv.p, var_out ? c->fdn.var.p : nullptr, dp.sigma_variance, &res));
    }
    return fr_finish(c, n, res, rgb_out, rgba8_out, var_out);
}

int crt_read_frame_adaptive(crt_ctx *c, uint32_t *counts, float *errors)
{
    if (!c) return CRT_EINVAL;
    FrameView v;
    CRT_TRY(fr_begin(c, "crt_read_frame_adaptive", true, v));
    const uint32_t tiles_x = (v.W + 7) / 8, tiles_y = (v.H + 7) / 8;
    const size_t ntiles = (size_t)tiles_x * tiles_y;
    if (ntiles) {
        CRT_ENSURE(c, c->fdn.errors, ntiles);
        CRT_ENSURE(c, c->fdn.flags, ntiles);
        CRT_TRY(fr_assemble(c, "crt_read_frame_adaptive", true));
        // E is a function of the frame's accumulator, Q and counts alone: crt_read_adaptive's kernel over the assembled frame
        AsParams A{};
        A.accum = v.accum; A.q = v.q; A.counts = v.counts; A.errors = c->fdn.errors.p; A.flags = c->fdn.flags.p;
        A.tw = v.W; A.th = v.H; A.tiles_x = tiles_x; A.tiles_y = tiles_y;
        A.min_samples = 0u; A.max_samples = 0u; A.threshold = 0.0f;
        HIPCHK(c, as_launch_select(A, false, c->stream));
        if (counts) HIPCHK(c, hipMemcpyAsync(counts, v.counts, ntiles * sizeof(uint32_t), hipMemcpyDeviceToHost, c->stream));
        if (errors) HIPCHK(c, hipMemcpyAsync(errors, c->fdn.errors.p, ntiles * sizeof(float), hipMemcpyDeviceToHost, c->stream));
    }
    HIPCHK(c, hipStreamSynchronize(c->stream));
    return wf_check_dropped(c);
}

}  // extern "C"
