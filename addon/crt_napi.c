/*
 * crt_napi.c -- thin N-API addon: 1:1 JavaScript wrappers over the C ABI of
 * include/crt.h (libcrt.so, hand-written HIP for gfx950).
 *
 * It stands where the reference's src/main.js talks to WebGPU:
 *   navigator.gpu.requestAdapter/requestDevice (main.js:8-9)        -> create()
 *   createBuffer + getMappedRange + unmap for b4..b8 (main.js:147-393) -> uploadScene()
 *   dispatchWorkgroups(1); dispatchWorkgroups(W/8,H/8) (main.js:598-611) -> trace(n)
 *   "uncapturederror" (main.js:11-14)                               -> thrown Error
 * Build: plain gcc against /usr/include/node (no node-gyp), see addon/Makefile.
 */
#include <node_api.h>
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "../include/crt.h"

#define NAPI_OK(env, call)                                                          \
    do {                                                                            \
        if ((call) != napi_ok) {                                                    \
            napi_throw_error((env), NULL, "N-API call failed: " #call);             \
            return NULL;                                                            \
        }                                                                           \
    } while (0)

static napi_value throw_crt(napi_env env, crt_ctx *ctx, int code, const char *what)
{
    char msg[640];
    const char *detail = crt_last_error(ctx);
    snprintf(msg, sizeof msg, "%s failed (%d): %s", what, code, detail ? detail : "");
    napi_throw_error(env, "ERR_CRT", msg);
    return NULL;
}

#define CRT_CHECK(env, ctx, what, call)                                  \
    do {                                                                 \
        int rc_ = (call);                                                \
        if (rc_ != CRT_OK) return throw_crt((env), (ctx), rc_, (what));  \
    } while (0)

/* What a handle holds: the context and the queue of asynchronous jobs on it.  The C ABI allows one thread per
 * context at a time, so the *Async entry points run their jobs one after the other (napi_async_work on the libuv
 * pool, the next one queued when the previous completes) and the synchronous entry points refuse to run while
 * jobs are pending ("await the promises first"). */
struct job;
typedef struct slot {
    crt_ctx *ctx;
    struct job *head, *tail;     /* pending jobs, head = the one running */
    napi_ref self;               /* strong reference to the handle while jobs are pending: a promise does not keep the
                                    external alive, and `traceAsync(create(0), n)` must not be collected mid-job */
} slot;

static void finalize_ctx(napi_env env, void *data, void *hint)
{
    (void)env; (void)hint;
    slot *s = (slot *)data;
    if (s) {
        /* (unreachable with jobs pending: `self` holds the handle until the queue is empty) */
        if (s->ctx) crt_destroy(s->ctx);
        free(s);
    }
}

static slot *get_slot(napi_env env, napi_value v)
{
    void *p = NULL;
    if (napi_get_value_external(env, v, &p) != napi_ok || !p || !((slot *)p)->ctx) {
        napi_throw_type_error(env, NULL, "invalid or destroyed crt context handle");
        return NULL;
    }
    return (slot *)p;
}

/* args[0] is always the handle (an external holding a slot); synchronous calls need an idle context */
static crt_ctx *get_ctx(napi_env env, napi_value v)
{
    slot *s = get_slot(env, v);
    if (!s) return NULL;
    if (s->head) {
        napi_throw_error(env, "ERR_CRT_BUSY", "asynchronous calls are pending on this context: await their promises first");
        return NULL;
    }
    return s->ctx;
}

/* Bytes of an ArrayBuffer / TypedArray / DataView / Buffer argument. */
static int get_bytes(napi_env env, napi_value v, void **data, size_t *len)
{
    bool is;
    if (napi_is_arraybuffer(env, v, &is) == napi_ok && is)
        return napi_get_arraybuffer_info(env, v, data, len) == napi_ok;
    if (napi_is_typedarray(env, v, &is) == napi_ok && is) {
        napi_typedarray_type t; size_t n, off; napi_value ab;
        if (napi_get_typedarray_info(env, v, &t, &n, data, &ab, &off) != napi_ok) return 0;
        static const size_t esz[] = {1, 1, 1, 2, 2, 4, 4, 4, 8, 8, 8};
        if ((size_t)t >= sizeof esz / sizeof esz[0]) return 0;      /* (an element type this table does not know) */
        *len = n * esz[t];
        return 1;
    }
    if (napi_is_dataview(env, v, &is) == napi_ok && is) {
        napi_value ab; size_t off;
        return napi_get_dataview_info(env, v, len, data, &ab, &off) == napi_ok;
    }
    if (napi_is_buffer(env, v, &is) == napi_ok && is)
        return napi_get_buffer_info(env, v, data, len) == napi_ok;
    return 0;
}

#define ARGS(n)                                                       \
    size_t argc = (n);                                                \
    napi_value argv[(n) > 0 ? (n) : 1];                               \
    NAPI_OK(env, napi_get_cb_info(env, info, &argc, argv, NULL, NULL)); \
    if (argc < (size_t)(n)) { napi_throw_type_error(env, NULL, "too few arguments"); return NULL; }

static napi_value undefined(napi_env env)
{
    napi_value u;
    napi_get_undefined(env, &u);
    return u;
}

static napi_value js_create(napi_env env, napi_callback_info info)
{
    ARGS(1)
    int32_t dev = 0;
    NAPI_OK(env, napi_get_value_int32(env, argv[0], &dev));
    crt_ctx *ctx = NULL;
    int rc = crt_create(&ctx, dev);
    if (rc != CRT_OK) return throw_crt(env, NULL, rc, "crt_create");
    slot *sl = (slot *)calloc(1, sizeof *sl);
    sl->ctx = ctx;
    napi_value ext;
    NAPI_OK(env, napi_create_external(env, sl, finalize_ctx, NULL, &ext));
    return ext;
}

static napi_value js_destroy(napi_env env, napi_callback_info info)
{
    ARGS(1)
    void *p = NULL;
    if (napi_get_value_external(env, argv[0], &p) == napi_ok && p && ((slot *)p)->ctx) {
        if (((slot *)p)->head) {
            napi_throw_error(env, "ERR_CRT_BUSY", "destroy: asynchronous calls are pending on this context");
            return NULL;
        }
        crt_destroy(((slot *)p)->ctx);
        ((slot *)p)->ctx = NULL;
    }
    return undefined(env);
}

/* uploadScene(h, primitives, lights, spectra, cie, camera) -- byte buffers exactly as
 * main.js builds them (80-byte records; Float32Array tables). */
static napi_value js_upload_scene(napi_env env, napi_callback_info info)
{
    ARGS(6)
    crt_ctx *ctx = get_ctx(env, argv[0]);
    if (!ctx) return NULL;
    void *p[5]; size_t n[5];
    static const char *names[5] = {"primitives", "lights", "spectra", "cie", "camera"};
    for (int i = 0; i < 5; i++) {
        if (!get_bytes(env, argv[i + 1], &p[i], &n[i])) {
            char m[96];
            snprintf(m, sizeof m, "uploadScene: %s must be an ArrayBuffer or typed array", names[i]);
            napi_throw_type_error(env, NULL, m);
            return NULL;
        }
    }
    if (n[0] % 80 || n[1] % 80 || n[2] % (301 * 4) || n[3] != 3 * 471 * 4 || n[4] != 64) {
        napi_throw_range_error(env, NULL, "uploadScene: sizes must be primitives/lights k*80 B, spectra k*1204 B, "
                                          "cie 5652 B, camera 64 B");
        return NULL;
    }
    CRT_CHECK(env, ctx, "crt_upload_scene",
              crt_upload_scene(ctx, p[0], n[0] / 80, p[1], n[1] / 80, (const float *)p[2], n[2] / (301 * 4),
                               (const float *)p[3], (const float *)p[4]));
    return undefined(env);
}

static napi_value js_set_tile(napi_env env, napi_callback_info info)
{
    ARGS(5)
    crt_ctx *ctx = get_ctx(env, argv[0]);
    if (!ctx) return NULL;
    uint32_t v[4];
    for (int i = 0; i < 4; i++) NAPI_OK(env, napi_get_value_uint32(env, argv[i + 1], &v[i]));
    CRT_CHECK(env, ctx, "crt_set_tile", crt_set_tile(ctx, v[0], v[1], v[2], v[3]));
    return undefined(env);
}

static napi_value js_build_accel(napi_env env, napi_callback_info info)
{
    ARGS(2)
    crt_ctx *ctx = get_ctx(env, argv[0]);
    if (!ctx) return NULL;
    int32_t mode;
    NAPI_OK(env, napi_get_value_int32(env, argv[1], &mode));
    CRT_CHECK(env, ctx, "crt_build_accel", crt_build_accel(ctx, mode));
    return undefined(env);
}

static napi_value js_reset(napi_env env, napi_callback_info info)
{
    ARGS(1)
    crt_ctx *ctx = get_ctx(env, argv[0]);
    if (!ctx) return NULL;
    CRT_CHECK(env, ctx, "crt_reset", crt_reset(ctx));
    return undefined(env);
}

static napi_value js_trace(napi_env env, napi_callback_info info)
{
    ARGS(2)
    crt_ctx *ctx = get_ctx(env, argv[0]);
    if (!ctx) return NULL;
    uint32_t n;
    NAPI_OK(env, napi_get_value_uint32(env, argv[1], &n));
    CRT_CHECK(env, ctx, "crt_trace", crt_trace(ctx, n));
    return undefined(env);
}

static napi_value js_sync(napi_env env, napi_callback_info info)
{
    ARGS(1)
    crt_ctx *ctx = get_ctx(env, argv[0]);
    if (!ctx) return NULL;
    CRT_CHECK(env, ctx, "crt_sync", crt_sync(ctx));
    return undefined(env);
}

static napi_value js_sample_count(napi_env env, napi_callback_info info)
{
    ARGS(1)
    crt_ctx *ctx = get_ctx(env, argv[0]);
    if (!ctx) return NULL;
    uint32_t s = 0;
    CRT_CHECK(env, ctx, "crt_sample_count", crt_sample_count(ctx, &s));
    napi_value out;
    NAPI_OK(env, napi_create_uint32(env, s, &out));
    return out;
}

static napi_value js_tile(napi_env env, napi_callback_info info)
{
    ARGS(1)
    crt_ctx *ctx = get_ctx(env, argv[0]);
    if (!ctx) return NULL;
    uint32_t t[4];
    CRT_CHECK(env, ctx, "crt_tile", crt_tile(ctx, t));
    napi_value arr;
    NAPI_OK(env, napi_create_array_with_length(env, 4, &arr));
    for (uint32_t i = 0; i < 4; i++) {
        napi_value v;
        NAPI_OK(env, napi_create_uint32(env, t[i], &v));
        NAPI_OK(env, napi_set_element(env, arr, i, v));
    }
    return arr;
}

static napi_value read_image(napi_env env, napi_callback_info info, int rgba)
{
    ARGS(1)
    crt_ctx *ctx = get_ctx(env, argv[0]);
    if (!ctx) return NULL;
    uint32_t t[4];
    CRT_CHECK(env, ctx, "crt_tile", crt_tile(ctx, t));
    size_t px = (size_t)t[2] * t[3];
    size_t bytes = px * (rgba ? 4 : 16);
    void *data = NULL;
    napi_value ab, ta;
    NAPI_OK(env, napi_create_arraybuffer(env, bytes, &data, &ab));
    if (rgba) CRT_CHECK(env, ctx, "crt_read_rgba8", crt_read_rgba8(ctx, (uint8_t *)data));
    else CRT_CHECK(env, ctx, "crt_read_accum", crt_read_accum(ctx, (float *)data));
    NAPI_OK(env, napi_create_typedarray(env, rgba ? napi_uint8_array : napi_float32_array, px * 4, ab, 0, &ta));
    return ta;
}
static napi_value js_read_accum(napi_env env, napi_callback_info info) { return read_image(env, info, 0); }
static napi_value js_read_rgba8(napi_env env, napi_callback_info info) { return read_image(env, info, 1); }

static napi_value js_write_accum(napi_env env, napi_callback_info info)
{
    ARGS(3)
    crt_ctx *ctx = get_ctx(env, argv[0]);
    if (!ctx) return NULL;
    void *p; size_t n;
    uint32_t s, t[4];
    if (!get_bytes(env, argv[1], &p, &n)) { napi_throw_type_error(env, NULL, "writeAccum: typed array expected"); return NULL; }
    NAPI_OK(env, napi_get_value_uint32(env, argv[2], &s));
    CRT_CHECK(env, ctx, "crt_tile", crt_tile(ctx, t));
    if (n != (size_t)t[2] * t[3] * 16) { napi_throw_range_error(env, NULL, "writeAccum: need tw*th*4 floats"); return NULL; }
    CRT_CHECK(env, ctx, "crt_write_accum", crt_write_accum(ctx, (const float *)p, s));
    return undefined(env);
}

static napi_value js_enable_counters(napi_env env, napi_callback_info info)
{
    ARGS(2)
    crt_ctx *ctx = get_ctx(env, argv[0]);
    if (!ctx) return NULL;
    bool on;
    NAPI_OK(env, napi_get_value_bool(env, argv[1], &on));
    CRT_CHECK(env, ctx, "crt_enable_counters", crt_enable_counters(ctx, on ? 1 : 0));
    return undefined(env);
}

static napi_value js_reset_counters(napi_env env, napi_callback_info info)
{
    ARGS(1)
    crt_ctx *ctx = get_ctx(env, argv[0]);
    if (!ctx) return NULL;
    CRT_CHECK(env, ctx, "crt_reset_counters", crt_reset_counters(ctx));
    return undefined(env);
}

static napi_value u64_array(napi_env env, const uint64_t *v, uint32_t n)
{
    napi_value arr;
    NAPI_OK(env, napi_create_array_with_length(env, n, &arr));
    for (uint32_t i = 0; i < n; i++) {
        napi_value d;
        NAPI_OK(env, napi_create_double(env, (double)v[i], &d));   /* exact below 2^53 */
        NAPI_OK(env, napi_set_element(env, arr, i, d));
    }
    return arr;
}

static napi_value js_counters(napi_env env, napi_callback_info info)
{
    ARGS(1)
    crt_ctx *ctx = get_ctx(env, argv[0]);
    if (!ctx) return NULL;
    uint64_t c[CRT_NCOUNTERS];
    CRT_CHECK(env, ctx, "crt_counters", crt_counters(ctx, c));
    return u64_array(env, c, CRT_NCOUNTERS);
}

static napi_value js_accel_stats(napi_env env, napi_callback_info info)
{
    ARGS(1)
    crt_ctx *ctx = get_ctx(env, argv[0]);
    if (!ctx) return NULL;
    uint64_t c[8];
    CRT_CHECK(env, ctx, "crt_accel_stats", crt_accel_stats(ctx, c));
    return u64_array(env, c, 8);
}

/* accelQuality(h) -> 12 numbers, as crt_accel_quality lays them out (NaN where a value is absent). */
static napi_value js_accel_quality(napi_env env, napi_callback_info info)
{
    ARGS(1)
    crt_ctx *ctx = get_ctx(env, argv[0]);
    if (!ctx) return NULL;
    double q[12];
    CRT_CHECK(env, ctx, "crt_accel_quality", crt_accel_quality(ctx, q));
    napi_value arr;
    NAPI_OK(env, napi_create_array_with_length(env, 12, &arr));
    for (uint32_t i = 0; i < 12; i++) {
        napi_value v;
        NAPI_OK(env, napi_create_double(env, q[i], &v));
        NAPI_OK(env, napi_set_element(env, arr, i, v));
    }
    return arr;
}

static napi_value js_last_trace_ms(napi_env env, napi_callback_info info)
{
    ARGS(1)
    crt_ctx *ctx = get_ctx(env, argv[0]);
    if (!ctx) return NULL;
    float ms = 0; uint32_t n = 0;
    CRT_CHECK(env, ctx, "crt_last_trace_ms", crt_last_trace_ms(ctx, &ms, &n));
    napi_value arr, a, b;
    NAPI_OK(env, napi_create_array_with_length(env, 2, &arr));
    NAPI_OK(env, napi_create_double(env, ms, &a));
    NAPI_OK(env, napi_create_uint32(env, n, &b));
    NAPI_OK(env, napi_set_element(env, arr, 0, a));
    NAPI_OK(env, napi_set_element(env, arr, 1, b));
    return arr;
}

static napi_value js_set_option(napi_env env, napi_callback_info info)
{
    ARGS(3)
    crt_ctx *ctx = get_ctx(env, argv[0]);
    if (!ctx) return NULL;
    char name[64]; size_t len; int64_t v;
    NAPI_OK(env, napi_get_value_string_utf8(env, argv[1], name, sizeof name, &len));
    NAPI_OK(env, napi_get_value_int64(env, argv[2], &v));
    CRT_CHECK(env, ctx, "crt_set_option", crt_set_option(ctx, name, v));
    return undefined(env);
}

/* The display step without stopping the pipeline (include/crt.h): the newest complete frame + its sample index. */
static napi_value js_read_latest_rgba8(napi_env env, napi_callback_info info)
{
    ARGS(1)
    crt_ctx *ctx = get_ctx(env, argv[0]);
    if (!ctx) return NULL;
    uint32_t t[4], smp = 0;
    CRT_CHECK(env, ctx, "crt_tile", crt_tile(ctx, t));
    size_t px = (size_t)t[2] * t[3];
    void *data = NULL;
    napi_value ab, ta, obj, sv;
    NAPI_OK(env, napi_create_arraybuffer(env, px * 4, &data, &ab));
    CRT_CHECK(env, ctx, "crt_read_latest_rgba8", crt_read_latest_rgba8(ctx, (uint8_t *)data, &smp));
    NAPI_OK(env, napi_create_typedarray(env, napi_uint8_array, px * 4, ab, 0, &ta));
    NAPI_OK(env, napi_create_object(env, &obj));
    NAPI_OK(env, napi_create_uint32(env, smp, &sv));
    NAPI_OK(env, napi_set_named_property(env, obj, "frame", ta));
    NAPI_OK(env, napi_set_named_property(env, obj, "sample", sv));
    return obj;
}

static napi_value js_latest_sample(napi_env env, napi_callback_info info)
{
    ARGS(1)
    crt_ctx *ctx = get_ctx(env, argv[0]);
    if (!ctx) return NULL;
    uint32_t s = 0;
    CRT_CHECK(env, ctx, "crt_latest_sample", crt_latest_sample(ctx, &s));
    napi_value out;
    NAPI_OK(env, napi_create_uint32(env, s, &out));
    return out;
}

static napi_value js_read_sample_rgba8(napi_env env, napi_callback_info info)
{
    ARGS(2)
    crt_ctx *ctx = get_ctx(env, argv[0]);
    if (!ctx) return NULL;
    uint32_t t[4], smp;
    NAPI_OK(env, napi_get_value_uint32(env, argv[1], &smp));
    CRT_CHECK(env, ctx, "crt_tile", crt_tile(ctx, t));
    size_t px = (size_t)t[2] * t[3];
    void *data = NULL;
    napi_value ab, ta;
    NAPI_OK(env, napi_create_arraybuffer(env, px * 4, &data, &ab));
    CRT_CHECK(env, ctx, "crt_read_sample_rgba8", crt_read_sample_rgba8(ctx, smp, (uint8_t *)data));
    NAPI_OK(env, napi_create_typedarray(env, napi_uint8_array, px * 4, ab, 0, &ta));
    return ta;
}

/* pinHost(typedArray) / unpinHost(typedArray): page-lock the array's memory; readSampleRgba8Into(h, k, typedArray) then reads
 * frame k straight into it (the caller's frame buffer, reused frame after frame). */
static napi_value js_pin_host(napi_env env, napi_callback_info info)
{
    ARGS(1)
    void *p; size_t n;
    if (!get_bytes(env, argv[0], &p, &n)) { napi_throw_type_error(env, NULL, "pinHost: typed array expected"); return NULL; }
    int rc = crt_pin_host(p, n);
    if (rc != CRT_OK) return throw_crt(env, NULL, rc, "crt_pin_host");
    return undefined(env);
}

static napi_value js_unpin_host(napi_env env, napi_callback_info info)
{
    ARGS(1)
    void *p; size_t n;
    if (!get_bytes(env, argv[0], &p, &n)) { napi_throw_type_error(env, NULL, "unpinHost: typed array expected"); return NULL; }
    int rc = crt_unpin_host(p);
    if (rc != CRT_OK) return throw_crt(env, NULL, rc, "crt_unpin_host");
    return undefined(env);
}

static napi_value js_read_sample_rgba8_into(napi_env env, napi_callback_info info)
{
    ARGS(3)
    crt_ctx *ctx = get_ctx(env, argv[0]);
    if (!ctx) return NULL;
    uint32_t t[4], smp;
    void *p; size_t n;
    NAPI_OK(env, napi_get_value_uint32(env, argv[1], &smp));
    if (!get_bytes(env, argv[2], &p, &n)) { napi_throw_type_error(env, NULL, "readSampleRgba8Into: typed array expected"); return NULL; }
    CRT_CHECK(env, ctx, "crt_tile", crt_tile(ctx, t));
    if (n < (size_t)t[2] * t[3] * 4) { napi_throw_range_error(env, NULL, "readSampleRgba8Into: need tw*th*4 bytes"); return NULL; }
    CRT_CHECK(env, ctx, "crt_read_sample_rgba8", crt_read_sample_rgba8(ctx, smp, (uint8_t *)p));
    return undefined(env);
}

/* ------------------------------------------------------------------ denoised preview (include/crt.h "Denoised preview")
 * denoise(h, {iterations, sigmaColor, sigmaNormal, sigmaPlane}) -> Uint8Array (tw*th*4 rgba8); a missing option (or a
 * missing object) takes the library's default.  readGbuffer(h) -> Float32Array (tw*th*8). */
static int opt_number(napi_env env, napi_value obj, const char *name, double *out)
{
    bool has = false;
    napi_value v;
    napi_valuetype t;
    if (napi_has_named_property(env, obj, name, &has) != napi_ok || !has) return 1;
    if (napi_get_named_property(env, obj, name, &v) != napi_ok || napi_typeof(env, v, &t) != napi_ok) return 0;
    if (t == napi_undefined) return 1;
    return t == napi_number && napi_get_value_double(env, v, out) == napi_ok;
}

/* One options object for the three filters.  `opts` lists (JS name, value): a property that is present and not undefined
 * must be a number and replaces *value; opts[0] is the iteration count, a non-negative integer.  `flag`, where one is
 * wanted, names a property whose truthiness goes to *flag_out.  Throws as `fn` and returns 0 on a refusal. */
typedef struct { const char *name; double *value; } dn_opt;

static int denoise_options(napi_env env, const char *fn, napi_value obj, int have_obj, const dn_opt *opts, size_t n_opts,
                           const char *flag, bool *flag_out)
{
    char msg[96];
    napi_valuetype t = napi_undefined;
    if (flag_out) *flag_out = false;
    if (have_obj && napi_typeof(env, obj, &t) != napi_ok) t = napi_boolean;
    if (t == napi_object) {
        for (size_t k = 0; k < n_opts; k++)
            if (!opt_number(env, obj, opts[k].name, opts[k].value)) {
                snprintf(msg, sizeof msg, "%s: options must be numbers", fn);
                napi_throw_type_error(env, NULL, msg);
                return 0;
            }
        bool has = false;
        napi_value v;
        if (flag_out && napi_has_named_property(env, obj, flag, &has) == napi_ok && has &&
            napi_get_named_property(env, obj, flag, &v) == napi_ok)
            napi_coerce_to_bool(env, v, &v), napi_get_value_bool(env, v, flag_out);
    } else if (t != napi_undefined && t != napi_null) {
        snprintf(msg, sizeof msg, "%s: options object expected", fn);
        napi_throw_type_error(env, NULL, msg);
        return 0;
    }
    const double it = *opts[0].value;
    if (!(it >= 0.0 && it <= 4294967295.0) || it != (double)(uint32_t)it) {
        snprintf(msg, sizeof msg, "%s: iterations must be a non-negative integer", fn);
        napi_throw_range_error(env, NULL, msg);
        return 0;
    }
    return 1;
}

/* The outputs of a filter call on the tile: rgba8 (tw*th*4 bytes) and, where wanted, one float per pixel. */
typedef struct { size_t px; void *rgba8, *plane; napi_value rgba8_ab, plane_ab; } dn_out;

static int outputs_of(napi_env env, crt_ctx *ctx, int frame, bool plane, dn_out *o)
{
    uint32_t tl[4];
    memset(o, 0, sizeof *o);
    const int rc = frame ? crt_image_size(ctx, tl + 2) : crt_tile(ctx, tl);
    if (rc != CRT_OK) { throw_crt(env, ctx, rc, frame ? "crt_image_size" : "crt_tile"); return 0; }
    o->px = (size_t)tl[2] * tl[3];
    if (napi_create_arraybuffer(env, o->px * 4, &o->rgba8, &o->rgba8_ab) != napi_ok ||
        (plane && napi_create_arraybuffer(env, o->px * 4, &o->plane, &o->plane_ab) != napi_ok)) {
        napi_throw_error(env, NULL, "out of memory");
        return 0;
    }
    return 1;
}

static int denoise_outputs(napi_env env, crt_ctx *ctx, bool plane, dn_out *o) { return outputs_of(env, ctx, 0, plane, o); }

/* ... as the call's result: the Uint8Array, or {rgba8, <name>: Float32Array(tw*th)} where the plane was wanted. */
static napi_value denoise_result(napi_env env, const dn_out *o, const char *name)
{
    napi_value ta, pta, obj;
    NAPI_OK(env, napi_create_typedarray(env, napi_uint8_array, o->px * 4, o->rgba8_ab, 0, &ta));
    if (!o->plane) return ta;
    NAPI_OK(env, napi_create_typedarray(env, napi_float32_array, o->px, o->plane_ab, 0, &pta));
    NAPI_OK(env, napi_create_object(env, &obj));
    NAPI_OK(env, napi_set_named_property(env, obj, "rgba8", ta));
    NAPI_OK(env, napi_set_named_property(env, obj, name, pta));
    return obj;
}

/* (handle, options?) of the three filters */
#define DENOISE_ARGS                                                                                \
    size_t argc = 2;                                                                                \
    napi_value argv[2];                                                                             \
    NAPI_OK(env, napi_get_cb_info(env, info, &argc, argv, NULL, NULL));                             \
    if (argc < 1) { napi_throw_type_error(env, NULL, "too few arguments"); return NULL; }           \
    crt_ctx *ctx = get_ctx(env, argv[0]);                                                           \
    if (!ctx) return NULL;

static int denoise_plain_options(napi_env env, const char *fn, napi_value opts, int have_opts, crt_denoise_params *p)
{
    double it = 5.0, sc = 1.0, sn = 0.5, sx = 0.3;
    const dn_opt o[] = {{"iterations", &it}, {"sigmaColor", &sc}, {"sigmaNormal", &sn}, {"sigmaPlane", &sx}};
    if (!denoise_options(env, fn, opts, have_opts, o, 4, NULL, NULL)) return 0;
    p->iterations = (uint32_t)it; p->sigma_color = (float)sc; p->sigma_normal = (float)sn; p->sigma_plane = (float)sx;
    return 1;
}

static napi_value js_denoise(napi_env env, napi_callback_info info)
{
    DENOISE_ARGS
    crt_denoise_params p;
    if (!denoise_plain_options(env, "denoise", argc > 1 ? argv[1] : NULL, argc > 1, &p)) return NULL;
    dn_out out;
    if (!denoise_outputs(env, ctx, false, &out)) return NULL;
    CRT_CHECK(env, ctx, "crt_denoise", crt_denoise(ctx, &p, NULL, (uint8_t *)out.rgba8));
    return denoise_result(env, &out, NULL);
}

/* denoiseLatest(h, {...denoise's options, rgb}) -> {rgba8: Uint8Array(tw*th*4), rgb?: Float32Array(tw*th*4), sample}: denoise
 * of the newest complete frame without finishing what is in flight (crt_denoise_latest); `sample` is the index of the frame
 * shown, and rgb: true adds the linear rgb.  Throws (CRT_ESTATE) while no frame is complete yet.
 * denoiseLatestInto(h, typedArray, {...denoise's options}) -> sample: the rgba8 straight into the caller's (pinned) frame
 * buffer, as readSampleRgba8Into.  denoiseLatestAsync(h, {...}) -> Promise of the object (below). */
static napi_value denoise_latest_result(napi_env env, size_t px, napi_value rgba8_ab, napi_value rgb_ab, uint32_t sample)
{
    napi_value ta, obj, v;
    NAPI_OK(env, napi_create_object(env, &obj));
    NAPI_OK(env, napi_create_typedarray(env, napi_uint8_array, px * 4, rgba8_ab, 0, &ta));
    NAPI_OK(env, napi_set_named_property(env, obj, "rgba8", ta));
    if (rgb_ab) {
        NAPI_OK(env, napi_create_typedarray(env, napi_float32_array, px * 4, rgb_ab, 0, &ta));
        NAPI_OK(env, napi_set_named_property(env, obj, "rgb", ta));
    }
    NAPI_OK(env, napi_create_uint32(env, sample, &v));
    NAPI_OK(env, napi_set_named_property(env, obj, "sample", v));
    return obj;
}

static int denoise_latest_options(napi_env env, const char *fn, napi_value opts, int have_opts, crt_denoise_params *p, bool *rgb)
{
    double it = 5.0, sc = 1.0, sn = 0.5, sx = 0.3;
    const dn_opt o[] = {{"iterations", &it}, {"sigmaColor", &sc}, {"sigmaNormal", &sn}, {"sigmaPlane", &sx}};
    if (!denoise_options(env, fn, opts, have_opts, o, 4, rgb ? "rgb" : NULL, rgb)) return 0;
    p->iterations = (uint32_t)it; p->sigma_color = (float)sc; p->sigma_normal = (float)sn; p->sigma_plane = (float)sx;
    return 1;
}

static napi_value js_denoise_latest(napi_env env, napi_callback_info info)
{
    DENOISE_ARGS
    crt_denoise_params p;
    bool rgb = false;
    if (!denoise_latest_options(env, "denoiseLatest", argc > 1 ? argv[1] : NULL, argc > 1, &p, &rgb)) return NULL;
    dn_out out;
    if (!denoise_outputs(env, ctx, false, &out)) return NULL;
    void *lin = NULL;
    napi_value lin_ab = NULL;
    if (rgb && napi_create_arraybuffer(env, out.px * 16, &lin, &lin_ab) != napi_ok) { napi_throw_error(env, NULL, "out of memory"); return NULL; }
    uint32_t smp = 0;
    CRT_CHECK(env, ctx, "crt_denoise_latest", crt_denoise_latest(ctx, &p, (float *)lin, (uint8_t *)out.rgba8, &smp));
    return denoise_latest_result(env, out.px, out.rgba8_ab, lin_ab, smp);
}

static napi_value js_denoise_latest_into(napi_env env, napi_callback_info info)
{
    size_t argc = 3;
    napi_value argv[3];
    NAPI_OK(env, napi_get_cb_info(env, info, &argc, argv, NULL, NULL));
    if (argc < 2) { napi_throw_type_error(env, NULL, "too few arguments"); return NULL; }
    crt_ctx *ctx = get_ctx(env, argv[0]);
    if (!ctx) return NULL;
    uint32_t t[4], smp = 0;
    void *dst; size_t n;
    crt_denoise_params p;
    if (!get_bytes(env, argv[1], &dst, &n)) { napi_throw_type_error(env, NULL, "denoiseLatestInto: typed array expected"); return NULL; }
    if (!denoise_latest_options(env, "denoiseLatestInto", argc > 2 ? argv[2] : NULL, argc > 2, &p, NULL)) return NULL;
    CRT_CHECK(env, ctx, "crt_tile", crt_tile(ctx, t));
    if (n < (size_t)t[2] * t[3] * 4) { napi_throw_range_error(env, NULL, "denoiseLatestInto: need tw*th*4 bytes"); return NULL; }
    CRT_CHECK(env, ctx, "crt_denoise_latest", crt_denoise_latest(ctx, &p, NULL, (uint8_t *)dst, &smp));
    napi_value out;
    NAPI_OK(env, napi_create_uint32(env, smp, &out));
    return out;
}

/* denoiseAdaptive(h, {iterations, sigmaVariance, sigmaNormal, sigmaPlane, variance}) -> Uint8Array (tw*th*4 rgba8), or
 * with variance: true -> {rgba8, variance: Float32Array(tw*th)}: the variance-guided filter of an adaptive render
 * (include/crt.h "Denoised preview of an adaptive render").  A missing option takes the library's default
 * (crt_denoise_adaptive_defaults).  denoiseAdaptiveAsync(h, {...}) -> Promise of the Uint8Array (below). */
static int denoise_adaptive_options(napi_env env, const char *fn, napi_value opts, int have_opts, crt_denoise_adaptive_params *p,
                                    bool *variance)
{
    if (crt_denoise_adaptive_defaults(p) != CRT_OK) { napi_throw_error(env, NULL, "crt_denoise_adaptive_defaults failed"); return 0; }
    double it = p->iterations, sv = p->sigma_variance, sn = p->sigma_normal, sx = p->sigma_plane;
    const dn_opt o[] = {{"iterations", &it}, {"sigmaVariance", &sv}, {"sigmaNormal", &sn}, {"sigmaPlane", &sx}};
    if (!denoise_options(env, fn, opts, have_opts, o, 4, variance ? "variance" : NULL, variance)) return 0;
    p->iterations = (uint32_t)it; p->sigma_variance = (float)sv; p->sigma_normal = (float)sn; p->sigma_plane = (float)sx;
    return 1;
}

static napi_value js_denoise_adaptive(napi_env env, napi_callback_info info)
{
    DENOISE_ARGS
    crt_denoise_adaptive_params p;
    bool variance = false;
    if (!denoise_adaptive_options(env, "denoiseAdaptive", argc > 1 ? argv[1] : NULL, argc > 1, &p, &variance)) return NULL;
    dn_out out;
    if (!denoise_outputs(env, ctx, variance, &out)) return NULL;
    CRT_CHECK(env, ctx, "crt_denoise_adaptive", crt_denoise_adaptive(ctx, &p, NULL, (uint8_t *)out.rgba8, (float *)out.plane));
    return denoise_result(env, &out, "variance");
}

/* denoiseFrame(h, {...denoise's options}) and denoiseAdaptiveFrame(h, {...denoiseAdaptive's}): the two filters over the whole
 * W x H frame of the latest PREVIEW gather, on any rank (include/crt.h "The frame of a partition"); the results as their
 * per-context forms give them, W*H pixels.  denoiseFrameAsync / denoiseAdaptiveFrameAsync -> Promise of the Uint8Array. */
static napi_value js_denoise_frame(napi_env env, napi_callback_info info)
{
    DENOISE_ARGS
    crt_denoise_params p;
    if (!denoise_plain_options(env, "denoiseFrame", argc > 1 ? argv[1] : NULL, argc > 1, &p)) return NULL;
    dn_out out;
    if (!outputs_of(env, ctx, 1, false, &out)) return NULL;
    CRT_CHECK(env, ctx, "crt_denoise_frame", crt_denoise_frame(ctx, &p, NULL, (uint8_t *)out.rgba8));
    return denoise_result(env, &out, NULL);
}

static napi_value js_denoise_adaptive_frame(napi_env env, napi_callback_info info)
{
    DENOISE_ARGS
    crt_denoise_adaptive_params p;
    bool variance = false;
    if (!denoise_adaptive_options(env, "denoiseAdaptive", argc > 1 ? argv[1] : NULL, argc > 1, &p, &variance)) return NULL;
    dn_out out;
    if (!outputs_of(env, ctx, 1, variance, &out)) return NULL;
    CRT_CHECK(env, ctx, "crt_denoise_adaptive_frame", crt_denoise_adaptive_frame(ctx, &p, NULL, (uint8_t *)out.rgba8, (float *)out.plane));
    return denoise_result(env, &out, "variance");
}

/* setSampleOffset(h, offset), sampleOffset(h) -> number, temporalReset(h): include/crt.h "Sample offset" and "Temporal
 * reuse across camera moves".
 * denoiseTemporal(h, {iterations, sigmaColor, sigmaNormal, sigmaPlane, maxHistory, normalTol, planeTol, history}) ->
 * Uint8Array (tw*th*4 rgba8), or with history: true -> {rgba8, history: Float32Array(tw*th)} (the weight Hw in samples).
 * A missing option takes the library's default (crt_denoise_temporal_defaults).  denoiseTemporalAsync(h, {...}) ->
 * Promise of the Uint8Array (below). */
static napi_value js_set_sample_offset(napi_env env, napi_callback_info info)
{
    ARGS(2)
    crt_ctx *ctx = get_ctx(env, argv[0]);
    if (!ctx) return NULL;
    uint32_t n;
    NAPI_OK(env, napi_get_value_uint32(env, argv[1], &n));
    CRT_CHECK(env, ctx, "crt_set_sample_offset", crt_set_sample_offset(ctx, n));
    return undefined(env);
}

static napi_value js_sample_offset(napi_env env, napi_callback_info info)
{
    ARGS(1)
    crt_ctx *ctx = get_ctx(env, argv[0]);
    if (!ctx) return NULL;
    uint32_t s = 0;
    CRT_CHECK(env, ctx, "crt_sample_offset", crt_sample_offset(ctx, &s));
    napi_value out;
    NAPI_OK(env, napi_create_uint32(env, s, &out));
    return out;
}

static napi_value js_temporal_reset(napi_env env, napi_callback_info info)
{
    ARGS(1)
    crt_ctx *ctx = get_ctx(env, argv[0]);
    if (!ctx) return NULL;
    CRT_CHECK(env, ctx, "crt_denoise_temporal_reset", crt_denoise_temporal_reset(ctx));
    return undefined(env);
}

static int denoise_temporal_options(napi_env env, napi_value opts, int have_opts, crt_denoise_temporal_params *p, bool *history)
{
    if (crt_denoise_temporal_defaults(p) != CRT_OK) { napi_throw_error(env, NULL, "crt_denoise_temporal_defaults failed"); return 0; }
    double it = p->iterations, sc = p->sigma_color, sn = p->sigma_normal, sx = p->sigma_plane, mh = p->max_history, nt = p->normal_tol,
           pt = p->plane_tol;
    const dn_opt o[] = {{"iterations", &it}, {"sigmaColor", &sc}, {"sigmaNormal", &sn}, {"sigmaPlane", &sx}, {"maxHistory", &mh},
                        {"normalTol", &nt}, {"planeTol", &pt}};
    if (!denoise_options(env, "denoiseTemporal", opts, have_opts, o, 7, "history", history)) return 0;
    p->iterations = (uint32_t)it;
    p->sigma_color = (float)sc; p->sigma_normal = (float)sn; p->sigma_plane = (float)sx;
    p->max_history = (float)mh; p->normal_tol = (float)nt; p->plane_tol = (float)pt;
    return 1;
}

static napi_value js_denoise_temporal(napi_env env, napi_callback_info info)
{
    DENOISE_ARGS
    crt_denoise_temporal_params p;
    bool history = false;
    if (!denoise_temporal_options(env, argc > 1 ? argv[1] : NULL, argc > 1, &p, &history)) return NULL;
    dn_out out;
    if (!denoise_outputs(env, ctx, history, &out)) return NULL;
    CRT_CHECK(env, ctx, "crt_denoise_temporal", crt_denoise_temporal(ctx, &p, NULL, (uint8_t *)out.rgba8, (float *)out.plane));
    return denoise_result(env, &out, "history");
}

/* denoiseSvgfDefaults() -> {iterations, sigmaVariance, sigmaNormal, sigmaPlane, maxHistory, normalTol, planeTol, minFrames}.
 * denoiseSvgf(h, {those, history, variance}) -> Uint8Array (tw*th*4 rgba8), or with history: true and / or variance: true
 * -> {rgba8, history?, variance?: Float32Array(tw*th)}: denoiseTemporal's blend followed by the variance-guided passes, the
 * variance taken from the temporal moments (include/crt.h "Variance-guided temporal filter").  A missing option takes the
 * library's default.  denoiseSvgfAsync(h, {...}) -> Promise of the Uint8Array (below).
 * readMoments(h) -> Float32Array (tw*th*4): (m1, s, Mw, 0) of the slot the last denoiseSvgf of this frame left. */
static napi_value js_denoise_svgf_defaults(napi_env env, napi_callback_info info)
{
    (void)info;
    crt_denoise_svgf_params p;
    if (crt_denoise_svgf_defaults(&p) != CRT_OK) { napi_throw_error(env, NULL, "crt_denoise_svgf_defaults failed"); return NULL; }
    const char *names[8] = {"iterations", "sigmaVariance", "sigmaNormal", "sigmaPlane", "maxHistory", "normalTol", "planeTol", "minFrames"};
    const double values[8] = {p.iterations, p.sigma_variance, p.sigma_normal, p.sigma_plane, p.max_history, p.normal_tol, p.plane_tol,
                              p.min_frames};
    napi_value obj, v;
    NAPI_OK(env, napi_create_object(env, &obj));
    for (int k = 0; k < 8; k++) {
        NAPI_OK(env, napi_create_double(env, values[k], &v));
        NAPI_OK(env, napi_set_named_property(env, obj, names[k], v));
    }
    return obj;
}

static int denoise_svgf_options(napi_env env, napi_value opts, int have_opts, crt_denoise_svgf_params *p, bool *history, bool *variance)
{
    if (crt_denoise_svgf_defaults(p) != CRT_OK) { napi_throw_error(env, NULL, "crt_denoise_svgf_defaults failed"); return 0; }
    double it = p->iterations, sv = p->sigma_variance, sn = p->sigma_normal, sx = p->sigma_plane, mh = p->max_history, nt = p->normal_tol,
           pt = p->plane_tol, mf = p->min_frames;
    const dn_opt o[] = {{"iterations", &it}, {"sigmaVariance", &sv}, {"sigmaNormal", &sn}, {"sigmaPlane", &sx}, {"maxHistory", &mh},
                        {"normalTol", &nt}, {"planeTol", &pt}, {"minFrames", &mf}};
    if (!denoise_options(env, "denoiseSvgf", opts, have_opts, o, 8, "history", history)) return 0;
    if (variance) {                                             /* (the options object has passed denoise_options' checks) */
        napi_valuetype t = napi_undefined;
        napi_value v;
        bool has = false;
        *variance = false;
        if (have_opts && napi_typeof(env, opts, &t) == napi_ok && t == napi_object &&
            napi_has_named_property(env, opts, "variance", &has) == napi_ok && has &&
            napi_get_named_property(env, opts, "variance", &v) == napi_ok)
            napi_coerce_to_bool(env, v, &v), napi_get_value_bool(env, v, variance);
    }
    p->iterations = (uint32_t)it;
    p->sigma_variance = (float)sv; p->sigma_normal = (float)sn; p->sigma_plane = (float)sx;
    p->max_history = (float)mh; p->normal_tol = (float)nt; p->plane_tol = (float)pt; p->min_frames = (float)mf;
    return 1;
}

static napi_value js_denoise_svgf(napi_env env, napi_callback_info info)
{
    DENOISE_ARGS
    crt_denoise_svgf_params p;
    bool history = false, variance = false;
    if (!denoise_svgf_options(env, argc > 1 ? argv[1] : NULL, argc > 1, &p, &history, &variance)) return NULL;
    dn_out out;
    if (!denoise_outputs(env, ctx, history, &out)) return NULL;
    void *var = NULL;
    napi_value var_ab, ta, pta, obj;
    if (variance) NAPI_OK(env, napi_create_arraybuffer(env, out.px * 4, &var, &var_ab));
    CRT_CHECK(env, ctx, "crt_denoise_svgf", crt_denoise_svgf(ctx, &p, NULL, (uint8_t *)out.rgba8, (float *)out.plane, (float *)var));
    if (!variance) return denoise_result(env, &out, "history");
    NAPI_OK(env, napi_create_typedarray(env, napi_uint8_array, out.px * 4, out.rgba8_ab, 0, &ta));
    NAPI_OK(env, napi_create_object(env, &obj));
    NAPI_OK(env, napi_set_named_property(env, obj, "rgba8", ta));
    if (history) {
        NAPI_OK(env, napi_create_typedarray(env, napi_float32_array, out.px, out.plane_ab, 0, &pta));
        NAPI_OK(env, napi_set_named_property(env, obj, "history", pta));
    }
    NAPI_OK(env, napi_create_typedarray(env, napi_float32_array, out.px, var_ab, 0, &pta));
    NAPI_OK(env, napi_set_named_property(env, obj, "variance", pta));
    return obj;
}

static napi_value js_read_moments(napi_env env, napi_callback_info info)
{
    ARGS(1)
    crt_ctx *ctx = get_ctx(env, argv[0]);
    if (!ctx) return NULL;
    uint32_t tl[4];
    CRT_CHECK(env, ctx, "crt_tile", crt_tile(ctx, tl));
    size_t px = (size_t)tl[2] * tl[3];
    void *data = NULL;
    napi_value ab, ta;
    NAPI_OK(env, napi_create_arraybuffer(env, px * 16, &data, &ab));
    CRT_CHECK(env, ctx, "crt_debug_read_moments", crt_debug_read_moments(ctx, (float *)data));
    NAPI_OK(env, napi_create_typedarray(env, napi_float32_array, px * 4, ab, 0, &ta));
    return ta;
}

/* debugReadClipBox(h) -> Float32Array (tw*th*8): per pixel lo.rgb, N, hi.rgb, valid of the box the last temporal call of
 * this frame clamped the history to under setOption(h, 'temporal_clip_pct', P) (include/crt.h "Clipped history"). */
static napi_value js_debug_read_clip_box(napi_env env, napi_callback_info info)
{
    ARGS(1)
    crt_ctx *ctx = get_ctx(env, argv[0]);
    if (!ctx) return NULL;
    uint32_t tl[4];
    CRT_CHECK(env, ctx, "crt_tile", crt_tile(ctx, tl));
    size_t px = (size_t)tl[2] * tl[3];
    void *data = NULL;
    napi_value ab, ta;
    NAPI_OK(env, napi_create_arraybuffer(env, px * 32, &data, &ab));
    CRT_CHECK(env, ctx, "crt_debug_read_clip_box", crt_debug_read_clip_box(ctx, (float *)data));
    NAPI_OK(env, napi_create_typedarray(env, napi_float32_array, px * 8, ab, 0, &ta));
    return ta;
}

static napi_value js_read_gbuffer(napi_env env, napi_callback_info info)
{
    ARGS(1)
    crt_ctx *ctx = get_ctx(env, argv[0]);
    if (!ctx) return NULL;
    uint32_t tl[4];
    CRT_CHECK(env, ctx, "crt_tile", crt_tile(ctx, tl));
    size_t px = (size_t)tl[2] * tl[3];
    void *data = NULL;
    napi_value ab, ta;
    NAPI_OK(env, napi_create_arraybuffer(env, px * 32, &data, &ab));
    CRT_CHECK(env, ctx, "crt_read_gbuffer", crt_read_gbuffer(ctx, (float *)data));
    NAPI_OK(env, napi_create_typedarray(env, napi_float32_array, px * 8, ab, 0, &ta));
    return ta;
}

/* renderAovs(h, n, {hits: Uint32Array(tw*th), alpha: Float32Array(tw*th), depth: Float32Array(tw*th),
 * normal: Float32Array(tw*th*4), albedo: Float32Array(tw*th*4)}): the feature planes of n samples (0: what the accumulator
 * holds) into the caller's typed arrays; a plane left out is not rendered (include/crt.h "Feature planes").  Blocking. */
static napi_value js_render_aovs(napi_env env, napi_callback_info info)
{
    ARGS(3)
    crt_ctx *ctx = get_ctx(env, argv[0]);
    if (!ctx) return NULL;
    uint32_t n = 0, tl[4];
    NAPI_OK(env, napi_get_value_uint32(env, argv[1], &n));
    CRT_CHECK(env, ctx, "crt_tile", crt_tile(ctx, tl));
    const size_t px = (size_t)tl[2] * tl[3];
    static const char *names[5] = {"hits", "alpha", "depth", "normal", "albedo"};
    static const size_t bytes_per_px[5] = {4, 4, 4, 16, 16};
    void *p[5] = {NULL, NULL, NULL, NULL, NULL};
    for (int i = 0; i < 5; i++) {
        bool has = false;
        napi_value v;
        NAPI_OK(env, napi_has_named_property(env, argv[2], names[i], &has));
        if (!has) continue;
        NAPI_OK(env, napi_get_named_property(env, argv[2], names[i], &v));
        size_t len = 0;
        if (!get_bytes(env, v, &p[i], &len) || len != px * bytes_per_px[i]) {
            char m[128];
            snprintf(m, sizeof m, "renderAovs: %s must be a typed array of %zu bytes", names[i], px * bytes_per_px[i]);
            napi_throw_type_error(env, NULL, m);
            return NULL;
        }
    }
    const crt_aov_planes out = {(uint32_t *)p[0], (float *)p[1], (float *)p[2], (float *)p[3], (float *)p[4]};
    CRT_CHECK(env, ctx, "crt_render_aovs", crt_render_aovs(ctx, n, &out));
    return undefined(env);
}

/* renderMattes(h, n, source, slots, {ids: Uint32Array(slots*tw*th), counts: Uint32Array(slots*tw*th), hits:
 * Uint32Array(tw*th), overflow: Uint32Array(tw*th)}): the id mattes of n samples (0: what the accumulator holds) into the
 * caller's typed arrays; source 0 = primitive, 1 = object (the id table), 2 = material; a plane left out is not rendered
 * (include/crt.h "ID mattes").  Blocking. */
static napi_value js_render_mattes(napi_env env, napi_callback_info info)
{
    ARGS(5)
    crt_ctx *ctx = get_ctx(env, argv[0]);
    if (!ctx) return NULL;
    uint32_t n = 0, slots = 0, tl[4];
    int32_t source = 0;
    NAPI_OK(env, napi_get_value_uint32(env, argv[1], &n));
    NAPI_OK(env, napi_get_value_int32(env, argv[2], &source));
    NAPI_OK(env, napi_get_value_uint32(env, argv[3], &slots));
    CRT_CHECK(env, ctx, "crt_tile", crt_tile(ctx, tl));
    const size_t px = (size_t)tl[2] * tl[3];
    static const char *names[4] = {"ids", "counts", "hits", "overflow"};
    const size_t want[4] = {px * slots * 4, px * slots * 4, px * 4, px * 4};
    void *p[4] = {NULL, NULL, NULL, NULL};
    for (int i = 0; i < 4; i++) {
        bool has = false;
        napi_value v;
        NAPI_OK(env, napi_has_named_property(env, argv[4], names[i], &has));
        if (!has) continue;
        NAPI_OK(env, napi_get_named_property(env, argv[4], names[i], &v));
        size_t len = 0;
        if (!get_bytes(env, v, &p[i], &len) || len != want[i]) {
            char m[128];
            snprintf(m, sizeof m, "renderMattes: %s must be a typed array of %zu bytes", names[i], want[i]);
            napi_throw_type_error(env, NULL, m);
            return NULL;
        }
    }
    const crt_matte_planes out = {(uint32_t *)p[0], (uint32_t *)p[1], (uint32_t *)p[2], (uint32_t *)p[3]};
    CRT_CHECK(env, ctx, "crt_render_mattes", crt_render_mattes(ctx, n, source, slots, &out));
    return undefined(env);
}

/* setPrimitiveIds(h, first, Uint32Array): replaces entries [first, first + length) of the id table that source 1 reports
 * (crt_set_primitive_ids); nothing else changes. */
static napi_value js_set_primitive_ids(napi_env env, napi_callback_info info)
{
    ARGS(3)
    crt_ctx *ctx = get_ctx(env, argv[0]);
    if (!ctx) return NULL;
    uint32_t first = 0;
    NAPI_OK(env, napi_get_value_uint32(env, argv[1], &first));
    void *p = NULL; size_t n = 0;
    if (!get_bytes(env, argv[2], &p, &n) || n % 4) {
        napi_throw_type_error(env, NULL, "setPrimitiveIds: ids must be a Uint32Array");
        return NULL;
    }
    CRT_CHECK(env, ctx, "crt_set_primitive_ids", crt_set_primitive_ids(ctx, first, (uint32_t)(n / 4), n ? (const uint32_t *)p : NULL));
    return undefined(env);
}

/* queryRays(h, Float32Array(n*8), mode, {hit: Uint32Array(n), prim: Uint32Array(n), id: Uint32Array(n), t: Float32Array(n),
 * position: Float32Array(n*4), normal: Float32Array(n*4), uv: Float32Array(n*2)}): what n caller rays hit -- each ray 8
 * floats (o, t_max, d, exclude bits), mode 0 = the closest hit, 1 = any hit (the `hit` plane alone) -- into the caller's
 * typed arrays; a plane left out is not computed (include/crt.h "Ray queries").  Blocking for the query alone: work in
 * flight is neither finished nor disturbed. */
static const char *const query_names[7] = {"hit", "prim", "id", "t", "position", "normal", "uv"};
static const size_t query_bytes[7] = {4, 4, 4, 4, 16, 16, 8};

static int query_planes(napi_env env, napi_value obj, size_t n, const char *who, crt_query_planes *out)
{
    void *p[7] = {NULL, NULL, NULL, NULL, NULL, NULL, NULL};
    for (int i = 0; i < 7; i++) {
        bool has = false;
        napi_value v;
        if (napi_has_named_property(env, obj, query_names[i], &has) != napi_ok) has = false;
        if (!has) continue;
        size_t len = 0;
        if (napi_get_named_property(env, obj, query_names[i], &v) != napi_ok || !get_bytes(env, v, &p[i], &len) || len != n * query_bytes[i]) {
            char m[128];
            snprintf(m, sizeof m, "%s: %s must be a typed array of %zu bytes", who, query_names[i], n * query_bytes[i]);
            napi_throw_type_error(env, NULL, m);
            return 0;
        }
    }
    const crt_query_planes q = {(uint32_t *)p[0], (uint32_t *)p[1], (uint32_t *)p[2], (float *)p[3], (float *)p[4], (float *)p[5], (float *)p[6]};
    *out = q;
    return 1;
}

static napi_value js_query_rays(napi_env env, napi_callback_info info)
{
    ARGS(4)
    crt_ctx *ctx = get_ctx(env, argv[0]);
    if (!ctx) return NULL;
    void *rays = NULL; size_t bytes = 0;
    if (!get_bytes(env, argv[1], &rays, &bytes) || bytes % sizeof(crt_ray)) {
        napi_throw_type_error(env, NULL, "queryRays: rays must be a Float32Array of 8 floats per ray");
        return NULL;
    }
    int32_t mode = 0;
    NAPI_OK(env, napi_get_value_int32(env, argv[2], &mode));
    const size_t n = bytes / sizeof(crt_ray);
    crt_query_planes out;
    if (!query_planes(env, argv[3], n, "queryRays", &out)) return NULL;
    CRT_CHECK(env, ctx, "crt_query_rays", crt_query_rays(ctx, n ? (const crt_ray *)rays : NULL, n, mode, &out));
    return undefined(env);
}

/* radianceRays(h, Float32Array(n*8), Uint32Array(n*4) | null, nSamples, planes?) -> {xyz: Float32Array(n*4), y2:
 * Float32Array(n), rgba8: Uint8Array(n*4)}: the path tracer's radiance along n caller rays -- each ray 8 floats (o, t_max,
 * d, exclude bits), each key (x, y, first sample, 0), null = (i, 0, 1) -- summed over nSamples paths per ray (include/crt.h
 * "Radiance queries").  planes: an array of the names wanted (default: all three).  Blocking for the call alone: work in
 * flight is neither finished nor disturbed. */
static napi_value js_radiance_rays(napi_env env, napi_callback_info info)
{
    size_t argc = 5;
    napi_value argv[5];
    NAPI_OK(env, napi_get_cb_info(env, info, &argc, argv, NULL, NULL));
    if (argc < 4) {
        napi_throw_type_error(env, NULL, "radianceRays: expected (handle, rays, keys | null, nSamples, planes?)");
        return NULL;
    }
    crt_ctx *ctx = get_ctx(env, argv[0]);
    if (!ctx) return NULL;
    void *rays = NULL, *keys = NULL; size_t bytes = 0, kbytes = 0;
    if (!get_bytes(env, argv[1], &rays, &bytes) || bytes % sizeof(crt_ray)) {
        napi_throw_type_error(env, NULL, "radianceRays: rays must be a Float32Array of 8 floats per ray");
        return NULL;
    }
    const size_t n = bytes / sizeof(crt_ray);
    napi_valuetype kt = napi_undefined;
    NAPI_OK(env, napi_typeof(env, argv[2], &kt));
    const bool have_keys = kt != napi_null && kt != napi_undefined;
    if (have_keys && (!get_bytes(env, argv[2], &keys, &kbytes) || kbytes != n * sizeof(crt_path_key))) {
        napi_throw_type_error(env, NULL, "radianceRays: keys must be null or a Uint32Array of 4 per ray");
        return NULL;
    }
    uint32_t n_samples = 0;
    NAPI_OK(env, napi_get_value_uint32(env, argv[3], &n_samples));
    static const char *const names[3] = {"xyz", "y2", "rgba8"};
    bool want[3] = {true, true, true};
    if (argc >= 5) {
        napi_valuetype pt = napi_undefined;
        NAPI_OK(env, napi_typeof(env, argv[4], &pt));
        if (pt != napi_undefined && pt != napi_null) {
            bool is_array = false;
            uint32_t count = 0;
            if (napi_is_array(env, argv[4], &is_array) != napi_ok || !is_array || napi_get_array_length(env, argv[4], &count) != napi_ok) {
                napi_throw_type_error(env, NULL, "radianceRays: planes must be an array of plane names");
                return NULL;
            }
            want[0] = want[1] = want[2] = false;
            for (uint32_t i = 0; i < count; i++) {
                napi_value v;
                char name[16];
                size_t len = 0;
                int k = -1;
                if (napi_get_element(env, argv[4], i, &v) == napi_ok && napi_get_value_string_utf8(env, v, name, sizeof name, &len) == napi_ok)
                    for (int j = 0; j < 3; j++) if (!strcmp(name, names[j])) k = j;
                if (k < 0) {
                    napi_throw_type_error(env, NULL, "radianceRays: planes holds a name other than xyz, y2, rgba8");
                    return NULL;
                }
                want[k] = true;
            }
        }
    }
    static const size_t elem[3] = {16, 4, 4};
    static const napi_typedarray_type kind[3] = {napi_float32_array, napi_float32_array, napi_uint8_array};
    static const size_t per[3] = {4, 1, 4};
    void *data[3] = {NULL, NULL, NULL};
    napi_value ab[3], res, v;
    for (int j = 0; j < 3; j++)
        if (want[j]) NAPI_OK(env, napi_create_arraybuffer(env, n * elem[j], &data[j], &ab[j]));
    const crt_radiance_planes out = {(float *)data[0], (float *)data[1], (uint8_t *)data[2]};
    if (n)                                                       /* (an empty ArrayBuffer may have no address: every plane would be NULL) */
        CRT_CHECK(env, ctx, "crt_radiance_rays", crt_radiance_rays(ctx, (const crt_ray *)rays, have_keys ? (const crt_path_key *)keys : NULL, n, n_samples, &out));
    NAPI_OK(env, napi_create_object(env, &res));
    for (int j = 0; j < 3; j++) {
        if (!want[j]) continue;
        NAPI_OK(env, napi_create_typedarray(env, kind[j], n * per[j], ab[j], 0, &v));
        NAPI_OK(env, napi_set_named_property(env, res, names[j], v));
    }
    return res;
}

/* pick(h, x, y) -> {hit, prim, id, t, position: Float32Array(4), normal: Float32Array(4), uv: Float32Array(2)}: what the
 * camera ray of pixel (x, y) of the full image hits (crt_pick; global coordinates), hit = 0 with prim = id = 0xFFFFFFFF
 * where it hits nothing.  Blocking for the query alone. */
static napi_value js_pick(napi_env env, napi_callback_info info)
{
    ARGS(3)
    crt_ctx *ctx = get_ctx(env, argv[0]);
    if (!ctx) return NULL;
    uint32_t xy[2] = {0, 0};
    NAPI_OK(env, napi_get_value_uint32(env, argv[1], &xy[0]));
    NAPI_OK(env, napi_get_value_uint32(env, argv[2], &xy[1]));
    napi_value ab, res, v;
    void *data = NULL;
    NAPI_OK(env, napi_create_arraybuffer(env, 64, &data, &ab));      /* position, normal, uv, then hit, prim, id, t */
    float *f = (float *)data;
    uint32_t *u = (uint32_t *)data + 10;
    const crt_query_planes out = {u, u + 1, u + 2, f + 13, f, f + 4, f + 8};
    CRT_CHECK(env, ctx, "crt_pick", crt_pick(ctx, xy, 1, &out));
    NAPI_OK(env, napi_create_object(env, &res));
    NAPI_OK(env, napi_create_uint32(env, u[0], &v)); NAPI_OK(env, napi_set_named_property(env, res, "hit", v));
    NAPI_OK(env, napi_create_uint32(env, u[1], &v)); NAPI_OK(env, napi_set_named_property(env, res, "prim", v));
    NAPI_OK(env, napi_create_uint32(env, u[2], &v)); NAPI_OK(env, napi_set_named_property(env, res, "id", v));
    NAPI_OK(env, napi_create_double(env, (double)f[13], &v)); NAPI_OK(env, napi_set_named_property(env, res, "t", v));
    NAPI_OK(env, napi_create_typedarray(env, napi_float32_array, 4, ab, 0, &v)); NAPI_OK(env, napi_set_named_property(env, res, "position", v));
    NAPI_OK(env, napi_create_typedarray(env, napi_float32_array, 4, ab, 16, &v)); NAPI_OK(env, napi_set_named_property(env, res, "normal", v));
    NAPI_OK(env, napi_create_typedarray(env, napi_float32_array, 2, ab, 32, &v)); NAPI_OK(env, napi_set_named_property(env, res, "uv", v));
    return res;
}

/* readMotion(h) -> Float32Array (tw*th*2): per pixel the film position (u, v) where the last denoiseTemporal looked for
 * it in the previous frame, NaN where there is none (include/crt.h crt_read_motion). */
static napi_value js_read_motion(napi_env env, napi_callback_info info)
{
    ARGS(1)
    crt_ctx *ctx = get_ctx(env, argv[0]);
    if (!ctx) return NULL;
    uint32_t tl[4];
    CRT_CHECK(env, ctx, "crt_tile", crt_tile(ctx, tl));
    size_t px = (size_t)tl[2] * tl[3];
    void *data = NULL;
    napi_value ab, ta;
    NAPI_OK(env, napi_create_arraybuffer(env, px * 8, &data, &ab));
    CRT_CHECK(env, ctx, "crt_read_motion", crt_read_motion(ctx, (float *)data));
    NAPI_OK(env, napi_create_typedarray(env, napi_float32_array, px * 2, ab, 0, &ta));
    return ta;
}

/* ------------------------------------------------------------------ scene edits (include/crt.h "Scene edits")
 * setCamera(h, camera: 16 floats), updatePrimitives(h, first, records: k*80 B), updateLights(h, first, records),
 * refitAccel(h) -> true when the tree had to be rebuilt. */
static napi_value js_set_camera(napi_env env, napi_callback_info info)
{
    ARGS(2)
    crt_ctx *ctx = get_ctx(env, argv[0]);
    if (!ctx) return NULL;
    void *p = NULL; size_t n = 0;
    if (!get_bytes(env, argv[1], &p, &n) || n != 64) {
        napi_throw_type_error(env, NULL, "setCamera: camera must be 16 floats (64 bytes)");
        return NULL;
    }
    CRT_CHECK(env, ctx, "crt_set_camera", crt_set_camera(ctx, (const float *)p));
    return undefined(env);
}

static napi_value update_records(napi_env env, napi_callback_info info, int lights)
{
    ARGS(3)
    crt_ctx *ctx = get_ctx(env, argv[0]);
    if (!ctx) return NULL;
    uint32_t first = 0;
    NAPI_OK(env, napi_get_value_uint32(env, argv[1], &first));
    void *p = NULL; size_t n = 0;
    if (!get_bytes(env, argv[2], &p, &n) || n % 80) {
        napi_throw_type_error(env, NULL, lights ? "updateLights: records must be k*80 bytes" : "updatePrimitives: records must be k*80 bytes");
        return NULL;
    }
    if (lights) CRT_CHECK(env, ctx, "crt_update_lights", crt_update_lights(ctx, first, (uint32_t)(n / 80), p));
    else CRT_CHECK(env, ctx, "crt_update_primitives", crt_update_primitives(ctx, first, (uint32_t)(n / 80), p));
    return undefined(env);
}
static napi_value js_update_primitives(napi_env env, napi_callback_info info) { return update_records(env, info, 0); }
static napi_value js_update_lights(napi_env env, napi_callback_info info) { return update_records(env, info, 1); }

/* transformPrimitives(h, ops: k*60 B, packed crt_prim_transform records {u32 first, u32 count, f32 m[12], f32
 * radius_scale}) moves the ranges on the device; readPrimitives(h, first, count) -> Uint8Array (count*80 B), the records
 * as the device holds them.  transformPrimitivesAsync / readPrimitivesAsync: the Promise forms (below). */
static napi_value js_transform_primitives(napi_env env, napi_callback_info info)
{
    ARGS(2)
    crt_ctx *ctx = get_ctx(env, argv[0]);
    if (!ctx) return NULL;
    void *p = NULL; size_t n = 0;
    if (!get_bytes(env, argv[1], &p, &n) || n % sizeof(crt_prim_transform)) {
        napi_throw_type_error(env, NULL, "transformPrimitives: ops must be k*60 bytes");
        return NULL;
    }
    CRT_CHECK(env, ctx, "crt_transform_primitives", crt_transform_primitives(ctx, (const crt_prim_transform *)p, (uint32_t)(n / sizeof(crt_prim_transform))));
    return undefined(env);
}

/* removePrimitives(h, ranges: k*8 B, packed crt_prim_range records {u32 first, u32 count}, lights?: m*80 B) and
 * appendPrimitives(h, records: k*80 B, lights?: m*80 B): crt_remove_primitives / crt_append_primitives.  lights missing,
 * undefined or null keeps the light list.  removePrimitivesAsync / appendPrimitivesAsync: the Promise forms (below). */
static int optional_lights(napi_env env, size_t argc, napi_value *argv, void **p, size_t *n)
{
    napi_valuetype t = napi_undefined;
    *p = NULL; *n = 0;
    if (argc < 3 || napi_typeof(env, argv[2], &t) != napi_ok || t == napi_undefined || t == napi_null) return 1;
    return get_bytes(env, argv[2], p, n) && *n % 80 == 0;
}

static napi_value edit_topology(napi_env env, napi_callback_info info, int append)
{
    size_t argc = 3;
    napi_value argv[3];
    NAPI_OK(env, napi_get_cb_info(env, info, &argc, argv, NULL, NULL));
    if (argc < 2) { napi_throw_type_error(env, NULL, "too few arguments"); return NULL; }
    crt_ctx *ctx = get_ctx(env, argv[0]);
    if (!ctx) return NULL;
    void *p = NULL, *lp = NULL; size_t n = 0, ln = 0;
    if (!get_bytes(env, argv[1], &p, &n) || n % (append ? 80 : sizeof(crt_prim_range))) {
        napi_throw_type_error(env, NULL, append ? "appendPrimitives: records must be k*80 bytes" : "removePrimitives: ranges must be k*8 bytes");
        return NULL;
    }
    if (!optional_lights(env, argc, argv, &lp, &ln)) {
        napi_throw_type_error(env, NULL, "removePrimitives / appendPrimitives: lights must be m*80 bytes, null or left out");
        return NULL;
    }
    if (append) CRT_CHECK(env, ctx, "crt_append_primitives", crt_append_primitives(ctx, p, (uint32_t)(n / 80), lp, ln / 80));
    else CRT_CHECK(env, ctx, "crt_remove_primitives", crt_remove_primitives(ctx, (const crt_prim_range *)p, (uint32_t)(n / sizeof(crt_prim_range)), lp, ln / 80));
    return undefined(env);
}
static napi_value js_remove_primitives(napi_env env, napi_callback_info info) { return edit_topology(env, info, 0); }
static napi_value js_append_primitives(napi_env env, napi_callback_info info) { return edit_topology(env, info, 1); }

static napi_value js_read_primitives(napi_env env, napi_callback_info info)
{
    ARGS(3)
    crt_ctx *ctx = get_ctx(env, argv[0]);
    if (!ctx) return NULL;
    uint32_t first = 0, count = 0;
    NAPI_OK(env, napi_get_value_uint32(env, argv[1], &first));
    NAPI_OK(env, napi_get_value_uint32(env, argv[2], &count));
    void *data = NULL;
    napi_value ab, ta;
    NAPI_OK(env, napi_create_arraybuffer(env, (size_t)count * 80, &data, &ab));
    CRT_CHECK(env, ctx, "crt_read_primitives", crt_read_primitives(ctx, first, count, count ? data : NULL));
    NAPI_OK(env, napi_create_typedarray(env, napi_uint8_array, (size_t)count * 80, ab, 0, &ta));
    return ta;
}

static napi_value js_refit_accel(napi_env env, napi_callback_info info)
{
    ARGS(1)
    crt_ctx *ctx = get_ctx(env, argv[0]);
    if (!ctx) return NULL;
    int rebuilt = 0;
    CRT_CHECK(env, ctx, "crt_refit_accel", crt_refit_accel(ctx, &rebuilt));
    napi_value b;
    NAPI_OK(env, napi_get_boolean(env, rebuilt != 0, &b));
    return b;
}

/* ------------------------------------------------------------------ adaptive sampling (include/crt.h "Adaptive sampling")
 * traceAdaptive(h, {samples, threshold, minSamples, maxSamples}) -> active tiles (0: done); a missing option takes the
 * library's default (crt_adaptive_defaults).  readAdaptive(h) -> {counts: Uint32Array, errors: Float32Array, tilesX, tilesY}. */
static napi_value trace_adaptive(napi_env env, napi_callback_info info, int filtered)
{
    const char *fn = filtered ? "traceAdaptiveFiltered" : "traceAdaptive";
    char msg[128];
    size_t argc = 2;
    napi_value argv[2];
    NAPI_OK(env, napi_get_cb_info(env, info, &argc, argv, NULL, NULL));
    if (argc < 1) { napi_throw_type_error(env, NULL, "too few arguments"); return NULL; }
    crt_ctx *ctx = get_ctx(env, argv[0]);
    if (!ctx) return NULL;
    crt_adaptive_params d;
    (void)crt_adaptive_defaults(&d);
    double s = d.samples, thr = d.threshold, mn = d.min_samples, mx = d.max_samples;
    napi_valuetype t = napi_undefined;
    if (argc > 1) NAPI_OK(env, napi_typeof(env, argv[1], &t));
    if (t == napi_object) {
        if (!opt_number(env, argv[1], "samples", &s) || !opt_number(env, argv[1], "threshold", &thr) ||
            !opt_number(env, argv[1], "minSamples", &mn) || !opt_number(env, argv[1], "maxSamples", &mx)) {
            snprintf(msg, sizeof msg, "%s: options must be numbers", fn);
            napi_throw_type_error(env, NULL, msg);
            return NULL;
        }
    } else if (t != napi_undefined && t != napi_null) {
        snprintf(msg, sizeof msg, "%s: options object expected", fn);
        napi_throw_type_error(env, NULL, msg);
        return NULL;
    }
    const double counts[3] = {s, mn, mx};
    for (int k = 0; k < 3; k++)
        if (!(counts[k] >= 0.0 && counts[k] <= 4294967295.0) || counts[k] != (double)(uint32_t)counts[k]) {
            snprintf(msg, sizeof msg, "%s: samples, minSamples and maxSamples must be non-negative integers", fn);
            napi_throw_range_error(env, NULL, msg);
            return NULL;
        }
    crt_adaptive_params p = {(uint32_t)s, (uint32_t)mn, (uint32_t)mx, (float)thr};
    uint32_t n = 0;
    if (filtered) {                                              /* (the filter's options live in the same object) */
        crt_denoise_adaptive_params f;
        if (!denoise_adaptive_options(env, fn, argc > 1 ? argv[1] : NULL, argc > 1, &f, NULL)) return NULL;
        CRT_CHECK(env, ctx, "crt_trace_adaptive_filtered", crt_trace_adaptive_filtered(ctx, &p, &f, &n));
    } else {
        CRT_CHECK(env, ctx, "crt_trace_adaptive", crt_trace_adaptive(ctx, &p, &n));
    }
    napi_value v;
    NAPI_OK(env, napi_create_uint32(env, n, &v));
    return v;
}
static napi_value js_trace_adaptive(napi_env env, napi_callback_info info) { return trace_adaptive(env, info, 0); }
/* traceAdaptiveFiltered(h, {samples, threshold, minSamples, maxSamples, iterations, sigmaVariance, sigmaNormal, sigmaPlane})
 * -> active tiles: traceAdaptive with the tiles judged by the variance denoiseAdaptive leaves (include/crt.h "Adaptive
 * sampling judged by the filtered preview"); readAdaptiveFiltered(h, {iterations, sigmaVariance, sigmaNormal, sigmaPlane})
 * -> readAdaptive's object with errors = E'. */
static napi_value js_trace_adaptive_filtered(napi_env env, napi_callback_info info) { return trace_adaptive(env, info, 1); }

/* readAdaptive(h) -> {counts, errors, tilesX, tilesY} of the context's rectangle; readFrameAdaptive(h): of the whole frame of
 * the latest PREVIEW gather (include/crt.h "The frame of a partition"). */
static napi_value read_adaptive(napi_env env, napi_callback_info info, int frame)
{
    size_t argc = 2;
    napi_value argv[2];
    NAPI_OK(env, napi_get_cb_info(env, info, &argc, argv, NULL, NULL));
    if (argc < 1) { napi_throw_type_error(env, NULL, "too few arguments"); return NULL; }
    crt_ctx *ctx = get_ctx(env, argv[0]);
    if (!ctx) return NULL;
    const int filtered = frame == 2;                             /* readAdaptiveFiltered(h, {the filter's options}) */
    frame = frame == 1;
    crt_denoise_adaptive_params f;
    if (filtered && !denoise_adaptive_options(env, "readAdaptiveFiltered", argc > 1 ? argv[1] : NULL, argc > 1, &f, NULL)) return NULL;
    uint32_t tl[4];
    if (frame) CRT_CHECK(env, ctx, "crt_image_size", crt_image_size(ctx, tl + 2));
    else CRT_CHECK(env, ctx, "crt_tile", crt_tile(ctx, tl));
    const uint32_t tx = (tl[2] + 7) / 8, ty = (tl[3] + 7) / 8;
    const size_t nt = (size_t)tx * ty;
    void *dc = NULL, *de = NULL;
    napi_value abc, abe, tc, te, obj, vx, vy;
    NAPI_OK(env, napi_create_arraybuffer(env, nt * 4, &dc, &abc));
    NAPI_OK(env, napi_create_arraybuffer(env, nt * 4, &de, &abe));
    if (frame) CRT_CHECK(env, ctx, "crt_read_frame_adaptive", crt_read_frame_adaptive(ctx, (uint32_t *)dc, (float *)de));
    else if (filtered) CRT_CHECK(env, ctx, "crt_read_adaptive_filtered", crt_read_adaptive_filtered(ctx, &f, (uint32_t *)dc, (float *)de));
    else CRT_CHECK(env, ctx, "crt_read_adaptive", crt_read_adaptive(ctx, (uint32_t *)dc, (float *)de));
    NAPI_OK(env, napi_create_typedarray(env, napi_uint32_array, nt, abc, 0, &tc));
    NAPI_OK(env, napi_create_typedarray(env, napi_float32_array, nt, abe, 0, &te));
    NAPI_OK(env, napi_create_object(env, &obj));
    NAPI_OK(env, napi_create_uint32(env, tx, &vx));
    NAPI_OK(env, napi_create_uint32(env, ty, &vy));
    NAPI_OK(env, napi_set_named_property(env, obj, "counts", tc));
    NAPI_OK(env, napi_set_named_property(env, obj, "errors", te));
    NAPI_OK(env, napi_set_named_property(env, obj, "tilesX", vx));
    NAPI_OK(env, napi_set_named_property(env, obj, "tilesY", vy));
    return obj;
}
static napi_value js_read_adaptive(napi_env env, napi_callback_info info) { return read_adaptive(env, info, 0); }
static napi_value js_read_frame_adaptive(napi_env env, napi_callback_info info) { return read_adaptive(env, info, 1); }
static napi_value js_read_adaptive_filtered(napi_env env, napi_callback_info info) { return read_adaptive(env, info, 2); }

/* ------------------------------------------------------------------ multi-GPU (include/crt.h "Multi-GPU") and composition
 * The reference drives one GPUDevice (src/main.js:8-9); a Node host reaches the tile-partitioned configurations through
 * these: one process (worker) per GPU, the communicator id made by one of them and passed around by the parent
 * (host/multi.js). */
static napi_value js_comm_unique_id(napi_env env, napi_callback_info info)
{
    ARGS(1)
    bool local = false;
    NAPI_OK(env, napi_get_value_bool(env, argv[0], &local));
    void *data = NULL;
    napi_value ab;
    NAPI_OK(env, napi_create_arraybuffer(env, CRT_COMM_ID_BYTES, &data, &ab));
    int rc = crt_comm_unique_id(data, local ? CRT_COMM_LOCAL : CRT_COMM_RCCL);
    if (rc != CRT_OK) return throw_crt(env, NULL, rc, "crt_comm_unique_id");
    return ab;
}

static napi_value js_comm_init(napi_env env, napi_callback_info info)
{
    ARGS(4)
    crt_ctx *ctx = get_ctx(env, argv[0]);
    if (!ctx) return NULL;
    void *p; size_t n;
    int32_t rank, world;
    if (!get_bytes(env, argv[1], &p, &n) || n != CRT_COMM_ID_BYTES) { napi_throw_type_error(env, NULL, "commInit: the id is the 128-byte buffer of commUniqueId"); return NULL; }
    NAPI_OK(env, napi_get_value_int32(env, argv[2], &rank));
    NAPI_OK(env, napi_get_value_int32(env, argv[3], &world));
    CRT_CHECK(env, ctx, "crt_comm_init", crt_comm_init(ctx, p, rank, world));
    return undefined(env);
}

static napi_value js_comm_partition(napi_env env, napi_callback_info info)
{
    ARGS(2)
    crt_ctx *ctx = get_ctx(env, argv[0]);
    if (!ctx) return NULL;
    uint32_t band;
    NAPI_OK(env, napi_get_value_uint32(env, argv[1], &band));
    CRT_CHECK(env, ctx, "crt_comm_partition", crt_comm_partition(ctx, band));
    return undefined(env);
}

static napi_value js_comm_info(napi_env env, napi_callback_info info)
{
    ARGS(1)
    crt_ctx *ctx = get_ctx(env, argv[0]);
    if (!ctx) return NULL;
    int v[4];
    CRT_CHECK(env, ctx, "crt_comm_info", crt_comm_info(ctx, v));
    napi_value arr;
    NAPI_OK(env, napi_create_array_with_length(env, 4, &arr));
    for (uint32_t i = 0; i < 4; i++) {
        napi_value e;
        NAPI_OK(env, napi_create_int32(env, v[i], &e));
        NAPI_OK(env, napi_set_element(env, arr, i, e));
    }
    return arr;
}

static napi_value js_comm_destroy(napi_env env, napi_callback_info info)
{
    ARGS(1)
    crt_ctx *ctx = get_ctx(env, argv[0]);
    if (!ctx) return NULL;
    CRT_CHECK(env, ctx, "crt_comm_destroy", crt_comm_destroy(ctx));
    return undefined(env);
}

static napi_value js_gather(napi_env env, napi_callback_info info)
{
    ARGS(2)
    crt_ctx *ctx = get_ctx(env, argv[0]);
    if (!ctx) return NULL;
    int32_t what;
    NAPI_OK(env, napi_get_value_int32(env, argv[1], &what));
    CRT_CHECK(env, ctx, "crt_gather", crt_gather(ctx, what));
    return undefined(env);
}

static napi_value read_frame(napi_env env, napi_callback_info info, int rgba)
{
    ARGS(1)
    crt_ctx *ctx = get_ctx(env, argv[0]);
    if (!ctx) return NULL;
    uint32_t wh[2];
    CRT_CHECK(env, ctx, "crt_image_size", crt_image_size(ctx, wh));
    size_t px = (size_t)wh[0] * wh[1];
    void *data = NULL;
    napi_value ab, ta;
    NAPI_OK(env, napi_create_arraybuffer(env, px * (rgba ? 4 : 16), &data, &ab));
    if (rgba) CRT_CHECK(env, ctx, "crt_read_frame_rgba8", crt_read_frame_rgba8(ctx, (uint8_t *)data));
    else CRT_CHECK(env, ctx, "crt_read_frame_accum", crt_read_frame_accum(ctx, (float *)data));
    NAPI_OK(env, napi_create_typedarray(env, rgba ? napi_uint8_array : napi_float32_array, px * 4, ab, 0, &ta));
    return ta;
}
static napi_value js_read_frame_rgba8(napi_env env, napi_callback_info info) { return read_frame(env, info, 1); }
static napi_value js_read_frame_accum(napi_env env, napi_callback_info info) { return read_frame(env, info, 0); }

static napi_value js_image_size(napi_env env, napi_callback_info info)
{
    ARGS(1)
    crt_ctx *ctx = get_ctx(env, argv[0]);
    if (!ctx) return NULL;
    uint32_t wh[2];
    CRT_CHECK(env, ctx, "crt_image_size", crt_image_size(ctx, wh));
    napi_value arr, a, b;
    NAPI_OK(env, napi_create_array_with_length(env, 2, &arr));
    NAPI_OK(env, napi_create_uint32(env, wh[0], &a));
    NAPI_OK(env, napi_create_uint32(env, wh[1], &b));
    NAPI_OK(env, napi_set_element(env, arr, 0, a));
    NAPI_OK(env, napi_set_element(env, arr, 1, b));
    return arr;
}

static napi_value js_set_row_bands(napi_env env, napi_callback_info info)
{
    ARGS(4)
    crt_ctx *ctx = get_ctx(env, argv[0]);
    if (!ctx) return NULL;
    uint32_t v[3];
    for (int i = 0; i < 3; i++) NAPI_OK(env, napi_get_value_uint32(env, argv[i + 1], &v[i]));
    CRT_CHECK(env, ctx, "crt_set_row_bands", crt_set_row_bands(ctx, v[0], v[1], v[2]));
    return undefined(env);
}

/* Device addresses cross the boundary as BigInt (or a Number / null for "none"). */
static int get_ptr(napi_env env, napi_value v, void **out)
{
    napi_valuetype t;
    *out = NULL;
    if (napi_typeof(env, v, &t) != napi_ok) return 0;
    if (t == napi_null || t == napi_undefined) return 1;
    if (t == napi_bigint) { uint64_t u; bool lossless; if (napi_get_value_bigint_uint64(env, v, &u, &lossless) != napi_ok) return 0; *out = (void *)(uintptr_t)u; return 1; }
    if (t == napi_number) { int64_t i; if (napi_get_value_int64(env, v, &i) != napi_ok || i < 0) return 0; *out = (void *)(uintptr_t)i; return 1; }
    return 0;
}

static napi_value ptr_pair(napi_env env, void *a, void *b)
{
    napi_value arr, x, y;
    NAPI_OK(env, napi_create_array_with_length(env, 2, &arr));
    NAPI_OK(env, napi_create_bigint_uint64(env, (uint64_t)(uintptr_t)a, &x));
    NAPI_OK(env, napi_create_bigint_uint64(env, (uint64_t)(uintptr_t)b, &y));
    NAPI_OK(env, napi_set_element(env, arr, 0, x));
    NAPI_OK(env, napi_set_element(env, arr, 1, y));
    return arr;
}

static napi_value js_device_buffers(napi_env env, napi_callback_info info)
{
    ARGS(1)
    crt_ctx *ctx = get_ctx(env, argv[0]);
    if (!ctx) return NULL;
    void *a = NULL, *b = NULL;
    CRT_CHECK(env, ctx, "crt_device_buffers", crt_device_buffers(ctx, &a, &b));
    return ptr_pair(env, a, b);
}

static napi_value js_frame_device_buffers(napi_env env, napi_callback_info info)
{
    ARGS(1)
    crt_ctx *ctx = get_ctx(env, argv[0]);
    if (!ctx) return NULL;
    void *a = NULL, *b = NULL;
    CRT_CHECK(env, ctx, "crt_frame_device_buffers", crt_frame_device_buffers(ctx, &a, &b));
    return ptr_pair(env, a, b);
}

static napi_value js_bind_output(napi_env env, napi_callback_info info)
{
    ARGS(3)
    crt_ctx *ctx = get_ctx(env, argv[0]);
    if (!ctx) return NULL;
    void *a, *b;
    if (!get_ptr(env, argv[1], &a) || !get_ptr(env, argv[2], &b)) { napi_throw_type_error(env, NULL, "bindOutput: device addresses are BigInt (or null)"); return NULL; }
    CRT_CHECK(env, ctx, "crt_bind_output", crt_bind_output(ctx, a, b));
    return undefined(env);
}

static napi_value js_set_stream(napi_env env, napi_callback_info info)
{
    ARGS(2)
    crt_ctx *ctx = get_ctx(env, argv[0]);
    if (!ctx) return NULL;
    void *st;
    if (!get_ptr(env, argv[1], &st)) { napi_throw_type_error(env, NULL, "setStream: a hipStream_t as BigInt (or null for the context's own)"); return NULL; }
    CRT_CHECK(env, ctx, "crt_set_stream", crt_set_stream(ctx, st));
    return undefined(env);
}

/* ------------------------------------------------------------------ asynchronous entry points
 * traceAsync(h, n), syncAsync(h), readRgba8Async(h), readAccumAsync(h) -> Promise.  The reference's frame() is
 * fire-and-forget (queue.submit, src/main.js:618-620): a Node display loop must not block its event loop on the
 * GPU either.  Jobs of one context run in call order. */
enum { JOB_TRACE, JOB_SYNC, JOB_READ_RGBA8, JOB_READ_ACCUM, JOB_GATHER, JOB_READ_FRAME_RGBA8, JOB_READ_FRAME_ACCUM, JOB_READ_SAMPLE_RGBA8,
       JOB_DENOISE_ADAPTIVE, JOB_DENOISE_TEMPORAL, JOB_DENOISE_SVGF, JOB_TRANSFORM_PRIMITIVES, JOB_READ_PRIMITIVES,
       JOB_DENOISE_FRAME, JOB_DENOISE_ADAPTIVE_FRAME, JOB_REMOVE_PRIMITIVES, JOB_APPEND_PRIMITIVES, JOB_DENOISE_LATEST };
typedef struct job {
    napi_async_work work;
    napi_deferred deferred;
    slot *sl;
    int op, rc;
    uint32_t n, px;
    crt_denoise_adaptive_params dn;     /* JOB_DENOISE_ADAPTIVE, JOB_DENOISE_ADAPTIVE_FRAME */
    crt_denoise_params df;              /* JOB_DENOISE_FRAME, JOB_DENOISE_LATEST */
    uint32_t sample;                    /* JOB_DENOISE_LATEST: the index of the frame shown */
    void *rgb;                          /* ... and with rgb: true the linear rgb's ArrayBuffer memory (kept alive by rgb_ref) */
    napi_ref rgb_ref;
    crt_denoise_temporal_params dt;     /* JOB_DENOISE_TEMPORAL */
    crt_denoise_svgf_params ds;         /* JOB_DENOISE_SVGF */
    crt_prim_transform *ops;            /* JOB_TRANSFORM_PRIMITIVES: the job's own copy of the n ops */
    uint32_t first;                     /* JOB_READ_PRIMITIVES: records [first, first + n) */
    void *edit, *lights;                /* JOB_REMOVE_PRIMITIVES / JOB_APPEND_PRIMITIVES: the job's own copies of the n ranges / records */
    size_t nlight;                      /* ... and of the light list (lights NULL: kept) */
    void *data;              /* ArrayBuffer memory of a read job (kept alive by ab_ref) */
    napi_ref ab_ref;
    char err[640];
    struct job *next;
} job;

static void job_execute(napi_env env, void *data)
{
    (void)env;
    job *j = (job *)data;
    crt_ctx *ctx = j->sl->ctx;
    switch (j->op) {
    case JOB_TRACE: j->rc = crt_trace(ctx, j->n); break;
    case JOB_SYNC: j->rc = crt_sync(ctx); break;
    case JOB_READ_RGBA8: j->rc = crt_read_rgba8(ctx, (uint8_t *)j->data); break;
    case JOB_READ_ACCUM: j->rc = crt_read_accum(ctx, (float *)j->data); break;
    case JOB_GATHER: j->rc = crt_gather(ctx, (int)j->n); break;
    case JOB_READ_FRAME_RGBA8: j->rc = crt_read_frame_rgba8(ctx, (uint8_t *)j->data); break;
    case JOB_READ_SAMPLE_RGBA8: j->rc = crt_read_sample_rgba8(ctx, j->n, (uint8_t *)j->data); break;
    case JOB_DENOISE_ADAPTIVE: j->rc = crt_denoise_adaptive(ctx, &j->dn, NULL, (uint8_t *)j->data, NULL); break;
    case JOB_DENOISE_FRAME: j->rc = crt_denoise_frame(ctx, &j->df, NULL, (uint8_t *)j->data); break;
    case JOB_DENOISE_LATEST: j->rc = crt_denoise_latest(ctx, &j->df, (float *)j->rgb, (uint8_t *)j->data, &j->sample); break;
    case JOB_DENOISE_ADAPTIVE_FRAME: j->rc = crt_denoise_adaptive_frame(ctx, &j->dn, NULL, (uint8_t *)j->data, NULL); break;
    case JOB_DENOISE_TEMPORAL: j->rc = crt_denoise_temporal(ctx, &j->dt, NULL, (uint8_t *)j->data, NULL); break;
    case JOB_DENOISE_SVGF: j->rc = crt_denoise_svgf(ctx, &j->ds, NULL, (uint8_t *)j->data, NULL, NULL); break;
    case JOB_TRANSFORM_PRIMITIVES: j->rc = crt_transform_primitives(ctx, j->ops, j->n); break;
    case JOB_REMOVE_PRIMITIVES: j->rc = crt_remove_primitives(ctx, (const crt_prim_range *)j->edit, j->n, j->lights, j->nlight); break;
    case JOB_APPEND_PRIMITIVES: j->rc = crt_append_primitives(ctx, j->edit, j->n, j->lights, j->nlight); break;
    case JOB_READ_PRIMITIVES: j->rc = crt_read_primitives(ctx, j->first, j->n, j->n ? j->data : NULL); break;
    default: j->rc = crt_read_frame_accum(ctx, (float *)j->data); break;
    }
    if (j->rc != CRT_OK) {
        const char *d = crt_last_error(ctx);
        snprintf(j->err, sizeof j->err, "asynchronous call failed (%d): %s", j->rc, d ? d : "");
    }
}

static void job_complete(napi_env env, napi_status status, void *data)
{
    job *j = (job *)data;
    slot *sl = j->sl;
    napi_value result = NULL;
    if (status != napi_ok && j->rc == CRT_OK) { j->rc = CRT_EDEVICE; snprintf(j->err, sizeof j->err, "asynchronous call cancelled"); }
    if (j->rc == CRT_OK) {
        if (j->ab_ref) {
            napi_value ab;
            const int bytes8 = j->op == JOB_READ_RGBA8 || j->op == JOB_READ_FRAME_RGBA8 || j->op == JOB_READ_SAMPLE_RGBA8 ||
                               j->op == JOB_DENOISE_ADAPTIVE || j->op == JOB_DENOISE_TEMPORAL || j->op == JOB_DENOISE_SVGF ||
                               j->op == JOB_DENOISE_FRAME || j->op == JOB_DENOISE_ADAPTIVE_FRAME;
            if (napi_get_reference_value(env, j->ab_ref, &ab) == napi_ok) {
                napi_value rgb_ab = NULL;
                if (j->op == JOB_DENOISE_LATEST) {
                    if (!j->rgb_ref || napi_get_reference_value(env, j->rgb_ref, &rgb_ab) == napi_ok)
                        result = denoise_latest_result(env, j->px, ab, rgb_ab, j->sample);
                }
                else if (j->op == JOB_READ_PRIMITIVES) napi_create_typedarray(env, napi_uint8_array, (size_t)j->n * 80, ab, 0, &result);
                else napi_create_typedarray(env, bytes8 ? napi_uint8_array : napi_float32_array, (size_t)j->px * 4, ab, 0, &result);
            }
        }
        if (!result) napi_get_undefined(env, &result);
        napi_resolve_deferred(env, j->deferred, result);
    } else {
        napi_value msg, code, errv;
        napi_create_string_utf8(env, j->err, NAPI_AUTO_LENGTH, &msg);
        napi_create_string_utf8(env, "ERR_CRT", NAPI_AUTO_LENGTH, &code);
        napi_create_error(env, code, msg, &errv);
        napi_reject_deferred(env, j->deferred, errv);
    }
    if (j->ab_ref) napi_delete_reference(env, j->ab_ref);
    if (j->rgb_ref) napi_delete_reference(env, j->rgb_ref);
    napi_delete_async_work(env, j->work);
    free(j->ops); free(j->edit); free(j->lights);
    /* the next job of this context */
    sl->head = j->next;
    if (!sl->head) {
        sl->tail = NULL;
        if (sl->self) { napi_ref r = sl->self; sl->self = NULL; napi_delete_reference(env, r); }   /* the handle may go now */
    } else napi_queue_async_work(env, sl->head->work);
    free(j);
}

static napi_value start_job(napi_env env, napi_callback_info info, int op)
{
    size_t argc = 3;
    napi_value argv[3];
    NAPI_OK(env, napi_get_cb_info(env, info, &argc, argv, NULL, NULL));
    if (argc < (op == JOB_READ_PRIMITIVES ? 3u : (op == JOB_TRACE || op == JOB_GATHER || op == JOB_READ_SAMPLE_RGBA8 || op == JOB_TRANSFORM_PRIMITIVES || op == JOB_REMOVE_PRIMITIVES || op == JOB_APPEND_PRIMITIVES) ? 2u : 1u)) { napi_throw_type_error(env, NULL, "too few arguments"); return NULL; }
    slot *sl = get_slot(env, argv[0]);
    if (!sl) return NULL;
    job *j = (job *)calloc(1, sizeof *j);
    j->sl = sl; j->op = op;
    if (op == JOB_DENOISE_FRAME && !denoise_plain_options(env, "denoiseFrameAsync", argc > 1 ? argv[1] : NULL, argc > 1, &j->df)) { free(j); return NULL; }
    bool latest_rgb = false;
    if (op == JOB_DENOISE_LATEST && !denoise_latest_options(env, "denoiseLatestAsync", argc > 1 ? argv[1] : NULL, argc > 1, &j->df, &latest_rgb)) { free(j); return NULL; }
    if ((op == JOB_DENOISE_ADAPTIVE || op == JOB_DENOISE_ADAPTIVE_FRAME) && !denoise_adaptive_options(env, "denoiseAdaptive", argc > 1 ? argv[1] : NULL, argc > 1, &j->dn, NULL)) { free(j); return NULL; }
    if (op == JOB_DENOISE_TEMPORAL && !denoise_temporal_options(env, argc > 1 ? argv[1] : NULL, argc > 1, &j->dt, NULL)) { free(j); return NULL; }
    if (op == JOB_DENOISE_SVGF && !denoise_svgf_options(env, argc > 1 ? argv[1] : NULL, argc > 1, &j->ds, NULL, NULL)) { free(j); return NULL; }
    if (op == JOB_TRACE || op == JOB_GATHER || op == JOB_READ_SAMPLE_RGBA8) {
        if (napi_get_value_uint32(env, argv[1], &j->n) != napi_ok) { free(j); napi_throw_type_error(env, NULL, "traceAsync / gatherAsync: a number expected"); return NULL; }
    }
    if (op == JOB_TRANSFORM_PRIMITIVES) {                        /* the caller may change its buffer before the job runs */
        void *p = NULL; size_t n = 0;
        if (!get_bytes(env, argv[1], &p, &n) || n % sizeof(crt_prim_transform)) { free(j); napi_throw_type_error(env, NULL, "transformPrimitivesAsync: ops must be k*60 bytes"); return NULL; }
        j->n = (uint32_t)(n / sizeof(crt_prim_transform));
        j->ops = (crt_prim_transform *)malloc(n ? n : 1);
        if (!j->ops) { free(j); napi_throw_error(env, NULL, "out of memory"); return NULL; }
        memcpy(j->ops, p, n);
    }
    if (op == JOB_REMOVE_PRIMITIVES || op == JOB_APPEND_PRIMITIVES) {   /* copies, as for the ops above */
        const size_t unit = op == JOB_APPEND_PRIMITIVES ? 80 : sizeof(crt_prim_range);
        void *p = NULL, *lp = NULL; size_t n = 0, ln = 0;
        if (!get_bytes(env, argv[1], &p, &n) || n % unit || !optional_lights(env, argc, argv, &lp, &ln)) {
            free(j);
            napi_throw_type_error(env, NULL, "removePrimitivesAsync / appendPrimitivesAsync: k*8 bytes of ranges / k*80 bytes of records, then lights (m*80 bytes) or null");
            return NULL;
        }
        j->n = (uint32_t)(n / unit);
        j->nlight = ln / 80;
        j->edit = malloc(n ? n : 1);
        j->lights = lp ? malloc(ln ? ln : 1) : NULL;
        if (!j->edit || (lp && !j->lights)) { free(j->edit); free(j->lights); free(j); napi_throw_error(env, NULL, "out of memory"); return NULL; }
        memcpy(j->edit, p, n);
        if (lp) memcpy(j->lights, lp, ln);
    }
    if (op == JOB_READ_PRIMITIVES) {
        napi_value ab;
        if (napi_get_value_uint32(env, argv[1], &j->first) != napi_ok || napi_get_value_uint32(env, argv[2], &j->n) != napi_ok) { free(j); napi_throw_type_error(env, NULL, "readPrimitivesAsync: first and count are numbers"); return NULL; }
        if (napi_create_arraybuffer(env, (size_t)j->n * 80, &j->data, &ab) != napi_ok ||
            napi_create_reference(env, ab, 1, &j->ab_ref) != napi_ok) { free(j); napi_throw_error(env, NULL, "out of memory"); return NULL; }
    }
    if (op == JOB_READ_RGBA8 || op == JOB_READ_ACCUM || op == JOB_READ_FRAME_RGBA8 || op == JOB_READ_FRAME_ACCUM || op == JOB_READ_SAMPLE_RGBA8 ||
        op == JOB_DENOISE_ADAPTIVE || op == JOB_DENOISE_TEMPORAL || op == JOB_DENOISE_SVGF || op == JOB_DENOISE_FRAME || op == JOB_DENOISE_ADAPTIVE_FRAME ||
        op == JOB_DENOISE_LATEST) {
        const int frame = op == JOB_READ_FRAME_RGBA8 || op == JOB_READ_FRAME_ACCUM || op == JOB_DENOISE_FRAME || op == JOB_DENOISE_ADAPTIVE_FRAME;
        const int bytes8 = op != JOB_READ_ACCUM && op != JOB_READ_FRAME_ACCUM;
        uint32_t t[4];
        if (frame) { if (crt_image_size(sl->ctx, t + 2) != CRT_OK) { free(j); return throw_crt(env, sl->ctx, CRT_ESTATE, "crt_image_size"); } }
        else if (crt_tile(sl->ctx, t) != CRT_OK) { free(j); return throw_crt(env, sl->ctx, CRT_ESTATE, "crt_tile"); }
        j->px = t[2] * t[3];
        napi_value ab;
        if (napi_create_arraybuffer(env, (size_t)j->px * (bytes8 ? 4 : 16), &j->data, &ab) != napi_ok ||
            napi_create_reference(env, ab, 1, &j->ab_ref) != napi_ok) { free(j); napi_throw_error(env, NULL, "out of memory"); return NULL; }
        if (latest_rgb && (napi_create_arraybuffer(env, (size_t)j->px * 16, &j->rgb, &ab) != napi_ok ||
                           napi_create_reference(env, ab, 1, &j->rgb_ref) != napi_ok)) {
            napi_delete_reference(env, j->ab_ref);
            free(j);
            napi_throw_error(env, NULL, "out of memory");
            return NULL;
        }
    }
    napi_value promise, name;
    if (napi_create_promise(env, &j->deferred, &promise) != napi_ok ||
        napi_create_string_utf8(env, "crt_async", NAPI_AUTO_LENGTH, &name) != napi_ok ||
        napi_create_async_work(env, NULL, name, job_execute, job_complete, j, &j->work) != napi_ok) {
        if (j->ab_ref) napi_delete_reference(env, j->ab_ref);
        if (j->rgb_ref) napi_delete_reference(env, j->rgb_ref);
        free(j->ops); free(j->edit); free(j->lights);
        free(j);
        napi_throw_error(env, NULL, "crt_napi: could not create the asynchronous job");
        return NULL;
    }
    if (sl->tail) { sl->tail->next = j; sl->tail = j; }
    else {
        if (!sl->self && napi_create_reference(env, argv[0], 1, &sl->self) != napi_ok) {
            sl->self = NULL;
            napi_delete_async_work(env, j->work);
            if (j->ab_ref) napi_delete_reference(env, j->ab_ref);
            if (j->rgb_ref) napi_delete_reference(env, j->rgb_ref);
            free(j->ops); free(j->edit); free(j->lights);
            free(j);
            napi_throw_error(env, NULL, "crt_napi: could not pin the context handle");
            return NULL;
        }
        sl->head = sl->tail = j;
        napi_queue_async_work(env, j->work);
    }
    return promise;
}
static napi_value js_trace_async(napi_env env, napi_callback_info info) { return start_job(env, info, JOB_TRACE); }
static napi_value js_sync_async(napi_env env, napi_callback_info info) { return start_job(env, info, JOB_SYNC); }
static napi_value js_read_rgba8_async(napi_env env, napi_callback_info info) { return start_job(env, info, JOB_READ_RGBA8); }
static napi_value js_read_accum_async(napi_env env, napi_callback_info info) { return start_job(env, info, JOB_READ_ACCUM); }
static napi_value js_gather_async(napi_env env, napi_callback_info info) { return start_job(env, info, JOB_GATHER); }
static napi_value js_read_sample_rgba8_async(napi_env env, napi_callback_info info) { return start_job(env, info, JOB_READ_SAMPLE_RGBA8); }
static napi_value js_read_frame_rgba8_async(napi_env env, napi_callback_info info) { return start_job(env, info, JOB_READ_FRAME_RGBA8); }
static napi_value js_read_frame_accum_async(napi_env env, napi_callback_info info) { return start_job(env, info, JOB_READ_FRAME_ACCUM); }
static napi_value js_denoise_adaptive_async(napi_env env, napi_callback_info info) { return start_job(env, info, JOB_DENOISE_ADAPTIVE); }
static napi_value js_denoise_frame_async(napi_env env, napi_callback_info info) { return start_job(env, info, JOB_DENOISE_FRAME); }
static napi_value js_denoise_latest_async(napi_env env, napi_callback_info info) { return start_job(env, info, JOB_DENOISE_LATEST); }
static napi_value js_denoise_adaptive_frame_async(napi_env env, napi_callback_info info) { return start_job(env, info, JOB_DENOISE_ADAPTIVE_FRAME); }
static napi_value js_denoise_temporal_async(napi_env env, napi_callback_info info) { return start_job(env, info, JOB_DENOISE_TEMPORAL); }
static napi_value js_denoise_svgf_async(napi_env env, napi_callback_info info) { return start_job(env, info, JOB_DENOISE_SVGF); }
static napi_value js_transform_primitives_async(napi_env env, napi_callback_info info) { return start_job(env, info, JOB_TRANSFORM_PRIMITIVES); }
static napi_value js_read_primitives_async(napi_env env, napi_callback_info info) { return start_job(env, info, JOB_READ_PRIMITIVES); }
static napi_value js_remove_primitives_async(napi_env env, napi_callback_info info) { return start_job(env, info, JOB_REMOVE_PRIMITIVES); }
static napi_value js_append_primitives_async(napi_env env, napi_callback_info info) { return start_job(env, info, JOB_APPEND_PRIMITIVES); }

static napi_value js_abi_version(napi_env env, napi_callback_info info)
{
    (void)info;
    napi_value v;
    NAPI_OK(env, napi_create_int32(env, crt_abi_version(), &v));
    return v;
}

static napi_value init(napi_env env, napi_value exports)
{
    static const struct { const char *name; napi_callback fn; } fns[] = {
        {"create", js_create}, {"destroy", js_destroy}, {"uploadScene", js_upload_scene},
        {"setTile", js_set_tile}, {"buildAccel", js_build_accel}, {"reset", js_reset},
        {"trace", js_trace}, {"sync", js_sync}, {"sampleCount", js_sample_count}, {"tile", js_tile},
        {"readAccum", js_read_accum}, {"readRgba8", js_read_rgba8}, {"writeAccum", js_write_accum},
        {"enableCounters", js_enable_counters}, {"resetCounters", js_reset_counters},
        {"counters", js_counters}, {"accelStats", js_accel_stats}, {"accelQuality", js_accel_quality}, {"lastTraceMs", js_last_trace_ms},
        {"setOption", js_set_option}, {"abiVersion", js_abi_version},
        {"traceAsync", js_trace_async}, {"syncAsync", js_sync_async},
        {"readRgba8Async", js_read_rgba8_async}, {"readAccumAsync", js_read_accum_async},
        {"readLatestRgba8", js_read_latest_rgba8}, {"latestSample", js_latest_sample}, {"readSampleRgba8", js_read_sample_rgba8},
        {"readSampleRgba8Async", js_read_sample_rgba8_async}, {"readSampleRgba8Into", js_read_sample_rgba8_into},
        {"pinHost", js_pin_host}, {"unpinHost", js_unpin_host},
        {"commUniqueId", js_comm_unique_id}, {"commInit", js_comm_init}, {"commPartition", js_comm_partition},
        {"commInfo", js_comm_info}, {"commDestroy", js_comm_destroy}, {"gather", js_gather},
        {"readFrameRgba8", js_read_frame_rgba8}, {"readFrameAccum", js_read_frame_accum}, {"imageSize", js_image_size},
        {"setRowBands", js_set_row_bands}, {"deviceBuffers", js_device_buffers}, {"frameDeviceBuffers", js_frame_device_buffers},
        {"bindOutput", js_bind_output}, {"setStream", js_set_stream},
        {"denoise", js_denoise}, {"denoiseLatest", js_denoise_latest}, {"denoiseLatestInto", js_denoise_latest_into},
        {"denoiseLatestAsync", js_denoise_latest_async},
        {"readGbuffer", js_read_gbuffer}, {"readMotion", js_read_motion}, {"renderAovs", js_render_aovs},
        {"renderMattes", js_render_mattes}, {"setPrimitiveIds", js_set_primitive_ids},
        {"queryRays", js_query_rays}, {"pick", js_pick}, {"radianceRays", js_radiance_rays},
        {"setCamera", js_set_camera}, {"updatePrimitives", js_update_primitives}, {"updateLights", js_update_lights},
        {"refitAccel", js_refit_accel},
        {"transformPrimitives", js_transform_primitives}, {"transformPrimitivesAsync", js_transform_primitives_async},
        {"readPrimitives", js_read_primitives}, {"readPrimitivesAsync", js_read_primitives_async},
        {"removePrimitives", js_remove_primitives}, {"removePrimitivesAsync", js_remove_primitives_async},
        {"appendPrimitives", js_append_primitives}, {"appendPrimitivesAsync", js_append_primitives_async},
        {"traceAdaptive", js_trace_adaptive}, {"readAdaptive", js_read_adaptive},
        {"traceAdaptiveFiltered", js_trace_adaptive_filtered}, {"readAdaptiveFiltered", js_read_adaptive_filtered},
        {"denoiseAdaptive", js_denoise_adaptive}, {"denoiseAdaptiveAsync", js_denoise_adaptive_async},
        {"setSampleOffset", js_set_sample_offset}, {"sampleOffset", js_sample_offset}, {"temporalReset", js_temporal_reset},
        {"denoiseTemporal", js_denoise_temporal}, {"denoiseTemporalAsync", js_denoise_temporal_async},
        {"denoiseSvgfDefaults", js_denoise_svgf_defaults}, {"denoiseSvgf", js_denoise_svgf}, {"denoiseSvgfAsync", js_denoise_svgf_async},
        {"readMoments", js_read_moments},
        {"debugReadClipBox", js_debug_read_clip_box},
        {"readFrameAdaptive", js_read_frame_adaptive}, {"denoiseFrame", js_denoise_frame}, {"denoiseFrameAsync", js_denoise_frame_async},
        {"denoiseAdaptiveFrame", js_denoise_adaptive_frame}, {"denoiseAdaptiveFrameAsync", js_denoise_adaptive_frame_async},
        {"gatherAsync", js_gather_async}, {"readFrameRgba8Async", js_read_frame_rgba8_async}, {"readFrameAccumAsync", js_read_frame_accum_async},
    };
    for (size_t i = 0; i < sizeof fns / sizeof fns[0]; i++) {
        napi_value f;
        if (napi_create_function(env, fns[i].name, NAPI_AUTO_LENGTH, fns[i].fn, NULL, &f) != napi_ok ||
            napi_set_named_property(env, exports, fns[i].name, f) != napi_ok) {
            napi_throw_error(env, NULL, "crt_napi: export failed");
            return NULL;
        }
    }
    return exports;
}

NAPI_MODULE(NODE_GYP_MODULE_NAME, init)
