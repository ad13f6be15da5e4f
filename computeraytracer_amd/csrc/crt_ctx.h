// crt_ctx.h -- the context behind include/crt.h and what every host unit needs of it: device resources that free
// themselves, the error path, and the few helpers the entry points share.  Internal: nothing here is part of the ABI.
//
// The host units:
//   crt_api.cpp         create / destroy, tile, reset, crt_trace, crt_sync, adaptive calls, reads / writes / binds, options
//   crt_scene.cpp       scene upload, tree build, scene edits and the refit
//   crt_wf_driver.cpp   the wavefront driver (decisions: crt_wf_policy.h)
//   crt_denoise_api.cpp the preview filters' entry points
//   crt_aov_api.cpp     the feature planes' entry points
//   crt_matte_api.cpp   the id mattes' entry points and the id table
//   crt_query_api.cpp   the ray queries' entry points
//   crt_radiance_api.cpp  the radiance queries' entry points
//   crt_debug.cpp       the debug read-outs
#pragma once
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cfloat>
#include <cmath>
#include <cstdarg>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <memory>
#include <string>
#include <utility>
#include <vector>

#include "../../include/crt.h"
#include "crt_bvh.h"
#include "crt_device.h"
#include "crt_launch.h"
#include "crt_math.h"
#include "crt_tile_class.h"
#include "crt_wf_policy.h"

namespace crt {

// Host copy of one 80-byte record (ComputeShader.wgsl:41-47, main.js:211-246).
struct HostPrim {
    uint32_t category;
    f3 d1, d2, d3;
    uint32_t emission, reflectance, material, index;
};

// Test hook (option "debug_fail_alloc" = k): the k-th device allocation from now on reports out-of-memory.
extern long long g_fail_alloc_in;

// A device buffer; it goes with its owner (a context, a scope).
template <typename T>
struct DevBuf {
    T *p = nullptr;
    size_t n = 0;
    DevBuf() = default;
    DevBuf(DevBuf &&o) noexcept : p(o.p), n(o.n) { o.p = nullptr; o.n = 0; }
    DevBuf &operator=(DevBuf &&o) noexcept { std::swap(p, o.p); std::swap(n, o.n); return *this; }   // (o frees what this held)
    DevBuf(const DevBuf &) = delete;
    DevBuf &operator=(const DevBuf &) = delete;
    ~DevBuf() { release(); }
    hipError_t alloc(size_t count) {
        release();
        if (count == 0) return hipSuccess;
        const bool inject = g_fail_alloc_in > 0 && --g_fail_alloc_in == 0;
        const hipError_t e = inject ? hipErrorOutOfMemory : hipMalloc((void **)&p, count * sizeof(T));
        if (e != hipSuccess) { p = nullptr; return e; }   // n stays 0: a later "is it large enough" test re-allocates
        n = count;
        return hipSuccess;
    }
    void release() { if (p) (void)hipFree(p); p = nullptr; n = 0; }
};

// An event, a stream of our own, a block of pinned host memory: created on first use, destroyed with their owner.
struct Event {
    hipEvent_t e = nullptr;
    Event() = default;
    Event(Event &&o) noexcept : e(o.e) { o.e = nullptr; }
    Event(const Event &) = delete;
    Event &operator=(const Event &) = delete;
    ~Event() { if (e) (void)hipEventDestroy(e); }
    hipError_t create() { return hipEventCreate(&e); }                                      // (with timing)
    hipError_t create(unsigned flags) { return hipEventCreateWithFlags(&e, flags); }
    operator hipEvent_t() const { return e; }
};

struct Stream {
    hipStream_t s = nullptr;
    Stream() = default;
    Stream(const Stream &) = delete;
    Stream &operator=(const Stream &) = delete;
    ~Stream() { if (s) (void)hipStreamDestroy(s); }
    hipError_t create(unsigned flags) { return hipStreamCreateWithFlags(&s, flags); }
    hipError_t create(unsigned flags, int priority) { return hipStreamCreateWithPriority(&s, flags, priority); }
    void sync() const { if (s) (void)hipStreamSynchronize(s); }
    operator hipStream_t() const { return s; }
};

template <typename T>
struct Pinned {
    T *p = nullptr;
    Pinned() = default;
    Pinned(const Pinned &) = delete;
    Pinned &operator=(const Pinned &) = delete;
    ~Pinned() { if (p) (void)hipHostFree(p); }
    hipError_t alloc(size_t count, unsigned flags)              // zeroed
    {
        const hipError_t e = hipHostMalloc((void **)&p, count * sizeof(T), flags);
        if (e != hipSuccess) { p = nullptr; return e; }
        std::memset(p, 0, count * sizeof(T));
        return hipSuccess;
    }
    operator T *() const { return p; }
};

// The driver's state between calls (crt_wf_driver.cpp): its view of the pool, and per pipe the launch parameters
// and the stream they go to.
struct WfRun : WfView {
    WfParams W[kWfMaxPipes] = {};
    hipStream_t stream[kWfMaxPipes] = {};
    AsTiles as{};                   // adaptive pool (as.active set): the active tiles its batches sample
};

}  // namespace crt

struct crt_ctx {
    int device = 0;
    crt::Stream own_stream;
    hipStream_t stream = nullptr;   // own_stream, or the one adopted through crt_set_stream (not ours: never destroyed)
    crt::Event ev0, ev1;
    std::string err;

    // host copies
    std::vector<crt::HostPrim> prims;
    std::vector<crt::HostPrim> lights;
    float camera[16] = {0};
    uint32_t W = 0, H = 0;
    bool have_scene = false;
    int accel_mode = -1;            // -1: not built
    int want_builder = 0;           // the builder crt_build_accel asked for: 0 host binned SAH, 1 GPU LBVH (CRT_ACCEL_LBVH), 2 GPU PLOC (CRT_ACCEL_PLOC)
    int accel_builder = 0;          // the builder that made the current tree (same numbers)
    crt::PlocOptions ploc;          // options "ploc_radius", "debug_ploc_max_depth", "debug_ploc_max_rounds"
    crt::Bvh bvh;
    crt::Bvh4 bvh4;
    crt::Bvh4Q bvh4q;
    crt::Bvh8Q bvh8q;
    int quantize = 1;
    int wf_width = 4;               // node width of the wavefront traversal: 4 (64-byte quantised nodes), or 8 (128-byte; measured slower)
    uint32_t wf_depth = 0;          // inner levels of the tree the wavefront kernels walk (sizes their stacks' overflow area)

    template <typename T> using DevBuf = crt::DevBuf<T>;
    // device scene
    DevBuf<unsigned char> d_raw;    // the scene's 80-byte records as uploaded (input of the all-device LBVH build); n is its
                                    // capacity in bytes since crt_append_primitives: the records are prims.size() * 80
    DevBuf<float4> d_prim, d_primD, d_nodes, d_nodes4, d_lights;
    DevBuf<int> w_overflow;
    DevBuf<uint4> d_nodes4q, d_nodes8q;
    DevBuf<uint32_t> d_slot_of_index;
    DevBuf<float> d_spectra, d_cie;
    crt::DevScene sc{};

    // tile + outputs
    uint32_t x0 = 0, y0 = 0, tw = 0, th = 0;
    uint32_t band = 0x40000000u, stride = 1, phase = 0;   // row interleave (rectangular tile by default)
    DevBuf<float4> d_accum;
    DevBuf<uchar4> d_rgba;
    DevBuf<uchar4> d_frames;        // option "frame_ring" = F: the rgba8 frame of each of the last F samples (tile-sized each)
    uint32_t frame_ring = 0;
    std::vector<uint8_t> frame_batch;   // per ring slot: the batch id whose resolve pass wrote that frame (its ev_resolved orders a read)
    crt::Stream read_stream;        // readbacks from the ring: they wait for the frame's own resolve pass, not for the retirement work queued behind it
    uint32_t ring_from = 1;         // the ring holds frames of samples >= this (a restored accumulator brings no frames with it)
    uint32_t resolved_upto = 0;     // samples whose resolve pass has been enqueued on the context's stream (frames <= this are in the ring / the framebuffer in stream order)
    float4 *accum_bound = nullptr;
    uchar4 *rgba_bound = nullptr;
    uint32_t sample = 0;            // samples requested so far (ComputeShader.wgsl:3 after that many frames)
    uint32_t published = 0;         // ... of which this many have been turned into batches (or run by the single-kernel form)
    uint32_t pending = 0;           // ... and this many wait to be merged with the next calls' (sample == published + pending)
    bool in_publish = false;
    uint32_t sample_offset = 0;     // crt_set_sample_offset: sample j since the reset is drawn with the reference's index offset + j
    uint32_t frame_id = 0;          // events that zeroed the accumulator so far (zero_state): a frame of crt_denoise_temporal
    int wf_cohort = 16;             // small calls are merged into batches of at least this many samples (1 = every call its own batch)

    DevBuf<unsigned long long> d_counters;
    bool counting = false;
    float last_ms = 0.0f;
    uint32_t last_launches = 0;
    bool last_timed = false;
    uint32_t spp_per_launch = 0;    // 0 = auto

    // wavefront pipeline (crt_wavefront.hip)
    int pipeline = 1;               // 1 = wavefront (default), 0 = v1 megakernel
    uint32_t wf_pool = 0;           // 0 = auto
    uint32_t wf_waves_per_cu = 0;   // persistent traversal waves per CU and pipe; 0 = auto (wf_waves)
    int num_cu = 0;
    DevBuf<float4> w_ray_o, w_ray_d, w_sh_d, w_beta, w_radiance, w_nee, w_staging[crt::kWfRing], w_recA, w_recB;
    DevBuf<uint4> w_rng, w_misc, w_recC;
    DevBuf<float2> w_hit;
    DevBuf<uint32_t> w_vis, w_dead, w_tea;
    DevBuf<uint8_t> w_dflag;        // per slot: a deferred NEE entry waits in w_nee
    DevBuf<uint32_t> w_tile_cls;    // per 8x8 tile of the tile rectangle: 2 bits, what its camera rays' root step is for every sample
    static constexpr int kMaxPipes = crt::kWfMaxPipes;
    int wf_pipes = 2;
    int wf_defer = 1;               // 1: crt_trace returns with its batch in flight; its paths finish under the next batches (or at crt_sync)
    int wf_tail_walk = 1;           // shade walks the ray lists once few paths are left
    int wf_gen_blocks = 128;        // k_wf_gen: waves per shard (64 shards)
    int wf_trace_form = 2;          // traversal kernel: 2 = k_wf_trace2 (ray ring + primitive tasks), 1 = k_wf_trace
    int wf_cull_miss = 1;           // k_wf_gen decides whole work chunks whose camera rays all miss the tree's root boxes
    int wf_cull_classes = 1;        // ... and looks the tile's class up first: the tiles that miss or enter for every sample are classified once per run
    int wf_defer_nee = 1;           // k_wf_shade finishes a path roulette ends at once and defers its pending NEE term
    int wf_affinity = 0;            // 1: a batch's work shards are region-major and traversal waves stay with their XCD's region (measured, no gain)
    uint64_t mapped_gen_launches = 0;   // k_wf_gen launches that took a MAP instantiation so far (crt_debug_mapped_gen_launches)
    uint64_t tile_cls_setups = 0;   // run set-ups that launched k_wf_tile_classes so far (crt_debug_tile_class_setups)
    bool cie_zero = false;          // the uploaded CIE table turns zero radiance into +0 for every wavelength (tc_culled_is_zero)
    int wf_chunk = 1;               // iterations per status record at most
    int wf_ahead = 3;               // iterations in flight per pipe before the pump waits for a status
    int wf_ring = 32;               // batches in flight at most (2..kWfRing): bounds how many calls a bound output can lag
    int wf_pool_spp = 8;            // automatic pool size: at least this many path slots per tile pixel (within 1 M .. 24 M)
    double wf_feed = 1.0;           // pump: weight of the work the iterations in flight are expected to consume
    std::unique_ptr<crt::WfRun> run;   // pipeline state between calls
    uint32_t wf_finish_at = 32768;  // paths of the oldest batch left (per pipe) at which they move to the side pool; 0 = never
    uint32_t wf_flush_at = 4096;    // the same for the LAST batch at crt_sync (nothing to hide its tail under); 0 = never
    uint32_t wf_side_ppw = 64, wf_flush_ppw = 4;   // k_wf_finish: paths per wave, under the next batch / at crt_sync
    DevBuf<crt::WfCtl> w_ctl[kMaxPipes];
    DevBuf<crt::WfWorkQ> w_wq;
    crt::Pinned<crt::WfStatus> h_status[kMaxPipes];        // pinned host records [kStatusRing], written by k_wf_status ...
    crt::WfStatus *d_status[kMaxPipes] = {};               // ... through these device pointers
    crt::Event ev_status[kMaxPipes][crt::kStatusRing];
    crt::Event ev_done[kMaxPipes][crt::kStatusRing];       // after the traversal launch of that iteration
    crt::Pinned<uint32_t> h_dropped;                       // pinned [kMaxPipes]: WfCtl::dropped after the last flush
    bool wf_host_ready = false;                            // the streams / events / pinned buffers below exist
    crt::Stream pipe_stream[kMaxPipes];                    // the pipes' own streams (the context's stream sets up, finishes stragglers and resolves)
    crt::Stream pub_stream;                                // publishes a new batch's queue (waits only for what it must)
    static constexpr int kFinishStreams = 3;
    crt::Stream fin_stream[kFinishStreams];                // k_wf_finish launches (lowest priority; each lasts as long as its longest path,
    crt::Event ev_fin[kFinishStreams];                     //  so consecutive ones overlap); the resolve passes wait for these events
    int fin_next = 0;
    crt::Event ev_fork, ev_join[kMaxPipes], ev_pub_join[kMaxPipes];
    crt::Event ev_evict[kMaxPipes][crt::kWfRing];          // after the shade launch of that pipe that evicts that batch id
    crt::Event ev_resolved[crt::kWfRing];                  // after the resolve pass of the batch that used the id last
    crt::Event ev_pub[crt::kWfRing];                       // after the queue reset of the batch that uses the id now
    bool time_kernels = false;
    std::vector<crt::Event> kev;    // event pairs around k_wf_trace launches
    float last_trace_kernel_ms = 0.0f;
    uint32_t last_trace_kernel_launches = 0;
    uint32_t last_iterations = 0;
    unsigned long long probes[8] = {0};   // traversal-efficiency probes of the counting kernels

    // The preview filters (crt_denoise.hip).  DESIGN.md 6e has the model: guide sets in a pool, history slots that name
    // the set they were blended with.
    struct DnGuideSet {             // a first-hit G-buffer of the tile and its keys
        DevBuf<float4> gbuf;        // 2 per tile pixel: (t, position), (normal, hit index bits)
        DevBuf<uint32_t> key;       // per tile pixel: material << 24 | reflectance index, 0xFFFFFFFF = miss
    };
    struct DnSlot {                 // one frame of history (crt_denoise_temporal, crt_denoise_svgf)
        DevBuf<float4> c;           // blended linear rgb before any spatial filter, w = its weight Hw in samples
        DevBuf<float4> m;           // crt_denoise_svgf: (m1, s, Mw, 0), the temporal moments of the luminance
        int guides = -1;            // the set of `sets` this frame was blended with (-1: none, the slot is not valid)
        float cam[12] = {0};        // that frame's camera_frame
        uint32_t frame = 0;         // frame_id it was made in
        bool valid = false;
        bool has_m = false;         // m belongs to this slot (a crt_denoise_svgf wrote it)
        bool snap = false;          // `snap` below is the scene as THIS slot saw it (at most one slot says so)
        void clear() { guides = -1; valid = has_m = snap = false; }     // (the buffers stay for the next use)
    };
    struct Denoise {
        // the G-buffer of the tile is sets[set] while `valid`: built on first use, kept until the scene, the accel structure
        // or the tile changes.  A rebuild writes a set that no slot names, so a third one exists only once both slots hold
        // one of their own and a plain crt_denoise needs another.
        DnGuideSet sets[3];
        int set = 0;
        bool valid = false;
        DevBuf<float4> c[2];        // the filter's ping-pong colour buffers ...
        DevBuf<uchar4> rgba;        // ... and its rgba8 output
        DevBuf<uint2> kv;           // crt_denoise_adaptive: per tile pixel (key, blurred variance bits) of the current pass
        DevBuf<float> var;          // ... and the variance left after the last pass
        DnSlot cur, prev;           // CURRENT: the last temporal call of this frame; PREVIOUS: what it was blended with
        DevBuf<float> hist;         // Hw alone, for history_out
        // option "temporal_motion" (DESIGN.md 6f): the history outlives crt_update_primitives.  snap is a copy of d_raw, the
        // scene as the newest valid slot saw it, taken by the first update after that slot was written.  Like d_raw it
        // may be larger than the records; a removal or an append edits it as it edits d_raw.
        bool motion = false;
        DevBuf<unsigned char> snap;
        DevBuf<float2> uv;          // crt_read_motion's output
        // option "temporal_clip_pct" (DESIGN.md 6l): the blend clamps the reprojected history to the box of the frame's own
        // 7x7 neighbourhood, and the history outlives crt_update_lights.
        int clip_pct = 0;           // the option's value P (0 = off)
        DevBuf<float4> box;         // 2 per tile pixel: (lo, N), (hi, valid); allocated only with the option on
        bool box_ran = false;       // the temporal call that wrote CURRENT ran the box kernel (crt_debug_read_clip_box)
        bool relit = false;         // the history has outlived a light edit: setting the option back to 0 drops it

        // crt_denoise_latest: recorded on the context's stream behind the snapshot of the accumulator; the
        // passes on read_stream wait for it.  wave_blocks (option "denoise_latest_wave_blocks"): k_dn_atrous_w64 for them.
        crt::Event ev_snap;
        bool wave_blocks = false;

        // Drop the history (the geometry snapshot goes with it).
        void drop() { cur.clear(); prev.clear(); snap.release(); relit = box_ran = false; }
    } dn;

    // The frame-level filters of a partitioned context (crt_denoise_frame, crt_denoise_adaptive_frame, crt_read_frame_adaptive;
    // DESIGN.md 6h): W x H buffers of their own -- dn is tile-sized and belongs to the history slots.  No history here.
    struct FrameDenoise {
        DnGuideSet guides;          // the G-buffer of the whole frame while `valid`: kept until the scene, the tree, the
        bool valid = false;         // camera or the partition changes (dropped wherever dn.valid is)
        DevBuf<float4> c[2];
        DevBuf<uchar4> rgba;
        DevBuf<uint2> kv;
        DevBuf<float> var;
        DevBuf<float> errors;       // crt_read_frame_adaptive: E per tile of the frame's grid ...
        DevBuf<uint32_t> flags;     // ... and the flags the selection kernel writes beside it
    } fdn;

    // The feature planes (crt_aov.hip).
    std::vector<float> albedo;      // the albedo table: crt_spectrum_rgb of every spectra row, rebuilt by crt_upload_scene
    DevBuf<float> d_albedo;         // ... on the device: made by the first crt_render_aovs after the upload
    struct Aov {                    // the planes of the tile, each allocated by the first call that asks for it
        DevBuf<uint32_t> hits;
        DevBuf<float> alpha, depth;
        DevBuf<float4> normal, albedo;
    } aov;

    // The id mattes (crt_matte.hip).
    std::vector<uint32_t> prim_ids; // the id table, beside `prims`: one id per primitive, the identity after crt_upload_scene;
                                    // crt_set_primitive_ids replaces entries, the topology edits compact and extend it
    DevBuf<uint32_t> d_prim_ids;    // ... on the device: made by the first crt_render_mattes of source OBJECT that needs it,
                                    // dropped whenever the host table changes
    struct Matte {                  // the planes of the tile, each allocated by the first call that asks for it
        DevBuf<uint32_t> ids, counts, hits, overflow;
    } matte;

    // Ray queries (crt_query.hip): the host forms' stream and staging, made by the first call that needs
    // them; a buffer grows by at least half.  Released by crt_upload_scene; the device form uses none of this.
    struct Query {
        crt::Stream stream;         // non-blocking: a query waits for nothing the pipeline has enqueued
        DevBuf<float4> rays;        // 2 per ray (crt_ray)
        DevBuf<uint2> xy;           // crt_pick: the pixel coordinates
        DevBuf<uint32_t> hit, prim, id;
        DevBuf<float> t;
        DevBuf<float4> position, normal;
        DevBuf<float2> uv;
        // radiance queries (crt_radiance.hip): they share the stream and `rays`
        DevBuf<uint4> keys;         // crt_path_key
        DevBuf<float4> rad_xyz;
        DevBuf<float> rad_y2;
        DevBuf<uchar4> rad_rgba8;
        void release() { rays.release(); xy.release(); hit.release(); prim.release(); id.release(); t.release(); position.release();
                         normal.release(); uv.release(); keys.release(); rad_xyz.release(); rad_y2.release(); rad_rgba8.release(); }
    } query;

    // scene edits (crt_refit.hip)
    float s_prims = 0.0f;           // max |corner coordinate| of the primitives: hit_pad = max(s_prims, |eye|) * 2^-17
    float tree_pad = 0.0f;          // the hit_pad the tree's boxes were made with (a larger one needs a refit)
    bool accel_stale = false;       // primitives changed since the tree's boxes were made: crt_refit_accel / crt_build_accel
    bool accel_topo = false;        // ... and records were added or removed (crt_remove_primitives, crt_append_primitives): the tree's
                                    // arrays belong to another primitive list, and crt_refit_accel rebuilds
    bool rf_ready = false;          // the level lists below belong to the current tree
    DevBuf<int> rf_lv2, rf_lv4;     // inner nodes of the BVH2 / the 4-wide tree, level by level from the root ...
    std::vector<uint32_t> rf_off2, rf_off4;   // ... level l = list[off[l] .. off[l+1])
    DevBuf<uint32_t> rf_nch4, rf_cnt;         // children per 4-wide node; a counter
    DevBuf<float> rf_fb;            // float boxes of the quantised 4-wide tree (32 floats per node)
    bool prims_moved = false;       // crt_transform_primitives moved records on the device: the geometry of `prims` is out of date
                                    // (refresh_prims before anything reads it; category, material, spectra and index never are)
    DevBuf<uint32_t> xf_tab;        // one call's ops table: prefix sums of the counts, then the ops (kept between calls);
                                    // crt_remove_primitives: the gaps, then the prefix sums of the removed counts
    // tree cost (crt_quality.hip, crt_accel_quality)
    int refit_rebuild_pct = 0;      // option "refit_rebuild_pct": crt_refit_accel rebuilds once the walked tree's cost passes this share of q_built (0 = never)
    bool q_built_ok = false;        // q_built belongs to the current tree (taken before its first refit, or by the first crt_accel_quality)
    double q_built[4] = {0, 0, 0, 0};   // boxes2 prims2 boxes4 prims4 of the tree as it was built
    uint64_t refits = 0;            // refits since the tree was built
    uint64_t policy_rebuilds = 0;   // rebuilds "refit_rebuild_pct" has made since crt_create
    DevBuf<double2> q_part;         // one pair per block of the node kernels: the BVH2's, then the 4-wide tree's
    DevBuf<double> q_out;           // per tree 4 doubles: boxes, prims, A(root), -

    // adaptive sampling (crt_adaptive.hip): allocated by the first crt_trace_adaptive, released with the tile
    bool as_on = false;             // the adaptive state: per-tile counts instead of `sample` (left by everything that zeroes it)
    bool as_broken = false;         // a crt_trace_adaptive failed part way: the counts lag the accumulator until crt_reset
    bool adaptive_temporal = false; // option "adaptive_temporal" (DESIGN.md 6i): crt_trace_adaptive takes the sample offset, and the
                                    // temporal calls take the adaptive state with the tile's count as each pixel's n
    int svgf_spatial_pct = 0;       // option "svgf_spatial_pct" (DESIGN.md 6j): crt_denoise_svgf estimates the variance of pixels with
                                    // short history from their 7x7 neighbourhood, times this / 100 (0 = off: v = 1 there)
    unsigned long long as_requested = 0;   // samples the crt_trace_adaptive calls of this adaptive state have enqueued per
                                           // active tile: no tile's count is above it
    DevBuf<uint32_t> as_counts;     // per 8x8 tile: samples it holds
    DevBuf<float> as_errors;        // per tile: E as the selection judged it
    DevBuf<uint32_t> as_flags;      // per tile: active in the last selection
    DevBuf<uint32_t> as_active;     // the active tiles, ascending (what the sampling kernels run over)
    DevBuf<uint32_t> as_n;          // their number
    DevBuf<float> as_q;             // per tile pixel: sum of Y^2 over its samples
};

namespace crt {

// The error path: the message goes to the context (crt_last_error), or, without one, to crt_create's.
int fail(crt_ctx *c, int code, const char *fmt, ...);

#define HIPCHK(c, call)                                                                           \
    do {                                                                                          \
        hipError_t e_ = (call);                                                                   \
        if (e_ != hipSuccess)                                                                     \
            return fail(c, e_ == hipErrorOutOfMemory ? CRT_ENOMEM : CRT_EDEVICE, "%s: %s", #call, \
                        hipGetErrorString(e_));                                                   \
    } while (0)

// Return the code of a call of ours if it is one.
#define CRT_TRY(expr)                 \
    do {                              \
        const int rc_ = (expr);       \
        if (rc_) return rc_;          \
    } while (0)

// Grow a DevBuf to `count` elements (the refusal names the buffer).  After a failed allocation the buffer reports
// n == 0 and is retried by the next call.
#define CRT_ENSURE(c, buf, count)                              \
    do {                                                       \
        if (buf.n < (count)) HIPCHK(c, buf.alloc(count));      \
    } while (0)

inline float4 *accum_ptr(crt_ctx *c) { return c->accum_bound ? c->accum_bound : c->d_accum.p; }
inline uchar4 *rgba_ptr(crt_ctx *c) { return c->rgba_bound ? c->rgba_bound : c->d_rgba.p; }

// How most entry points open: the context's device, everything in flight finished (wf_flush) and, with `sync`, the
// context's stream idle.
int quiesce(crt_ctx *c, bool sync);

// crt_api.cpp
int alloc_tile(crt_ctx *c);
int zero_state(crt_ctx *c);
int as_refuse(crt_ctx *c, const char *what);
int as_refuse_broken(crt_ctx *c, const char *what);

// crt_scene.cpp
HostPrim read_prim(const uint8_t *base, size_t i);
float prims_scale(const std::vector<HostPrim> &prims);
float pad_of(float S, const float cam[16]);
void light_rows(const HostPrim &l, float4 out[3]);
void camera_frame(const float cam[16], float out[12]);
int build_tree(crt_ctx *c, int mode);
uint32_t wf_stack_need(const crt_ctx *c);
uint32_t wf_stack_lds(const crt_ctx *c);
uint32_t wf_overflow_levels(const crt_ctx *c);

// crt_denoise_api.cpp: what the filters' entry points (and the debug read-outs of their state) do first -- the checks, then
// the context's device and everything in flight finished; `values` must be positive and finite, `which` names them in
// the refusal -- and last.
// DN_TEMPORAL: the uniform state, or with option "adaptive_temporal" the adaptive one (the temporal calls).
enum DnState { DN_UNIFORM, DN_ADAPTIVE, DN_EITHER, DN_TEMPORAL };
int dn_begin(crt_ctx *c, const char *what, uint32_t iterations, const float *values, int count, const char *which, DnState state);
int dn_finish(crt_ctx *c, size_t n, const float4 *res, float *rgb_out, uint8_t *rgba8_out, const float *plane = nullptr,
              float *plane_out = nullptr);
// The adaptive filter for its two callers, crt_denoise_adaptive and the selection of crt_trace_adaptive_filtered (DESIGN.md
// 6k): its parameters checked (NULL = the defaults), the filters' refusals that do not depend on the frame state (row bands,
// ...; adaptive: the counts are per tile), and the filter itself on the context's stream with everything in flight finished;
// *var_dev = the plane of v' (with `var`).
int dn_adaptive_params(crt_ctx *c, const char *what, const crt_denoise_adaptive_params *params, crt_denoise_adaptive_params *out);
int dn_check_state(crt_ctx *c, const char *what, bool adaptive = false);
int dn_adaptive_run(crt_ctx *c, const crt_denoise_adaptive_params &dp, bool rgba, bool var, float4 **res, const float **var_dev);

// crt_aov_api.cpp: the albedo table of a new scene (crt_upload_scene)
void aov_rebuild_albedo(crt_ctx *c, const float *spectra, size_t nspectra, const float *cie);

// crt_matte_api.cpp: the id table of a new scene (crt_upload_scene: the identity) and under the topology edits.  All host
// only; each drops the device copy.  matte_ids_reserve is called before anything changes (it may throw std::bad_alloc).
void matte_ids_identity(crt_ctx *c);
void matte_ids_reserve(crt_ctx *c, size_t n_new);
void matte_ids_remove(crt_ctx *c, const crt_prim_range *live, size_t m);      // ascending, disjoint, non-empty ranges
void matte_ids_append(crt_ctx *c, uint32_t count);
int matte_ids_device(crt_ctx *c);   // the device copy, made if it is missing (an allocation and a blocking copy; else nothing)

// crt_wf_driver.cpp
struct AsBatch {                    // one batch of a crt_trace_adaptive call: its samples off + 1 .. off + n of every active tile
    uint32_t off;                   // samples of the call before this batch
    uint32_t n_active;              // tiles in the active list
    uint32_t commit;                // last batch of the call: the call's samples (committed to the counts after its resolve)
};
WfOptions wf_options(const crt_ctx *c);
int wf_ensure_overflow(crt_ctx *c);
int wf_flush(crt_ctx *c);
int wf_check_dropped(crt_ctx *c);
int wf_tick(crt_ctx *c);
int wf_publish_pending(crt_ctx *c, bool force);
int wf_trace_batch(crt_ctx *c, uint32_t n, const AsBatch *as = nullptr);
int wf_wait_sample(crt_ctx *c, uint32_t sample);
double wf_now_ms();
std::string wf_state(crt_ctx *c);

}  // namespace crt
