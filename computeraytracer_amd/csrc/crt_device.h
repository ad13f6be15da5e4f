// crt_device.h -- device-side scene layout and kernel parameters.
//
// HBM layout (all arrays 16-byte aligned, read-only during a trace):
//   prim   : 3 x float4 per primitive, in BVH leaf order ("slot" order), 48 B:
//              A = (data1.xyz, meta)        meta = cat | mat<<2 | emis<<4 | refl<<18
//              B = (data2.xyz, index bits)  sphere: (r, r*r, 0, index)
//              C = (data3.xyz, e2.e2)       (w used by patches only)
//   primD  : 1 x float4 per primitive: (unit normal of a patch, e1.e1); read for
//            category-0 records only (triangles and spheres never touch it)
//   nodes  : 4 x float4 per inner node, 64 B:
//              (c0.lo.xyz, c0.hi.x) (c0.hi.yz, c1.lo.xy) (c1.lo.z, c1.hi.xyz) (ref0, ref1, -, -)
//   slot_of_index : u32 per primitive (original position -> slot), used by the
//            reference-order loop (CRT_ACCEL_NONE and the NaN-ray fallback)
//   spectra, cie : the reference's tables, unchanged (f32[n][301], f32[3][471])
//   lights : 3 x float4 per light: (data1, emission bits) (data2, index bits) (data3, 1/area)
//   accum  : float4 per tile pixel (xyz + pad; the reference's 16-byte stride)
//   rgba8  : uchar4 per tile pixel
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "crt_work_map.h"

namespace crt {

constexpr uint32_t kNoHit = 0xFFFFFFFFu;
constexpr int kStackDepth = 64;     // single-ray BVH2 walk: the SAH builder stops at depth 30, a GPU LBVH can reach 62
constexpr uint32_t kWalk4q = 1u, kWalkFellBack = 2u;   // which single-ray walk ran (crt_shade.h finish_walk_*, crt_debug_walk_rays)
constexpr uint32_t kNLambda = 301;
constexpr uint32_t kNCie = 471;
constexpr int CRT_NCOUNTERS_DEV = 16;   // 8 public (crt_counters) + 8 traversal-efficiency probes

struct DevScene {
    const float4 *prim;
    const float4 *primD;
    const uint32_t *slot_of_index;
    const float4 *nodes;
    const float4 *nodes4;       // 8 x float4 per 4-wide node (128 B)
    const uint4 *nodes4q;       // 4 x uint4 per quantised 4-wide node (64 B), or null
    const uint4 *nodes8q;       // 8 x uint4 per quantised 8-wide node (128 B = one L2 line), or null
    const float *spectra;
    const float *cie;
    const float4 *lights;
    uint32_t nprim;
    uint32_t npatch;       // planar patches (category 0) in the scene: with none, nobody needs primD
    int32_t root;
    int32_t root4;
    int32_t root8;
    uint32_t n_nodes4;
    uint32_t nspectra;
    uint32_t nlight;
    float hit_pad;
    uint32_t nf_last[2];   // array positions of the last and the second-to-last patch / sphere (kNoHit: none): what the
                           // reference's loop returns for a ray with a NaN in its direction (crt_wavefront.hip, NEE)
    float inv_nlight;      // 1.0f / f32(nlight)
    uint32_t W, H;         // full image
    float qbase[3], qscale[3];  // plane = qbase + q * qscale (quantised nodes)
    float cam[12];         // llc, horizontal, vertical, eye  (ComputeShader.wgsl:470-487 hoisted)
};

struct TraceParams {
    DevScene sc;
    uint32_t x0, y0, tw, th;        // tile rectangle (local buffer is tw x th)
    uint32_t band, stride, phase;   // row interleave: global y = y0 + (ly/band)*band*stride + phase*band + ly%band
    uint32_t first_sample, n_samples;
    float4 *accum;
    uchar4 *rgba;
    unsigned long long *counters;   // CRT_NCOUNTERS, may be null
    uint32_t tiles_x, tiles_y;
};

// The active tiles of an adaptive call (crt_adaptive.hip), a kernel argument of its own for the adaptive
// instantiations of k_trace, k_wf_gen and k_wf_resolve (so that the uniform ones keep their parameter blocks).
struct AsTiles {
    const uint32_t *active;         // the active tiles, ascending
    const uint32_t *base;           // per tile: samples it held when the call began (its first sample is base + 1 + offset)
    float *q;                       // per tile pixel: sum of Y^2 over its samples
    uint32_t n_active;
};

// Adaptive sampling (crt_adaptive.hip): the tile selection's inputs and outputs.
struct AsParams {
    const float4 *accum;
    const float *q;                 // per tile pixel: sum of Y^2 over the pixel's samples
    const uint32_t *counts;         // per tile: samples it holds
    float *errors;                  // per tile: E
    uint32_t *flags;                // per tile: 1 = active
    uint32_t *active;               // the active tiles, ascending
    uint32_t *n_active;
    uint32_t tw, th, tiles_x, tiles_y;
    uint32_t min_samples, max_samples;
    float threshold;
};

// ... of crt_trace_adaptive_filtered: the tile's error from the variance the adaptive filter carried.
struct AsVarParams {
    const float *var;               // per tile pixel: v' after the filter's last pass (crt_denoise_adaptive's var_out)
    const uint32_t *counts;         // per tile: samples it holds
    float *errors;                  // per tile: E' = sqrt(max v')
    uint32_t *flags;                // per tile: 1 = active
    uint32_t tw, th, tiles_x, tiles_y;
    uint32_t min_samples, max_samples;
    float threshold;
};


// ---------------------------------------------------------------------------------------------
// Wavefront pipeline state (crt_wavefront.hip).  A pool of P path slots lives in HBM (SoA,
// one float4/uint4 per slot per array, so every access is a coalesced 16-byte stream):
//   ray_o   (o.xyz, exclude bits)         next extension ray of the slot
//   ray_d   (d.xyz, -)
//   sh_d    (light dir.xyz, t of the light's own primitive)   pending shadow ray
//   beta, radiance, nee                   path throughput, radiance, NEE term waiting for visibility
//   rng     uvec4 PCG state               (ComputeShader.wgsl:899)
//   misc    (work id, flags, last_bounce_pdf bits, etaScale bits); a fresh slot (kWfFresh): (work id, flags, sample, tea seed)
//   hit     (t, hit slot bits)            written by the trace kernel for extension rays
//   vis     in: light primitive index, out: 1 = light visible    (shadow rays)
//   dflag   one byte: a deferred NEE entry waits in nee[slot] (WfParams::dflag)
//   list[parity][class]                   slots with an active ray this iteration (ballot/popc compacted)
//   staging[b] (xyz, -) per (sample, pixel)  finished samples of the batch with id b, summed in sample order by k_wf_resolve
constexpr uint32_t kWfAlive = 1u, kWfDying = 2u, kWfShadow = 4u, kWfSpecular = 8u, kWfInTrans = 16u;
// The slot holds a camera ray k_wf_gen has started and nobody has shaded yet: misc = (work id, flags, sample, tea seed)
// and ray_o / ray_d / beta / rng hold nothing -- the shade step rebuilds the ray from those (camera_ray)
constexpr uint32_t kWfFresh = 32u;
constexpr uint32_t kWfNanRay = 1u << 31;   // the slot's (camera) ray is non-finite and has not been traced: the next shade step resolves it with the reference loop
constexpr uint32_t kWfHasRad = 1u << 30;   // radiance[slot] holds the path's radiance (else it is still zero: nothing was ever stored)
// ray-list entries: the slot, and on shadow-list entries a mark "this slot also listed an extension ray"
constexpr uint32_t kWfListSlot = 0x7FFFFFFFu, kWfListAlsoExt = 0x80000000u;
constexpr uint32_t kWfDepthShift = 8, kWfLambdaShift = 16;      // depth: 8 bits, lambda0: 9 bits
constexpr uint32_t kWfBatchShift = 25;                          // 5 bits: which of the (up to kWfRing) batches in flight the path belongs to
constexpr uint32_t kWfRing = 32;                                // batch ids cycle 0..ring-1 (ring <= kWfRing): queues, staging buffers, side pools are indexed by id
// Stragglers: once only a few paths of a batch are left (its queue is long empty, the pool is busy with the
// next batch), k_wf_shade moves them out of the pool into a small side pool, where k_wf_finish runs them to
// their end on another stream.  Side-pool slots precede the pool in the same arrays:
// [(id*pipes + pipe)*kWfSideCap, +kWfSideCap).
constexpr uint32_t kWfSideCap = 65536;
// Traversal stacks: kWfStackLds (k_wf_trace) / kWfStackLds2 (k_wf_trace2) entries per lane in LDS, the rest in a global
// overflow area of at least kWfOverflowLevels levels.  A nearest-first walk holds at most (node width - 1) entries per
// inner level of the walked tree; crt_scene.cpp sizes the area from that depth (wf_overflow_levels) and, where that would
// take more than kWfOverflowMaxLevels, builds the shallower tree instead.  The pushes themselves are unchecked.
constexpr int kWfStackLds = 32, kWfStackLds2 = 16;
constexpr uint32_t kWfOverflowLevels = 96, kWfOverflowMaxLevels = 384;

// Every queue counter is sharded kWfShards ways, one 128-byte line per shard: same-address
// returning atomics serialize at ~11 ns each on gfx950, which at one atomic per wave would
// cost more than the kernels themselves.  Shade block b appends to shard b % kWfShards of
// the ray lists; traversal waves and re-arming waves pick a non-empty shard with one
// wave-wide load + ballot.
constexpr uint32_t kWfShards = 64;
// rays listed by shade per class / fetch cursor of trace / slots still alive after the shade launch, per batch id
// n_dead: slots this shard's shade blocks found or left dead in the launch (k_wf_gen re-arms them by whole waves)
struct WfShard { uint32_t n[4], cur, n_dead, pad0[26], alive[kWfRing]; };
static_assert(sizeof(WfShard) == 256, "two lines per shard: the list counters and cursor, the per-batch counts");
struct WfWork { uint32_t cur, pad[31]; };                    // next work item of this shard's range
struct WfCtl {                       // device control block, one per context
    WfShard shard[4][kWfShards];     // ring-indexed by iteration & 3 (it-1 is read, it written, it+1 zeroed)
    unsigned long long counters[kWfShards][CRT_NCOUNTERS_DEV];   // sharded like everything the waves add to (a shard = one 128-byte line); the host sums
    uint32_t side_count[kWfRing];    // paths moved to the side pool, per batch id
    uint32_t dropped;                // paths a capacity guard had to leave behind (side pool full, bounce guard of
                                     // k_wf_finish): must stay 0 -- the host turns anything else into CRT_EDEVICE
    uint32_t max_sp[kWfShards];      // counting traversal kernels only: the deepest stack (entries) a lane of the shard's waves reached
    unsigned long long gen_culled[kWfShards];   // (pixel, sample) k_wf_gen decided without a slot (its CULL form), always counted: crt_debug_gen_culled
    unsigned long long deferred_nee[kWfShards]; // paths k_wf_shade finished at once with their NEE term deferred, always counted: crt_debug_deferred_nee
};
// The work queue is shared by the pipes of a context (two half-pools run on two streams so that
// one half's streaming shade pass overlaps the other half's latency-bound traversal).  There are kWfRing
// of them, one per batch id: the next batch's work is published while the current batch's queue
// still holds a few iterations' worth, so the pool never runs dry between batches.
struct WfWorkQ {
    WfWork work[kWfShards];
    uint32_t work_done;              // set once every work shard is exhausted (saves the scans)
    uint32_t work_per_shard;         // the queue's extent (k_wf_init copies WfSeg here for write_status)
    unsigned long long work_total;
    uint32_t map_samples, map_tiles; // WfSeg::map_samples and the frame's tiles: the shard sizes under "wf_affinity" (crt_work_map.h)
    uint32_t pad_[26];
};
static_assert(sizeof(WfWorkQ) == (kWfShards + 1) * 128, "whole lines");
// One batch's share of the parameters (indexed by batch id like the queues and the staging buffers).
struct WfSeg {
    unsigned long long work_total;   // n_samples * npix_padded
    uint32_t work_per_shard;         // work items per shard (multiple of 64)
    uint32_t first_sample;
    uint32_t map_samples;            // 0: shard s holds ids [s * work_per_shard, +work_per_shard); else the batch's samples, and the
    uint32_t pad_;                   // shards are region-major (option "wf_affinity", crt_work_map.h: sizes differ per shard)
};

// What the host needs to know about an iteration, reduced on the device (write_status in crt_wavefront.hip) into one
// small record in pinned host memory.
struct WfStatus {
    uint32_t it_end;                       // the status describes the state after iterations < it_end of this pipe
    uint32_t dropped;                      // WfCtl::dropped
    uint32_t bound;                        // largest number of rays one shard listed in the last iteration
    uint32_t pad_;
    unsigned long long rays;               // rays listed in the last iteration (= alive slots once the queues are dry)
    unsigned long long consumed[kWfRing];  // work items taken from that batch's queue so far (all pipes)
    uint32_t left[kWfRing];                // 1: that batch's queue still holds work
    uint32_t alive[kWfRing];               // paths of that batch alive in THIS pipe's pool after its last shade launch
};

// k_wf_finish runs the side-pool paths of several (batch, pipe) pairs in one launch: segment s = blocks
// [s * blocks_per_seg, (s + 1) * blocks_per_seg), paths side_base .. + min(side_count, kWfSideCap) of that pipe's control block.
constexpr uint32_t kWfFinishSegs = 32;
struct WfFinishSegs {
    struct WfCtl *ctl[kWfFinishSegs];
    uint32_t base[kWfFinishSegs], batch[kWfFinishSegs];
    uint32_t n, blocks_per_seg;
};

struct WfParams {
    DevScene sc;
    float4 *ray_o, *ray_d, *sh_d, *beta, *radiance, *nee;
    uint4 *rng, *misc;
    float2 *hit;
    uint32_t *vis;
    // The rays of an iteration as compacted records, [iteration parity][class: camera, bounce, shadow of camera hit, shadow],
    // entry i of a shard's list at [(parity*4 + class) * list_cap*kWfShards + shard*list_cap + i]:
    //   recA (o.xyz, exclude bits)   recB extension ray: (d.xyz, slot | kWfListAlsoExt if already resolved)
    //                                     shadow ray:    (light dir.xyz, t of the light's own primitive)
    //   recC shadow rays only: (slot | kWfListAlsoExt if the slot also listed an extension ray, light primitive index, its slot, -)
    // (the records ARE the ray lists: tail mode walks recB.w / recC.x of the previous iteration)
    float4 *recA, *recB;
    uint4 *recC;
    uint32_t *dead;                  // [shard * list_cap + i]: slots that are dead after this iteration's shade launch (k_wf_gen's input)
    uint32_t rearm;                  // k_wf_shade: list the dead slots (a k_wf_gen launch follows: some queue may hold work)
    uint32_t gen_blocks;             // k_wf_gen: blocks per shard (block j of a shard takes chunks j, j + gen_blocks, ... of its dead list)
    uint32_t cull_miss;              // k_wf_gen: option "wf_cull_miss" (wf_gen_culls: whether the launch takes the CULL form)
    float4 *staging[kWfRing];        // finished samples, per batch id (several batches can be in flight)
    uint32_t batch_id;           // id of the newest batch (k_wf_init: the batch being set up; k_wf_resolve / k_wf_finish: the batch to resolve / finish)
    WfStatus *status_out;            // k_wf_shade: where its first wave writes the PREVIOUS iteration's status record (pinned host memory), or null
    uint32_t count_alive;            // k_wf_shade: count the alive paths per batch id (WfShard::alive) -- needed once more than one batch is in flight
    uint32_t keep_pool;              // k_wf_init: leave the slots and list counters alone (paths of the batches before live on)
    uint32_t side_base[kWfRing];     // first side-pool slot of this pipe, per batch id
    uint32_t evict_mask;             // k_wf_shade: bit b = move the alive paths of batch id b to the side pool first
    WfCtl *ctl;
    WfWorkQ *wq;                     // [kWfRing], by batch id
    WfSeg seg[kWfRing];
    uint32_t seg_order[kWfRing];     // ids of the queues dead slots re-arm from, oldest first
    uint32_t seg_n;                  // how many of them
    uint32_t slot_base;              // this pipe's slots are [slot_base, slot_base + P)
    uint32_t reset_wq;               // k_wf_init also resets the work queue of batch_id
    uint32_t P;                      // slots of this pipe
    uint32_t x0, y0, tw, th;         // tile rectangle (local buffer is tw x th)
    uint32_t band, stride, phase;    // row interleave: global y = y0 + (ly/band)*band*stride + phase*band + ly%band
    uint32_t tiles_x, tiles_y;
    uint32_t npix_padded;            // tiles_x*tiles_y*64: work item = sample_off * npix_padded + tile*64 + lane
    uint32_t list_cap;               // list entries per shard
    uint32_t tail_bound;             // 0: one shade thread per slot; >0: tail mode, threads walk the previous
                                     //    iteration's ray lists (<= tail_bound entries per shard and list)
    uint32_t n_samples;              // k_wf_resolve: samples of the batch to resolve
    float4 *accum;
    uchar4 *rgba;
    uchar4 *frames;                  // k_wf_resolve: ring of `frame_ring` tile-sized rgba8 frames, frame of sample s at [(s - 1) % frame_ring], or null
    uint32_t frame_ring;
    const uint32_t *tea;             // per tile pixel: tea(px, py*100), the 16-round seed of the pixel's RNG (:98), computed once
    uint32_t count;                  // 1: maintain ctl->counters
    uint32_t trace_form;             // 2: k_wf_trace2 (ray ring + primitive tasks) where the tree is the quantised 4-wide one; else k_wf_trace
    int *stack_overflow;             // [level - LDS entries][global lane], for stacks deeper than the LDS part (wf_overflow_levels levels)
    uint32_t overflow_lanes;
    // DESIGN.md 5.9 (option "wf_cull_classes"): 2 bits per 8x8 tile, 16 tiles per word (crt_tile_class.h), written by
    // k_wf_tile_classes at run set-up and read-only during the run; null = k_wf_gen's CULL form tests every sample
    const uint32_t *tile_cls;
    uint32_t cls_miss_zero;          // a culled path's staging value is +0 for every wavelength (tc_culled_is_zero): MISS chunks store the constant
    // DESIGN.md 5.10 (option "wf_defer_nee"): a path that roulette ends with its NEE shadow ray pending finishes in that
    // shade step and frees its slot; what stays behind is a deferred entry -- nee[slot] = (the sample's XYZ WITH the term,
    // staging cell index) and dflag[slot] = kWfDeferred | batch id -- which the slot's thread of the pipe's NEXT shade
    // launch turns into a staging store iff vis[slot] == 1, whatever the slot holds by then.
    uint8_t *dflag;                  // one byte per slot, 0 = no entry
    uint32_t defer;                  // k_wf_shade: create such entries in this launch (the host: rearm && wf_defer_nee; I11 of crt_wf_driver.cpp)
    // DESIGN.md 5.11 (option "wf_affinity"): traversal waves start on a ray-list shard whose residue modulo 8 is their XCD's
    // id and prefer that residue when they move on; for speed only, every shard is drained whatever the ids say
    uint32_t affinity;
};
constexpr uint32_t kWfDeferred = 0x80u;                         // WfParams::dflag: an entry is pending; the low 5 bits are its batch id
static_assert(kWfRing <= 32u, "a deferred entry's batch id has 5 bits");
static_assert(sizeof(WfParams) + sizeof(WfFinishSegs) <= 4096u, "the kernels take WfParams by value: kernel arguments are 4 KiB at most");

// k_dn_reproject (crt_denoise.hip): the blend of a frame with the reprojected history of the previous one.
// The projection into the previous film plane is binary64 (binary32 places a tap no better than 5e-5 pixel at 480 pixels,
// and the history of neighbouring pixels differs by whole units); everything else is binary32.
struct DnReprojParams {
    double m[9];                    // rows of [hor' ver' (llc' - eye')]^-1 of the previous camera
    double eye_prev[3];
    double W, H, x0, y0;            // the full image's size and the rectangle's origin
    const float4 *accum;            // this frame: XYZ sums of n samples,
    const float4 *gbuf;             //   its G-buffer and keys
    const uint32_t *key;
    const float4 *h_prev;           // previous frame: blended linear rgb, w = its weight Hw in samples; null = no history
    const float4 *gbuf_prev;
    const uint32_t *key_prev;
    float4 *h_cur;                  // out: (c, Hw) of this frame
    uchar4 *rgba;                   // null, or the rgba8 of c (no filter pass follows)
    float *hist;                    // null, or Hw alone
    uint32_t tw, th;
    float n;
    float eye[3];
    float kappa_prev, kappa;        // pixel footprint per unit distance: (|hor| / W) / |llc + hor/2 + ver/2 - eye|
    float max_history, normal_tol2, plane_tol;
    // the 80-byte records as they are and as the previous slot saw them; raw_prev null = the same scene
    const unsigned char *raw, *raw_prev;
    uint32_t nprim;
    // DESIGN.md 6l (option "temporal_clip_pct"): per pixel (lo, N), (hi, valid) as k_dn_clip_box left them; null = off
    const float4 *box;
};

// k_dn_clip_box (option "temporal_clip_pct"): before k_dn_reproject, the colour box of every pixel from the
// frame's own 7x7 neighbourhood; the blend clamps the reprojected history to it.
struct DnClipParams {
    const float4 *accum;            // this frame: XYZ sums of n samples
    const uint32_t *key;
    float4 *box;                    // out: 2 per pixel, (lo.rgb, N) and (hi.rgb, valid)
    uint32_t tw, th;
    float n;
    float gamma;                    // the option's factor, P / 100
};

// k_dn_reproject<*, true>: the blend above plus the temporal moments of the pixel's luminance, and the
// variance they give as the w of the filter's input.  A struct of its own, so that the <*, false> kernels keep theirs.
struct DnSvgfParams : DnReprojParams {
    const float4 *m_prev;           // previous frame: (m1, s, Mw, 0) per pixel; null = the slot has no moments
    float4 *m_cur;                  // out: the moments of this frame
    float4 *cv;                     // out: (c, v), the input of the variance-guided passes
    float *var;                     // null, or v alone (no filter pass follows)
    float min_frames;               // v is trusted from Mw / n >= this on
};

// k_dn_spatial_var (option "svgf_spatial_pct"): after k_dn_reproject<*, true>, the pixels whose variance the
// moments do not give yet take an estimate from the spread of m1 over their 7x7 neighbourhood.  A struct of its own, so that
// k_dn_reproject keeps its argument block.
struct DnSpatialParams {
    const float4 *m_cur;            // this frame's moments (m1, s, Mw, 0), as k_dn_reproject left them
    const float4 *gbuf;             // its G-buffer and keys
    const uint32_t *key;
    float4 *cv;                     // (c, v): only the w lane is rewritten
    float *var;                     // null, or v alone (no filter pass follows)
    uint32_t tw, th;
    float n, min_frames;            // what decides `known`, as in DnSvgfParams
    float b;                        // the option's factor, P / 100
    float inv_n, inv_x;             // the filter's 1 / sigma_normal^2 and 1 / sigma_plane
};

// k_dn_reproject<*, *, true>: the blend in the adaptive state, where the n of pixel p is the count of its 8x8
// tile.  Derived from either block above, so that the <*, *, false> kernels keep theirs.
template <class Base>
struct DnAdaptive : Base {
    const uint32_t *counts;         // per 8x8 tile of the rectangle, row-major: samples it holds (>= 1)
    uint32_t tiles_x;               // ceil(tw / 8)
};

// What the launchers of the four preview filters share (crt_denoise.hip; declared in crt_launch.h).
struct DnFilter {
    const float4 *gbuf;             // the guides: G-buffer and keys of the tile
    const uint32_t *key;
    float4 *c[2];                   // the colour buffers the passes alternate between
    uchar4 *rgba;                   // null, or where the last launch writes the result's rgba8
    uint32_t tw, th, iterations;
    float sigma_normal, sigma_plane;
    hipStream_t stream;
};

// k_aov (crt_aov.hip): the feature planes of the camera rays of samples first + 1 .. first + n of every pixel
// of the rectangle.  A plane whose pointer is null is not stored.
struct AovParams {
    const float *albedo;            // the albedo table: 3 floats per spectra row (crt_spectrum_rgb of the row)
    const uint32_t *counts;         // null: every pixel takes n; else per 8x8 tile of the rectangle, row-major, its n
    uint32_t *hits;                 // per pixel: h, the camera rays that hit something
    float *alpha;                   // (float)h / (float)n
    float *depth;                   // mean t of the hits (CRT_INFINITY at h = 0)
    float4 *normal;                 // mean hit normal, w = +0 (zeros at h = 0)
    float4 *albedo_out;             // mean albedo of the hit primitives, w = +0 (zeros at h = 0)
    uint32_t x0, y0, tw, th, tiles_x;
    uint32_t first, n;
    int brute;                      // CRT_ACCEL_NONE: the reference's loop over every primitive
};

// k_matte (crt_matte.hip): the id mattes of the camera rays of samples first + 1 .. first + n of every pixel
// of the rectangle.  A plane whose pointer is null is not stored.
struct MatteParams {
    const uint32_t *table;          // CRT_MATTE_OBJECT: the id table, one entry per primitive in array order; else unused
    const uint32_t *counts;         // null: every pixel takes n; else per 8x8 tile of the rectangle, row-major, its n
    uint32_t *ids;                  // slots planes of tw * th: plane r = the id of rank r (0xFFFFFFFF: no entry)
    uint32_t *counts_out;           // slots planes: the camera rays that hit that id (0: no entry)
    uint32_t *hits;                 // per pixel: h, the camera rays that hit something
    uint32_t *overflow;             // per pixel: the hits whose id found no slot
    uint32_t x0, y0, tw, th, tiles_x;
    uint32_t first, n;
    uint32_t slots;                 // 1 .. CRT_MATTE_MAX_SLOTS: entries of a pixel's table (sizes the kernel's dynamic LDS)
    int source;                     // CRT_MATTE_PRIMITIVE, _OBJECT, _MATERIAL
    int brute;                      // CRT_ACCEL_NONE: the reference's loop over every primitive
};

// The G-buffer's ray of a pixel (k_dn_gbuffer) and crt_pick's: the primary ray of sample kDnSample.  Its stratum
// (8 + r) / 16 lies within 1/16 pixel of the pixel's centre on both axes, and it is a pure function of (x, y).
constexpr uint32_t kDnSample = 8;

// k_query (crt_query.hip): the closest hit, or whether there is any, of n rays -- the caller's, or the
// G-buffer's rays of n pixels.  A plane whose pointer is null is not stored.
struct QueryParams {
    const float4 *rays;             // caller rays: 2 per ray, (o.xyz, t_max) (d.xyz, exclude bits) = crt_ray; pick: unused
    const uint2 *xy;                // pick: global pixel coordinates per ray; else unused
    const uint32_t *table;          // the id table, one entry per primitive in array order; read only where `id` is stored
    uint32_t *hit;                  // 1 = a primitive was hit
    uint32_t *prim;                 // its array position (kNoHit at a miss)
    uint32_t *id;                   // table[prim] (kNoHit at a miss)
    float *t;                       // the hit's t (at a miss the ray's own t_max)
    float4 *position, *normal;      // hit_attributes' (zeros at a miss), w = +0
    float2 *uv;                     // hit_uv_rec's (zeros at a miss)
    size_t n;
    int wide_ok;                    // 0: the BVH2 even where there is a quantised 4-wide tree (option "pipeline" = 0)
};

// k_radiance (crt_radiance.hip): n_samples paths along each of n caller rays, summed per ray.  A plane whose
// pointer is null is not stored.
struct RadianceParams {
    const float4 *rays;             // 2 per ray, (o.xyz, t_max) (d.xyz, exclude bits) = crt_ray
    const uint4 *keys;              // (x, y, first sample, 0) = crt_path_key per ray; null: (i, 0, 1)
    float4 *xyz;                    // the sum of the paths' XYZ, w = +0
    float *y2;                      // the sum of Y * Y
    uchar4 *rgba8;                  // tonemap_rgba8(xyz, n_samples)
    size_t n;
    uint32_t n_samples;
    int wide_ok;                    // as QueryParams'
};

// The grid of k_radiance: at most this many 64-lane blocks per compute unit, beyond which lanes stride (the
// more blocks the better, up to one ray per lane, on every grid measured).
constexpr uint32_t kRadianceWavesPerCu = 128;

}  // namespace crt
