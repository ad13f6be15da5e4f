/*
 * crt.h -- C ABI of libcrt.so, the MI355X (gfx950) drop-in for the reference's
 * WebGPU path-trace compute pass.
 *
 * What it replaces (all paths under Meryx/ComputeRayTracer):
 *   - the device side:  src/shaders/ComputeShader.wgsl:77-117 (`main`) and
 *     src/shaders/UpdateVariables.wgsl:1-7 (`sample++`);
 *   - the host calls that feed and drive it in src/main.js:
 *       createBuffer/getMappedRange/unmap of bind-group-0 entries b4..b8
 *                                   (main.js:147-155,249-253,263-296,313-393)
 *       the zeroed accumulator + sample counter           (main.js:298-311)
 *       per-frame  dispatchWorkgroups(1) ; dispatchWorkgroups(ceil(W/8),ceil(H/8))
 *                                                          (main.js:598-611)
 *       uncapturederror reporting                          (main.js:11-14)
 *
 * Conventions: plain C, caller-owned host pointers, sizes in records unless
 * stated; every function returns 0 on success or a negative CRT_E* code and
 * leaves a message for crt_last_error().  One thread per context.  Work is
 * enqueued on the context's HIP stream; crt_sync / crt_read_* wait for it.
 * There is NO CPU fallback: without a HIP device crt_create fails.
 */
#ifndef CRT_H
#define CRT_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define CRT_ABI_VERSION 2

enum {
    CRT_OK = 0,
    CRT_EINVAL = -1,   /* bad argument / malformed buffer            */
    CRT_EDEVICE = -2,  /* HIP runtime error (message has the detail) */
    CRT_ESTATE = -3,   /* call out of order (e.g. trace before upload) */
    CRT_ENOMEM = -4
};

/* Acceleration modes for crt_build_accel. */
enum {
    CRT_ACCEL_NONE = 0, /* the reference's own loop over every primitive
                           (ComputeShader.wgsl:503-518), on the GPU        */
    CRT_ACCEL_BVH2 = 1, /* binned-SAH BVH2 built on the host; returns exactly
                           what the loop returns (closest t; equal t -> later
                           primitive) */
    CRT_ACCEL_LBVH = 2, /* the same structure built on the GPU, end to end (Morton order,
                           Karras hierarchy, collapse to 4-wide, quantisation, leaf-ordered
                           records): milliseconds instead of seconds to build (10 M
                           triangles: 0.11 s), same image, more nodes visited per ray  */
    CRT_ACCEL_PLOC = 3  /* the same BVH2 and wide-tree structures, built on the GPU by parallel
                           locally-ordered clustering over the LBVH's Morton order (option
                           "ploc_radius"): same image, a build of milliseconds, and a tree
                           closer to the SAH builder's than the LBVH's (fewer nodes visited
                           per ray).  Follows the LBVH mode's contract; a hierarchy too deep
                           for the walk's stacks is built as the LBVH by the same call, with
                           a note in crt_last_error */
};

/* Counter slots for crt_counters(). */
enum {
    CRT_CNT_RAYS = 0,        /* intersect() invocations (primary+bounce+shadow) */
    CRT_CNT_NODES = 1,       /* BVH child boxes tested (2 per inner-node visit) */
    CRT_CNT_PRIMS = 2,       /* primitive intersection tests                    */
    CRT_CNT_PATHS = 3,       /* pixel-samples                                   */
    CRT_CNT_BOUNCES = 4,     /* path-loop iterations                            */
    CRT_CNT_SHADOW = 5,      /* shadow rays (subset of RAYS)                    */
    CRT_CNT_HITS = 6,        /* closest-hit attribute fetches                   */
    CRT_CNT_WALKED = 7,      /* rays that actually walked the BVH: RAYS minus shadow rays decided
                                without a walk (light's own primitive missed, or cos_theta == 0 and the
                                NEE term exactly zero) -- wavefront pipeline only                     */
    CRT_NCOUNTERS = 8
};

typedef struct crt_ctx crt_ctx;

/* ~ navigator.gpu.requestAdapter()/requestDevice(), main.js:8-9. */
int crt_create(crt_ctx **out, int device_ordinal);
void crt_destroy(crt_ctx *ctx);
const char *crt_last_error(crt_ctx *ctx);   /* ctx may be NULL: last create error */
int crt_abi_version(void);

/* ~ the b4..b8 buffer uploads (main.js:147-393).  Byte layouts are exactly the
 * reference's: 80-byte Primitive records (category@0, data1@16, data2@32,
 * data3@48, data4@64 = emission_idx, reflectance_idx, material, index), camera
 * = 16 floats (eye,_,lookat,_,up,width,height,focal,_,_), spectra = nspectra
 * rows of 301 floats (last row = glass extinction), cie = 3 x 471 floats.
 * Requirements checked here: data4.w == array position (main.js:124,133
 * guarantees it), category in {0 patch,1 sphere,2 triangle}, material in
 * {0,1,2}, nlight >= 1.  Resets the accumulator and the accel structure. */
int crt_upload_scene(crt_ctx *ctx,
                     const void *primitives, size_t nprim,
                     const void *lights, size_t nlight,
                     const float *spectra, size_t nspectra,
                     const float *cie,
                     const float camera[16]);

/* Restrict this context to the pixel rectangle [x0,x1) x [y0,y1) of the full
 * W x H image (image-tile partition across GPUs).  Default: the whole image.
 * RNG seeds use the GLOBAL pixel coordinates (ComputeShader.wgsl:98), so a
 * tile is bit-identical to the same pixels of a full-frame render.  Resets the
 * accumulator. */
int crt_set_tile(crt_ctx *ctx, uint32_t x0, uint32_t y0, uint32_t x1, uint32_t y1);

/* Row-interleaved partition for load balance across GPUs: this context renders the rows y of
 * the full frame with (y / band_rows) % parts == part, full width, packed densely in its
 * buffers (local row j is global row ((j / band) * parts + part) * band + j % band).
 * Resets the accumulator.  crt_set_tile returns to a plain rectangle. */
int crt_set_row_bands(crt_ctx *ctx, uint32_t band_rows, uint32_t parts, uint32_t part);

int crt_build_accel(crt_ctx *ctx, int mode);

/* ~ main.js:298-311: zero alt_color_buffer, sample = 0. */
int crt_reset(crt_ctx *ctx);

/* ~ n_samples iterations of frame() (main.js:597-611):
 *   { sample++ (UpdateVariables.wgsl) ; path-trace dispatch (ComputeShader.wgsl) }.
 * Samples are accumulated into alt_color_buffer in order; the rgba8
 * framebuffer holds the tone-mapped average after the last one.
 * Asynchronous, and (option "wf_defer", default 1) PIPELINED across calls: a call publishes
 * its samples as a batch, enqueues the work the batch needs and returns without waiting for it;
 * up to "wf_ring" (default 32) batches are in flight, resolved in order under the following
 * crt_trace calls or in crt_sync.  A call only blocks for back-pressure (the ring is full).
 * Small calls are MERGED: their samples become one batch once "wf_cohort" (default 16) samples
 * have come together, or at crt_sync / any call that reads state (a batch of many samples per
 * pixel keeps the paths in flight inside a band of the image and runs 1.4x faster per sample;
 * the frames are the same bit for bit; "wf_cohort" = 1 makes every call its own batch).  So:
 *   - after crt_sync (or any crt_read_*, crt_counters, crt_last_*_ms) the buffers
 *     hold every sample requested so far;
 *   - in between, buffers bound with crt_bind_output hold, in stream order, the
 *     complete frame of an EARLIER crt_trace call -- at most wf_ring batches before the
 *     last one -- never a half-resolved one.  A display/gather loop that shows the latest
 *     complete frame while the next ones render needs no sync at all. */
int crt_trace(crt_ctx *ctx, uint32_t n_samples);
/* Finish everything requested so far and wait for it. */
int crt_sync(crt_ctx *ctx);

/* Current value of the `sample` counter (ComputeShader.wgsl:3). */
int crt_sample_count(crt_ctx *ctx, uint32_t *out);

/* Tile geometry: out[4] = x0, y0, width, height. */
int crt_tile(crt_ctx *ctx, uint32_t out[4]);

/* Readback of this context's tile, row-major, row 0 = top (the reference never
 * reads back; its blit pass is display-only).  accum: tw*th*4 floats (x,y,z,
 * pad -- the 16-byte stride of array<vec3<f32>>); rgba8: tw*th*4 bytes. */
int crt_read_accum(crt_ctx *ctx, float *out);
int crt_read_rgba8(crt_ctx *ctx, uint8_t *out);
/* The display step of the reference's frame loop (src/main.js:597-620 shows EVERY sample's frame: compute pass, blit,
 * requestAnimationFrame) without stopping the pipeline:
 *   crt_read_latest_rgba8   the newest COMPLETE frame in stream order and its sample index -- no flush: batches in
 *                           flight stay in flight (crt_read_rgba8 finishes everything first);
 *   crt_latest_sample       that index alone (non-blocking; retires what has finished meanwhile);
 *   crt_read_sample_rgba8   the frame as it was after exactly `sample` samples, from a ring of the last F frames (option
 *                           "frame_ring" = F, set before tracing; k_wf_resolve then stores every sample's frame, bit-identical
 *                           to a synced crt_trace(1) loop).  Waits only for the batch that holds the sample; a display loop
 *                           that requests frames a cohort ahead of the one it shows (host/display_loop.js) sees every frame
 *                           index exactly once while small calls are still merged into cohorts.  CRT_EINVAL for a sample that
 *                           has not been requested, has left the ring, or predates the context's last crt_reset /
 *                           crt_write_accum / change of "frame_ring" (a restored accumulator brings no frames with it). */
int crt_read_latest_rgba8(crt_ctx *ctx, uint8_t *out, uint32_t *sample);
/* Page-lock / release caller memory (hipHostRegister): readbacks into pinned memory run at PCIe speed -- for the frame
 * buffer a display loop reads every frame into.  No context needed; errors are reported through crt_last_error(NULL). */
int crt_pin_host(void *ptr, size_t bytes);
int crt_unpin_host(void *ptr);
int crt_latest_sample(crt_ctx *ctx, uint32_t *out);
int crt_read_sample_rgba8(crt_ctx *ctx, uint32_t sample, uint8_t *out);
/* Restore an accumulator + sample count (checkpoint/resume). */
int crt_write_accum(crt_ctx *ctx, const float *in, uint32_t sample);

/* Device pointers of the tile buffers (for an RCCL gather by the caller). */
int crt_device_buffers(crt_ctx *ctx, void **accum_dev, void **rgba8_dev);
/* Render into caller-owned DEVICE memory instead (e.g. a slice of a gather
 * buffer): accum_dev >= tw*th*16 B, rgba8_dev >= tw*th*4 B; NULL restores the
 * internal buffers. */
int crt_bind_output(crt_ctx *ctx, void *accum_dev, void *rgba8_dev);
/* Enqueue on the caller's hipStream_t instead of the context's own. */
int crt_set_stream(crt_ctx *ctx, void *hip_stream);

/* The context's device ordinal and the HIP stream it enqueues on (hipStream_t as void*), the full image's size
 * (out[2] = W, H): for code that composes with the context from outside, like the gather below. */
int crt_get_device(crt_ctx *ctx, int *out);
int crt_get_stream(crt_ctx *ctx, void **out);
int crt_image_size(crt_ctx *ctx, uint32_t out[2]);

/* ------------------------------------------------------------------ Multi-GPU: the frame across the ranks of a communicator
 * The reference drives ONE GPUDevice (src/main.js:8-9) and has no exchange step.  Here the frame is partitioned by rows
 * across `world` contexts -- one per GPU, as a rule one process per GPU -- the scene replicated, and the path's only
 * exchange is the gather of the finished strips: an RCCL all-gather over xGMI issued from libcrt on the context's stream
 * (SURVEY 8e).  Pixels depend on their global coordinates only (ComputeShader.wgsl:85-86,98), so the assembled frame is
 * bit-identical for every world size.
 *
 *   crt_comm_unique_id(id, CRT_COMM_RCCL)      on one rank; hand the 128 bytes to the others (IPC, a file, a socket)
 *   crt_comm_init(ctx, id, rank, world)        every rank, after crt_create (collective for RCCL)
 *   crt_upload_scene(ctx, ...)                 the same scene on every rank
 *   crt_comm_partition(ctx, band_rows)         this rank's rows: bands of band_rows rows dealt round-robin (8 balances
 *                                              regions of different path length), 0 = contiguous strips; the context then
 *                                              renders into strip buffers owned by the communicator (resets the accumulator)
 *   crt_build_accel; loop { crt_trace(ctx, n); crt_gather(ctx, CRT_GATHER_RGBA8); }     every rank
 *   crt_sync(ctx); crt_gather(ctx, CRT_GATHER_RGBA8 | CRT_GATHER_ACCUM);
 *   crt_read_frame_rgba8 / crt_read_frame_accum(ctx, out)       any rank: the whole W x H frame
 *
 * crt_gather is asynchronous and stream-ordered like crt_trace: it ships what the strip holds THEN -- after crt_sync
 * every sample requested so far, in a pipelined loop the latest complete frame (crt_trace's contract for bound outputs).
 * CRT_COMM_LOCAL is the same interface for contexts of ONE process (any devices): strips are exchanged with
 * device-to-device copies, no RCCL; every rank posts its crt_gather before any rank reads the frame.
 *
 * A partition goes STALE when the application calls crt_upload_scene, crt_set_tile or crt_set_row_bands on the context
 * after crt_comm_partition, or crt_bind_output with other pointers than the communicator's strips (crt_comm_partition's own
 * use of those calls does not count): the context no longer renders into the strips, and W and H may have changed.  On a
 * stale partition crt_gather, crt_read_frame_rgba8, crt_read_frame_accum and crt_frame_device_buffers return CRT_ESTATE
 * ("call crt_comm_partition again"); they enqueue nothing and write nothing to `out`.  The communicator's buffers live until
 * the next crt_comm_partition or crt_comm_destroy, so a copy a peer has in flight into them stays safe; crt_comm_info
 * keeps answering; crt_trace_adaptive takes a stale partition for none; a fresh crt_comm_partition (on every rank, if W or
 * H changed) makes everything work again.  A peer that is still current may post its crt_gather, but the frame of that
 * gather is never complete (crt_read_frame_*: CRT_ESTATE). */
#define CRT_COMM_ID_BYTES 128
enum { CRT_COMM_RCCL = 0, CRT_COMM_LOCAL = 1 };
enum { CRT_GATHER_RGBA8 = 1, CRT_GATHER_ACCUM = 2, CRT_GATHER_PREVIEW = 4 /* "The frame of a partition" below */ };
int crt_comm_unique_id(void *out_id /* CRT_COMM_ID_BYTES */, int transport);
int crt_comm_init(crt_ctx *ctx, const void *id, int rank, int world);
int crt_comm_partition(crt_ctx *ctx, uint32_t band_rows);
int crt_gather(crt_ctx *ctx, int what);
int crt_read_frame_rgba8(crt_ctx *ctx, uint8_t *out /* W*H*4, row 0 = top */);
int crt_read_frame_accum(crt_ctx *ctx, float *out /* W*H*4 floats */);
/* Device pointers of the assembled frame of the latest gather (valid until the next crt_comm_partition). */
int crt_frame_device_buffers(crt_ctx *ctx, void **accum_dev, void **rgba8_dev);
/* out[4] = rank, world, transport (-1: no communicator), rows of this rank. */
int crt_comm_info(crt_ctx *ctx, int out[4]);
int crt_comm_destroy(crt_ctx *ctx);          /* also done by crt_destroy */
/* The row layout itself (no GPU involved): the rows of the H-row frame that belong to `part` of `parts`, in local order;
 * n_rows receives their number, global_rows (may be NULL) their indices.  band_rows = 0: contiguous strips. */
int crt_layout_rows(uint32_t H, uint32_t band_rows, uint32_t parts, uint32_t part, uint32_t *n_rows, uint32_t *global_rows);

/* ------------------------------------------------------------------ Denoised preview
 * The reference shows one sample per frame (src/main.js:584-621): for the first hundreds of frames that is Monte-Carlo
 * noise.  crt_denoise filters the accumulator's average with an edge-aware a-trous wavelet filter (Dammertz et al.
 * 2010; DESIGN.md "Denoised preview" defines it), guided by the first hit of each pixel: the primary ray of sample 8
 * (within 1/16 pixel of the pixel's centre), its position, normal and material key.  It only READS the accumulator and
 * the sample count: alt_color_buffer, the rgba8 framebuffer, `sample` and the counters stay as they are.
 * Both calls are sync points like crt_read_rgba8 (every pipelined batch is finished first).  CRT_ESTATE without a
 * scene or accel structure, at sample 0, or under a row-band partition (crt_set_row_bands, crt_comm_partition with
 * band_rows > 0: neighbouring local rows are not neighbouring image rows; crt_denoise_frame filters the gathered frame
 * instead); a crt_set_tile rectangle is filtered on its own, its edges taken as image borders.  The G-buffer is built on first use and kept until crt_upload_scene,
 * crt_build_accel, crt_set_tile or crt_set_row_bands. */
typedef struct {
    uint32_t iterations;   /* filter passes, step 2^i in pass i: 0..10 (0 = the plain average, as crt_read_rgba8) */
    float sigma_color;     /* edge-stopping scales, all > 0 and finite */
    float sigma_normal;
    float sigma_plane;
} crt_denoise_params;
/* NULL params = defaults {5, 1.0, 0.5, 0.3}.  rgb_out: tw*th*4 floats (linear rgb + pad) or NULL; rgba8_out: tw*th*4
 * bytes (the reference's colour tail: exposure, gamma, unorm8) or NULL.  CRT_EINVAL for iterations > 10 or a bad sigma. */
int crt_denoise(crt_ctx *ctx, const crt_denoise_params *params, float *rgb_out, uint8_t *rgba8_out);
/* crt_denoise of the newest COMPLETE frame, without a flush: to crt_denoise what crt_read_latest_rgba8 is to
 * crt_read_rgba8 -- the filtered preview of a display loop that keeps its crt_trace(1) calls a cohort ahead.  Batches in
 * flight stay in flight and samples merged into an unpublished cohort stay unpublished; the call gives the driver one
 * turn (as crt_read_latest_rgba8 does), takes s = the newest sample whose resolve pass is enqueued, and returns the filtered
 * frame of exactly s samples: rgb_out and rgba8_out are, bit for bit, what crt_denoise with the same parameters returns on
 * a context that holds exactly s samples of the same scene; *sample = s (`sample` may be NULL).  Parameters, defaults and
 * CRT_EINVAL cases are crt_denoise's.  It blocks until its own outputs are written and waits for nothing the pipeline
 * enqueued after the resolve pass of sample s: the context's stream gets one snapshot pass (accumulator / s into the
 * filter's buffer), everything else runs on a second stream.  It only reads the frame state: the accumulator, the rgba8
 * framebuffer, `sample`, the counters, the frame ring and the history slots of the temporal filters stay as they are (the
 * G-buffer is built on first use and kept, as by crt_denoise, in a guide set no history slot names), and a later crt_sync
 * leaves the accumulator bit for bit what it would have been without the call.
 * CRT_ESTATE where crt_denoise refuses (no scene or accel structure, a stale tree, row bands, the adaptive state), and when
 * s == 0 -- no complete frame yet: *sample is set to 0 and the caller tries again later; CRT_ENOMEM as crt_denoise.  A
 * refused call enqueues nothing and writes nothing to rgb_out / rgba8_out.  With nothing in flight ("pipeline" = 0,
 * CRT_ACCEL_NONE, "wf_defer" = 0, after crt_sync) the call equals crt_denoise and *sample = crt_sample_count.
 * Option "denoise_latest_wave_blocks" = 1 (default 0) runs its passes in one-wave blocks of 8x8 pixels (the same bits). */
int crt_denoise_latest(crt_ctx *ctx, const crt_denoise_params *params, float *rgb_out, uint8_t *rgba8_out, uint32_t *sample);
/* The G-buffer: tw*th*8 floats, the crt_debug_intersect record per pixel (t, px,py,pz, nx,ny,nz, index_bits;
 * index 0xFFFFFFFF = miss). */
int crt_read_gbuffer(crt_ctx *ctx, float *out);

/* ------------------------------------------------------------------ Feature planes
 * What compositing and an external denoiser ask for beside the beauty image: anti-aliased alpha, depth,
 * normal and albedo.  crt_read_gbuffer is ONE ray per pixel, a filter guide; these planes are averages over the very
 * camera rays the image was averaged over, so a silhouette pixel is fractional and a pixel that sees two primitives
 * reports both.  The camera ray of sample s of pixel (x, y) is a pure function of (x, y, s): the planes are rendered after
 * the fact by a kernel of their own, and the path-tracing kernels are not involved.
 *
 * For every pixel (px, py) of the context's rectangle (global coordinates), with B = crt_sample_offset, the camera rays of
 * samples B + 1 .. B + n are taken in this order; each one's closest hit is found as crt_read_gbuffer finds it.  The
 * sums start at +0; a hit does h++, st = st + t, sn = sn + normal, sa = sa + A[reflectance index] (per component), every
 * step one binary32 operation.  Then alpha = (float)h / (float)n and, with h > 0, depth = st / (float)h,
 * normal = sn / (float)h (not renormalised), albedo = sa / (float)h.
 * n_samples > 0: that many samples for every pixel (also at sample 0 and in the adaptive state).  n_samples == 0: what
 * the accumulator holds -- crt_sample_count in the uniform state (CRT_ESTATE at 0), in the adaptive state the count of
 * the pixel's 8x8 tile; a tile that holds 0 samples gives the h = 0 outputs and alpha = 0 / 0, a NaN.
 * A, the albedo table, has one row per spectra row: crt_spectrum_rgb of it, rebuilt by crt_upload_scene on the host.
 * The row is taken by the hit primitive's reflectance index (data4.y) whatever its material: emitters and glass get the
 * colour of their reflectance row too.
 * A sync point like crt_read_gbuffer (what is in flight finishes first), and it only reads: the accumulator, the rgba8
 * framebuffer, `sample`, the counters, the frame ring, the adaptive state and the filters' state and history stay as
 * they are, and the next crt_trace / crt_trace_adaptive continues bit for bit.  A crt_set_tile rectangle is rendered on
 * its own and equals the crop of the full frame.  The device planes belong to the context (allocated on first use, before
 * anything is enqueued: CRT_ENOMEM leaves nothing behind), and go with it.
 * CRT_ESTATE without a scene or accel structure, with a stale tree (crt_update_primitives, crt_remove_primitives, ...:
 * crt_refit_accel first), and under a row-band partition where crt_read_gbuffer refuses; CRT_EINVAL for out == NULL or
 * when B + n would pass 2^32 - 1.
 * Out of scope: a frame-level form across a crt_comm_partition; feeding these planes into the library's own filters. */
typedef struct {
    uint32_t *hits;   /* tw*th    camera rays of the pixel that hit something, h                            */
    float *alpha;     /* tw*th    (float)h / (float)n                                                       */
    float *depth;     /* tw*th    mean t of the hits; 2139095040.0f (the kernels' CRT_INFINITY) at h = 0    */
    float *normal;    /* tw*th*4  mean hit normal (not renormalised), channel 3 = +0; zeros at h = 0        */
    float *albedo;    /* tw*th*4  mean albedo of the hit primitives, channel 3 = +0; zeros at h = 0         */
} crt_aov_planes;     /* any pointer may be NULL (that plane is neither allocated nor stored); row-major over the
                       * context's rectangle, row 0 = top */
int crt_render_aovs(crt_ctx *ctx, uint32_t n_samples, const crt_aov_planes *out);
/* One row of the albedo table (no context, no GPU): the reflectance spectrum[301] under an equal-energy illuminant with
 * white Y = 1, as linear sRGB.  In binary64, k ascending from 0 to 300: X = sum (double)spectrum[k] * cieX[k + 40], Y and
 * Z likewise, N = sum cieY[k + 40]; x = X / N, y = Y / N, z = Z / N; out[r] = (m0 x + m1 y) + m2 z with the XYZ -> linear
 * sRGB matrix of the tone map (3.2404542, ...), each rounded once to float.  CRT_EINVAL for a NULL pointer. */
int crt_spectrum_rgb(const float *spectrum /* 301 */, const float *cie /* 3*471 */, float out[3]);
/* The table crt_render_aovs reads: nspectra*3 floats, row i = crt_spectrum_rgb of spectra row i.  No GPU work. */
int crt_read_albedo_table(crt_ctx *ctx, float *out /* nspectra*3 */);

/* ------------------------------------------------------------------ ID mattes
 * What compositing asks for to isolate one object: per pixel, which ids its camera rays hit and how many
 * rays hit each -- an anti-aliased matte per primitive, object or material, in the Cryptomatte style.  crt_read_gbuffer
 * reports one primitive per pixel, from one ray; the planes of crt_render_aovs average over primitives without saying
 * which.  Like those planes the mattes are rendered after the fact, over the very camera rays the image holds, by a
 * kernel of their own; every output is an integer.
 *
 * Rays.  For every pixel of the context's rectangle, with B = crt_sample_offset, the camera rays of samples B + 1 .. B + n
 * are taken in this order; each one's closest hit is found exactly as crt_render_aovs finds it (the reference's loop over
 * every primitive under CRT_ACCEL_NONE and for a non-finite ray).  n is crt_render_aovs': n_samples > 0 is that many
 * samples for every pixel (also at sample 0 and in the adaptive state); n_samples == 0 is what the accumulator holds --
 * crt_sample_count in the uniform state (CRT_ESTATE at 0), in the adaptive state the count of the pixel's 8x8 tile.
 * The id of a hit of the primitive at array position i, by `source`:
 *   CRT_MATTE_PRIMITIVE  i
 *   CRT_MATTE_OBJECT     entry i of the id table (below)
 *   CRT_MATTE_MATERIAL   material << 24 | reflectance index (data4.z, data4.y): the key the preview filters compare
 * The table.  Each pixel keeps a table of `slots` entries (1 .. CRT_MATTE_MAX_SLOTS), empty at the start.  For every hit,
 * in sample order: h++; if the id is in the table its count goes up by one; else, if the table holds fewer than `slots`
 * entries, the entry (id, 1) is added; else overflow++.
 * Ranking.  The entries are ranked by count descending, equal counts by id ascending (unsigned); rank r goes to plane r.
 * A rank without an entry holds id 0xFFFFFFFF and count 0.
 * So for every pixel: sum of counts + overflow = hits <= n.  With overflow == 0 the result is the exact ranking over all
 * the ids the pixel saw and does not depend on the sample order.  With overflow > 0 it is NOT: an id that first appeared
 * after the table had filled is counted in `overflow` only, however many rays hit it, and the ranking is that of the
 * first `slots` ids in sample order -- ask for more slots.  The coverage of an id is count / n; the C call returns
 * integers only and the bindings divide.
 * The contract is crt_render_aovs': a sync point; it only reads -- the accumulator, the rgba8 framebuffer, `sample`, the
 * counters, the frame ring, the adaptive state and the filters' state and history stay as they are, and the next
 * crt_trace / crt_trace_adaptive continues bit for bit; a crt_set_tile rectangle equals the crop of the full frame; the
 * device planes belong to the context and every allocation is made before anything is enqueued (CRT_ENOMEM leaves
 * nothing behind).  CRT_ESTATE in crt_render_aovs' cases: no scene or accel structure, a stale tree, row bands,
 * n_samples == 0 at sample 0, the adaptive state after a call that failed part-way.  CRT_EINVAL for out == NULL, slots
 * outside 1 .. 16, an unknown source, or when B + n would pass 2^32 - 1.
 * Out of scope: a frame-level form across a crt_comm_partition; Cryptomatte / EXR files; the exact ranking of a pixel
 * that sees more than `slots` ids; editing ids on the device; feeding ids into the library's own filters. */
enum { CRT_MATTE_PRIMITIVE = 0, CRT_MATTE_OBJECT = 1, CRT_MATTE_MATERIAL = 2 };
#define CRT_MATTE_MAX_SLOTS 16
typedef struct {
    uint32_t *ids;       /* slots*tw*th  plane r (tw*th values, row-major, row 0 = top) = the id of rank r; 0xFFFFFFFF = no entry */
    uint32_t *counts;    /* slots*tw*th  camera rays of the pixel that hit that id; 0 where there is no entry */
    uint32_t *hits;      /* tw*th        camera rays that hit anything: crt_render_aovs' hits plane */
    uint32_t *overflow;  /* tw*th        hits whose id found no slot (above) */
} crt_matte_planes;      /* any pointer may be NULL: that plane is neither allocated nor stored */
int crt_render_mattes(crt_ctx *ctx, uint32_t n_samples, int source, uint32_t slots, const crt_matte_planes *out);
/* The id table: one uint32_t per primitive, on the host beside the records.  crt_upload_scene makes it the identity
 * (entry i = i); the device copy is made by the first crt_render_mattes of source OBJECT that needs it and dropped
 * whenever the table changes, so the upload and the scene edits allocate on the device what they did without it.
 * crt_set_primitive_ids replaces entries [first, first+count) and touches nothing else: the accumulator is not reset, the
 * tree does not go stale, no history is dropped.  CRT_EINVAL, with nothing changed, for a range outside the scene, ids ==
 * NULL with count > 0, or an id of 0xFFFFFFFF (reserved for "no entry"); CRT_ESTATE without a scene.
 * crt_read_primitive_ids copies from the host table: no GPU work, the same range checks.
 * Under the scene edits: crt_update_primitives and crt_transform_primitives leave the table alone;
 * crt_remove_primitives compacts it exactly as it compacts the records (a survivor keeps its id); crt_append_primitives
 * gives appended primitive nprim + k the id nprim + k (the caller then sets the ids it wants).  The host memory the table
 * needs is reserved before anything changes, and a refused edit leaves the table as it was. */
int crt_set_primitive_ids(crt_ctx *ctx, uint32_t first, uint32_t count, const uint32_t *ids);
int crt_read_primitive_ids(crt_ctx *ctx, uint32_t first, uint32_t count, uint32_t *out);

/* ------------------------------------------------------------------ Ray queries
 * "Here are my rays, what do they hit?" (DESIGN.md 6p): closest-hit and occlusion queries for caller rays, from host
 * memory or from device memory on a stream of the caller's, and the same for the camera ray under a pixel.  A kernel of
 * its own walks the tree the stragglers' kernel walks; the path tracer is not involved and is NOT stopped.
 *
 * Definition.  A ray (o, d, t_max, exclude) hits primitive i at distance t exactly when the reference's loop over every
 * primitive (ComputeShader.wgsl:503-518) accepts it with that exclude index, started with the ray's t_max and no hit
 * held: 0.001 <= t <= t_max -- the end is inclusive, an equal t is accepted while nothing is held -- and every other rule
 * is the hit test's own (the triangle's pad, the patch's grazing cut, the sphere's far root when the near one is below
 * 0.001).  CRT_QUERY_CLOSEST reports the smallest t; equal t goes to the later primitive, as everywhere in this library.
 * d need not be normalised: t is in units of |d|.  exclude = 0xFFFFFFFF excludes nothing.  t_max = 2139095040.0f (the
 * kernels' "infinity") or +inf is "no limit"; a NaN or negative t_max can never be beaten and gives a miss -- it is not
 * an error, device rays cannot be validated.  A ray whose origin or direction has a component that is NaN or of
 * magnitude >= 3.0e38 is a miss in every accel mode: it is never walked and never sent through the loop over all
 * primitives.  This differs on purpose from crt_read_gbuffer and the debug hooks, which give such a ray the reference's
 * loop: a public call must not spend nprim tests on each ray of a garbage batch.
 * CRT_QUERY_ANY reports `hit` alone, 1 exactly when CRT_QUERY_CLOSEST would hit: the walk stops at the first accepted
 * primitive, and which one that is depends on the tree, so every other plane must be NULL (CRT_EINVAL).
 * uv: the surface coordinates the hit test itself computed for the winning primitive, its operations in its order,
 * recomputed after the walk from the same record.  Triangle (v0, e1, e2): pvec = cross(d, e2), inv = 1 / dot(e1, pvec),
 * tvec = o - v0, u = dot(tvec, pvec) * inv, v = dot(d, cross(tvec, e1)) * inv (the hit is v0 + u e1 + v e2).  Patch
 * (P0, e1, e2): m = (o + t d) - P0, u = dot(m, e1) / dot(e1, e1), v = dot(m, e2) / dot(e2, e2).  Spheres: +0, +0.
 * Which walk: the quantised 4-wide tree where the stragglers' kernel walks it (a ray whose stack it cannot hold is
 * repeated on the BVH2); the BVH2 under options "quantize" 0, "wf_width" 8 and "pipeline" 0; the reference's loop under
 * CRT_ACCEL_NONE.  The result does not depend on it.
 *
 * Contract, the same for the three calls.  They read only the scene, the tree and the id table: the accumulator, the
 * framebuffer, `sample`, the counters, the frame ring, the adaptive state, the filters' state and history and the
 * G-buffer stay as they are.  They do NOT flush: batches in flight stay in flight, samples merged into an unpublished
 * cohort stay unpublished, the pipeline's driver gets no turn.  They work at sample 0, in the adaptive state, under
 * crt_set_tile, row bands and a crt_comm_partition: none of these bears on a ray.  CRT_ESTATE without a scene or an accel
 * structure, and while the tree is stale (after an edit, until crt_refit_accel or crt_build_accel).  CRT_EINVAL for out
 * == NULL, every plane NULL, an unknown mode, rays == NULL with n > 0, rays or a 4-wide plane (position, normal) not
 * 16-byte aligned, n >= 2^32.  n == 0 succeeds and does nothing.
 * crt_query_rays (host pointers) runs on a non-blocking stream the context owns and waits for that stream only.  Its
 * staging buffers belong to the context, grow by at least half and are released by crt_upload_scene and crt_destroy;
 * every allocation -- staging, and the id table's device copy where `id` is asked for and a change has dropped it -- is
 * made before anything is enqueued, so CRT_ENOMEM enqueues nothing and writes nothing to `out`.  Growing a buffer frees
 * the old one, and hipFree waits for the device: a call that grows (the first, or a larger n than any before) can wait
 * for work in flight; the calls after it do not.
 * crt_query_rays_device takes rays_dev and the pointers of *out_dev (a struct in host memory) as device pointers reachable
 * from the context's device, enqueues ONE launch on hip_stream (a hipStream_t as crt_set_stream takes it; NULL = the null
 * stream) and returns without waiting.  It allocates nothing but the id table's device copy, and that only when needed.
 * The caller orders its reads after the launch, and must have finished its queries before any call that changes the
 * scene or the tree (crt_upload_scene, crt_build_accel, the scene edits, crt_refit_accel, crt_set_primitive_ids) and
 * before crt_destroy: those calls wait for the context's streams, not for the caller's.
 * crt_pick (host pointers) queries the G-buffer's ray of each pixel (x, y): the primary ray of sample 8 with the pixel's
 * own seed, generated in the kernel, no limit, no exclude.  Coordinates are global and must be below W and H (CRT_EINVAL);
 * crt_set_tile does not move them.  For a finite camera ray, t, position, normal and prim are bit for bit
 * crt_read_gbuffer's record of that pixel.  It follows crt_query_rays' contract, so a click in a display loop does not
 * stop the pipeline.
 * Out of scope: caller rays through the wavefront kernel's ray lists; sorting or compacting rays; a per-ray t_min;
 * instancing; a frame-level form across ranks. */
typedef struct { float o[3]; float t_max; float d[3]; uint32_t exclude; } crt_ray;   /* 32 bytes; arrays 16-byte aligned */
enum { CRT_QUERY_CLOSEST = 0, CRT_QUERY_ANY = 1 };
typedef struct {
    uint32_t *hit;      /* n    1 = a primitive was hit, else 0                                              */
    uint32_t *prim;     /* n    array position of the hit primitive; 0xFFFFFFFF at a miss                    */
    uint32_t *id;       /* n    entry `prim` of the id table (crt_set_primitive_ids); 0xFFFFFFFF at a miss   */
    float *t;           /* n    the hit's t; at a miss the ray's own t_max, bit for bit                      */
    float *position;    /* n*4  the hit point o + t d, channel 3 = +0; zeros at a miss                       */
    float *normal;      /* n*4  the unit normal (faces the ray on patches and triangles, outward on
                                spheres), channel 3 = +0; zeros at a miss                                    */
    float *uv;          /* n*2  surface coordinates (above); +0, +0 on spheres and at a miss                 */
} crt_query_planes;     /* any pointer may be NULL: that plane is neither allocated nor stored */
int crt_query_rays(crt_ctx *ctx, const crt_ray *rays, size_t n, int mode, const crt_query_planes *out);
int crt_query_rays_device(crt_ctx *ctx, const crt_ray *rays_dev, size_t n, int mode, const crt_query_planes *out_dev,
                          void *hip_stream);
int crt_pick(crt_ctx *ctx, const uint32_t *xy /* n pairs, global pixel coordinates */, size_t n, const crt_query_planes *out);

/* ------------------------------------------------------------------ Radiance queries
 * "Here are my rays, how much light arrives along them?" (DESIGN.md 6q): the path tracer's radiance for caller rays -- a
 * panorama, a fisheye or thin-lens view, an irradiance probe, a light-meter reading, the texels of a lightmap (crt_query_rays
 * returns the uv to bake into) -- from host memory or from device memory on a stream of the caller's.  A kernel of its own
 * beside the path tracer, built as the ray queries' kernel is; the pipeline is not involved and is NOT stopped.
 *
 * Definition.  For ray i with record (o, t_max, d, exclude) and key (x, y, s0) -- keys == NULL means x = (uint32_t)i,
 * y = 0, s0 = 1 -- the sums start at +0, and for j = 0 .. n_samples-1, in this order:
 *   1. s = s0 + j in uint32_t arithmetic (it wraps);
 *   2. rng = {y, x*100u, s, tea(x, y*100u)}, as ComputeShader.wgsl:98 seeds sample s of pixel (x, y);
 *   3. two rnd(rng) draws whose values are not used: the camera's two jitter draws, which put the stream where the
 *      reference has it when path_trace starts;
 *   4. sample_wavelengths (one draw);
 *   5. the reference's path_trace (:119-295) from (o, d) with that stream and those wavelengths, with exactly two
 *      extensions, both of the FIRST segment only: `exclude` takes the place of the initial 0xFFFFFFFF, and a first hit
 *      must satisfy crt_query_rays' definition with the ray's t_max (2139095040.0f or +inf = no limit; a NaN or negative
 *      limit makes the first segment a miss).  With exclude = 0xFFFFFFFF and no limit the path is the reference's own, bit
 *      for bit: with the rays of a camera and keys (x, y, s) the sums are what crt_read_accum holds;
 *   6. c = spectral_to_xyz(radiance, wavelengths);
 *   7. xyz = xyz + c, per component;
 *   8. y2 = y2 + (c.y * c.y), both operations rounded.
 * Then rgba8 = the reference's colour tail of xyz / (float)n_samples (what crt_read_rgba8 shows for n_samples samples).
 * d is used as given and every radiometric quantity assumes a unit vector: the caller normalises.
 * A caller ray whose o or d has a component that is NaN or of magnitude >= 3.0e38 is never walked and gets zeros in every
 * plane (crt_query_rays' rule and its reason).  A bounce ray that becomes non-finite inside a path is handled as the
 * path tracer handles it, by the loop over every primitive.
 * The context's camera does not enter, except through hit_pad (crt_debug_hit_pad: max(primitive scale, |eye|) * 2^-17),
 * which is part of the triangles' acceptance rule.  crt_set_sample_offset does not enter: the keys carry the sample
 * index.  crt_set_tile, row bands, the adaptive state and a crt_comm_partition do not enter.
 * Which walk: crt_query_rays' (the quantised 4-wide tree where the stragglers' kernel walks it, else the BVH2; shadow
 * rays primed with the light's own hit; the reference's loop under CRT_ACCEL_NONE).  The result does not depend on it,
 * nor on which lane ran a ray or what ran beside it: a ray's output is a function of its record, its key and n_samples.
 *
 * Contract: crt_query_rays', word for word where it applies.  The calls read only the scene, the lights, the spectra
 * tables and the tree: the accumulator, the framebuffer, `sample`, the counters (crt_counters counts none of these rays),
 * the frame ring, the adaptive state, the filters' state and history and the G-buffer stay as they are.  They do NOT
 * flush and give the pipeline's driver no turn.  CRT_ESTATE without a scene or an accel structure, and while the tree is
 * stale.  CRT_EINVAL for out == NULL, every plane NULL, rays == NULL with n > 0, rays, keys or xyz not 16-byte aligned,
 * n >= 2^32, n_samples == 0.  n == 0 succeeds and does nothing.
 * crt_radiance_rays (host pointers) runs on the ray queries' stream and reuses their ray staging; its own staging buffers
 * grow by at least half and are released by crt_upload_scene and crt_destroy; every allocation is made before anything is
 * enqueued, so CRT_ENOMEM enqueues nothing and writes nothing to `out`.  (Growing frees the old buffer and hipFree waits
 * for the device, as for crt_query_rays.)
 * crt_radiance_rays_device takes rays_dev, keys_dev and the pointers of *out_dev (a struct in host memory) as device
 * pointers, enqueues ONE launch on hip_stream (NULL = the null stream), allocates nothing and returns without waiting.
 * The launch keeps no state in device memory, so calls on different streams cannot disturb each other.  The caller orders
 * its reads after the launch and must have finished its calls before any call that changes the scene or the tree and
 * before crt_destroy, as for crt_query_rays_device.
 * Out of scope: caller rays through the wavefront pool; a t_max or exclude beyond the first segment; per-ray sample
 * counts; sorting or compacting rays; a frame-level form across ranks; splitting the radiance by bounce or by light. */
typedef struct { uint32_t x, y, first_sample, reserved; } crt_path_key;   /* 16 bytes; arrays 16-byte aligned; reserved = 0 */
typedef struct {
    float   *xyz;     /* n*4  sum over the samples of the path's XYZ (what crt_read_accum holds per pixel), channel 3 = +0 */
    float   *y2;      /* n    sum over the samples of Y*Y: q = q + (Y*Y), both operations rounded (DESIGN.md 6c's second moment) */
    uint8_t *rgba8;   /* n*4  the reference's colour tail of xyz / (float)n_samples (what crt_read_rgba8 shows) */
} crt_radiance_planes; /* any pointer may be NULL; all NULL is CRT_EINVAL; xyz 16-byte aligned */
int crt_radiance_rays(crt_ctx *ctx, const crt_ray *rays, const crt_path_key *keys, size_t n, uint32_t n_samples,
                      const crt_radiance_planes *out);
int crt_radiance_rays_device(crt_ctx *ctx, const crt_ray *rays_dev, const crt_path_key *keys_dev, size_t n, uint32_t n_samples,
                             const crt_radiance_planes *out_dev, void *hip_stream);
/* Test hook: the lanes G of the persistent grid a call of n rays launches (lane g owns rays g, g + G, ...). */
int crt_debug_radiance_lanes(crt_ctx *ctx, size_t n, uint64_t *out);

/* ------------------------------------------------------------------ Scene edits
 * Move the camera or edit primitives and lights of the uploaded scene in place (DESIGN.md "Scene edits"), instead of
 * crt_upload_scene + crt_build_accel.  The tree's topology is kept; crt_refit_accel recomputes its boxes on the GPU.
 * Culling never decides a hit, so the image equals the one a fresh upload and build of the edited buffers gives.
 * Rules shared by the edit calls (crt_set_camera, crt_update_primitives, crt_transform_primitives, crt_update_lights,
 * crt_remove_primitives, crt_append_primitives, crt_refit_accel):
 *   - each is a sync point (what is in flight finishes first, against the old scene);
 *   - then the frame state resets as crt_reset does: accumulator zeroed, sample 0, frame ring emptied;
 *   - tile, row bands, bound outputs, stream, options and a crt_comm_partition stay (W and H never change: every rank
 *     of a partitioned run makes the same call);
 *   - the denoise G-buffer is rebuilt on next use;
 *   - every input is validated before anything changes: on CRT_EINVAL the context is as it was.
 * Out of scope: changing a category or material, resolution changes (crt_upload_scene). */
/* camera: 16 floats as for crt_upload_scene; floats 11, 12 must equal the current width and height.  hit_pad is
 * recomputed as max(primitive scale, |eye|) * 2^-17 without scanning the primitives; a pad larger than the one the
 * tree's boxes were made with refits the tree here (the caller need not). */
int crt_set_camera(crt_ctx *ctx, const float camera[16]);
/* Replace primitive records [first, first+count) (count x 80 bytes).  Each record's index must equal its position,
 * its category and material must be unchanged, its spectrum indices < nspectra, and the range inside the scene.
 * With a tree (CRT_ACCEL_BVH2 / LBVH) the tree becomes stale: crt_trace, crt_denoise, crt_read_gbuffer and
 * crt_debug_intersect return CRT_ESTATE until crt_refit_accel or crt_build_accel.  Several updates may precede one
 * refit.  Under CRT_ACCEL_NONE nothing goes stale.
 * The history of crt_denoise_temporal is dropped, unless option "temporal_motion" is 1: then it is kept, and the first
 * update after a history slot was written first copies the records as they were (nprim x 80 bytes on the device) so that
 * the next crt_denoise_temporal can look every edited primitive's pixels up where they were ("Temporal reuse" below).
 * If that copy cannot be allocated the call returns CRT_ENOMEM with the context, the scene and the history as they were. */
int crt_update_primitives(crt_ctx *ctx, uint32_t first, uint32_t count, const void *records);
/* Move primitive ranges where they lie on the device, instead of transforming them on the host and uploading them
 * through crt_update_primitives.  One call takes any number of ops; each moves primitives
 * [first, first+count) by the row-major 3x4 matrix m.  The arithmetic is binary32, every product and sum rounded, in
 * this order:
 *   point  (x, y, z): x' = ((m0*x + m1*y) + m2*z) + m3,  y' from m4..m7,  z' from m8..m11
 *   vector (x, y, z): the same without the last addition
 *   patches and triangles: data1.xyz is a point, data2.xyz and data3.xyz are vectors
 *   spheres: data1.xyz is a point, data2.x (the radius) is multiplied by radius_scale
 * Every other byte of a record stays as it was (category, the w lanes, a sphere's unused lanes, data4).  With spheres in
 * a range the caller makes m a similarity of scale radius_scale.
 * The contract is crt_update_primitives': a sync point; the frame state resets; with a tree the tree goes stale until
 * crt_refit_accel or crt_build_accel (several calls may precede one refit); hit_pad is recomputed and equals a fresh
 * upload's; the history of crt_denoise_temporal is dropped unless option "temporal_motion" is 1, and then the records
 * are first copied as they were (CRT_ENOMEM leaves the context, the scene and the history as they were), so that the
 * temporal filters and crt_read_motion follow a transformed mesh as they follow an uploaded edit.  Light records are
 * not touched: an emitter is moved with crt_update_lights.
 * CRT_EINVAL, with the context as it was: ops NULL with n_ops > 0, a range outside the scene, two ranges that share a
 * primitive (the ops may come in any order; count 0 is allowed), a non-finite m entry or radius_scale. */
typedef struct {
    uint32_t first, count;   /* primitives [first, first+count) */
    float m[12];             /* row-major 3x4: rows (m0 m1 m2 | m3), (m4 m5 m6 | m7), (m8 m9 m10 | m11) */
    float radius_scale;      /* spheres: radius' = radius * radius_scale */
} crt_prim_transform;
int crt_transform_primitives(crt_ctx *ctx, const crt_prim_transform *ops, uint32_t n_ops);
/* Remove or append primitives of the uploaded scene on the device, instead of crt_upload_scene +
 * crt_build_accel: no record crosses the bus again but the appended ones, and tile, bound outputs, sample offset, options and a
 * crt_comm_partition stay.  The contract is crt_update_primitives'; beyond it, every allocation is made before anything
 * changes: on CRT_EINVAL or CRT_ENOMEM records, lights, tree, temporal history and accumulator are as they were, and
 * the call can be repeated.  After either call nprim, the patch count, hit_pad and the host copy of the records are
 * what a fresh upload of the resulting buffers gives; crt_update_primitives validates against the new list at once.
 * crt_remove_primitives removes the ranges (any order; they may touch; count 0 is allowed).  The survivors keep their
 * order and close ranks; each survivor's data4.w becomes its new position, every other byte of its record stays.
 * CRT_EINVAL: ranges NULL with n_ranges > 0, a range outside the scene, two ranges that share a primitive, a call that
 * would leave no primitive (the empty scene is crt_upload_scene's).
 * crt_append_primitives adds count records (80 bytes each) after the last one, validated as crt_upload_scene validates:
 * category and material in {0, 1, 2}, spectrum indices < nspectra, data4.w == nprim + k, the total below 2^28.  The
 * record array on the device has a capacity: an append that fits is a copy to its tail; one that does not moves the
 * records, device to device, to an array at least half as large again.
 * Lights: lights == NULL (then nlight must be 0) keeps the light list.  After a removal a kept light whose data4.w names
 * a primitive (is below the old nprim) has it lowered by the number of primitives removed before that one; CRT_EINVAL
 * if that primitive is itself removed -- pass the new light list.  An index at or above the old nprim is left alone.
 * With lights != NULL the list is replaced whole, with the upload's validation (nlight >= 1, emission index in range);
 * its indices are taken as given, in the new numbering; 1/area is recomputed.  So an emitter appears or goes in one call.
 * The tree: under CRT_ACCEL_NONE the packed records are re-derived here and nothing goes stale.  With a tree, a call
 * that added or removed a record leaves it TOPOLOGY-STALE: stale as after crt_update_primitives (the same calls refuse
 * with the same message), and crt_refit_accel rebuilds it with the builder that made it (*rebuilt = 1, refits back to
 * 0, the as-built quality retaken, out[9] of crt_accel_quality not counted up); crt_build_accel clears the state too.
 * Any number of edits of any kind may precede one refit.  Until then the tree's arrays belong to another primitive
 * list: crt_debug_read_accel, crt_accel_quality and crt_accel_stats return CRT_ESTATE (they keep working on an ordinarily
 * stale tree); crt_read_primitives and crt_debug_hit_pad keep working.  A call that changes no record (no live range,
 * count 0) stales the tree in the ordinary sense only, as an empty crt_transform_primitives does.
 * The history of crt_denoise_temporal is dropped, unless option "temporal_motion" is 1 and lights == NULL: then it is
 * kept; the copy of the records as the newest slot saw them is taken first if it has none, a removal compacts and
 * renumbers that copy exactly as it does the records (an unchanged record still compares equal, byte for byte), and an
 * append adds the new records to it as well, so that a pixel on an appended primitive takes the camera-only path,
 * whose key and plane tests reject what was there before.  A new light list drops the history as crt_update_lights
 * does without option "temporal_clip_pct" -- and with it too: that option keeps the history across crt_update_lights
 * alone.  Transient device memory: one more copy of the records, and one of the history's copy where it is kept. */
typedef struct { uint32_t first, count; } crt_prim_range;   /* primitives [first, first+count) */
int crt_remove_primitives(crt_ctx *ctx, const crt_prim_range *ranges, uint32_t n_ranges, const void *lights, size_t nlight);
int crt_append_primitives(crt_ctx *ctx, const void *records, uint32_t count, const void *lights, size_t nlight);
/* Primitive records [first, first+count) as they lie on the device (count x 80 bytes): after crt_transform_primitives the
 * only place where the caller sees the geometry.  A sync point like crt_read_gbuffer; it only reads, and it works on a
 * stale tree.  CRT_EINVAL for a range outside the scene or out NULL with count > 0. */
int crt_read_primitives(crt_ctx *ctx, uint32_t first, uint32_t count, void *out);
/* Replace light records [first, first+count) (count x 80 bytes, crt_upload_scene's validation; 1/area recomputed).  The
 * history of the temporal filters is dropped, unless option "temporal_clip_pct" is on: then it is kept, and the blend clips
 * what the new lighting has made stale ("Clipped history"). */
int crt_update_lights(crt_ctx *ctx, uint32_t first, uint32_t count, const void *records);
/* Recompute every box of the tree (BVH2 and 4-wide, float and quantised; the quantisation grid re-derived) from the
 * current primitives, topology kept.  Rebuilds with the builder that made the tree instead, and sets *rebuilt = 1
 * (rebuilt may be NULL), for an 8-wide tree (option "wf_width" = 8) or when the refitted boxes cannot be quantised.
 * A no-op on the tree without one.  Clears the stale state, as crt_build_accel does.
 * Option "refit_rebuild_pct" = P (below, with crt_accel_quality) also rebuilds once the refitted tree has decayed. */
int crt_refit_accel(crt_ctx *ctx, int *rebuilt);
/* The surface-area cost of the trees as they lie on the device, so that a caller who refits frame after frame can tell
 * when a refitted tree has become worse than a fresh one.  All arithmetic is binary64 on box values
 * converted from what the device holds.  A(box) = dx*dy + dy*dz + dz*dx with d = hi - lo, summed in that order.
 *   BVH2 (16 floats per node: c0.lo c0.hi c1.lo c1.hi ref0 ref1): the box of inner node i is the union of its two child
 *     boxes, the root box is the root node's;  boxes2 = sum over inner nodes of 2 A(box_i) / A(root),
 *     prims2 = sum over leaf children of count A(child box) / A(root)  (a leaf is ref < 0, ~ref = first << 3 | count - 1).
 *   The 4-wide tree the wavefront kernels walk, float (32 floats per node) or quantised (16 dwords per node; where both
 *     exist, the quantised one): an empty slot has ref == 0 and is skipped; a quantised plane is
 *     (double)base[a] + (double)q * (double)scale[a] (the product is exact, so the value is one rounded sum); the box of
 *     node i is the union of its nch_i live child boxes;  boxes4 = sum over nodes of nch_i A(box_i) / A(root),
 *     prims4 = sum over leaf children of count A(child box) / A(root).
 * A union takes the smaller lo and the larger hi per axis (fmin / fmax).  The sums run over the dense node arrays in a
 * fixed order without atomics (two calls on the same tree return the same bits) and are divided by A(root) once, at the
 * end; boxes2 is twice the SAH cost of DESIGN.md 3.  A tree with no inner node (one leaf) and CRT_ACCEL_NONE: all four
 * values are 0.  Where the wavefront kernels walk the 8-wide tree (option "wf_width" = 8, where a refit already
 * rebuilds) boxes4 and prims4 are NaN.  Non-finite boxes give non-finite values, reported as they come.
 *   out[0] boxes2  [1] prims2  [2] boxes4  [3] prims4 -- the tree as it lies on the device now
 *   out[4..7] the same four for the tree as it was built (before any refit)
 *   out[8] refits since the tree was built    [9] rebuilds "refit_rebuild_pct" has made since crt_create
 *   out[10] 1 = [2], [3], [6], [7] are present (0: the 8-wide tree is walked and they are NaN)    [11] 0
 * The as-built values are taken from the untouched tree by the first refit after a build, or by the first
 * crt_accel_quality, and kept until the next build (crt_build_accel, an upload, any rebuild by crt_refit_accel);
 * crt_build_accel itself computes nothing.  A sync point.  It only reads, and it works on a stale tree, whose boxes it
 * shows as they are (like crt_debug_read_accel).  CRT_ESTATE without a scene or accel structure.
 * Option "refit_rebuild_pct" = P: 0 (default) = off; 100..100000; anything else is CRT_EINVAL.  With P != 0,
 * crt_refit_accel, after it has refitted, computes Q = boxes + prims of the walked tree (the 4-wide tree where there is
 * one, else the BVH2).  If Q_now > Q_built * P / 100, both finite, it rebuilds with the builder that made the tree (the
 * path of the 8-wide and unquantisable cases), sets *rebuilt = 1, takes the new tree's values as the as-built ones and
 * adds one to out[9].  A non-finite Q on either side means no action.  The refit inside crt_set_camera does not apply
 * the policy.  With P = 0 crt_refit_accel launches what it launched before the option existed (the first refit of a
 * tree also takes the as-built values, once). */
int crt_accel_quality(crt_ctx *ctx, double out[12]);
/* Test hook: the hit_pad the kernels use. */
int crt_debug_hit_pad(crt_ctx *ctx, float *out);

/* ------------------------------------------------------------------ Adaptive sampling
 * Per 8x8 tile of the context's rectangle: stop sampling the tiles that have converged.  Sample s of pixel
 * (x, y) depends on (x, y, s) only, so a pixel of a tile that holds n samples holds exactly the accumulator of a uniform
 * render of n samples, whatever the other tiles hold; its rgba8 is tone-mapped with its tile's count.
 * A tile's error E is the largest, over its pixels, of the standard error of the mean luminance Y, times the slope of the
 * exposure curve 1 - exp(-2.2 Y) at that mean (NaN counts as +inf; E = +inf below 2 samples).  Tile t holding n_t
 * samples is ACTIVE iff (max_samples == 0 || n_t < max_samples) && (n_t < min_samples || !(E_t <= threshold)).
 * crt_trace_adaptive finishes what is in flight, selects the active tiles on the GPU (reading back their number, 4 bytes),
 * enqueues `samples` more samples for each of them (samples n_t + 1 .. n_t + samples) and returns without waiting for them,
 * like crt_trace.  Tiles that are not active are not touched.
 * State: the first successful call puts the context into the ADAPTIVE state; it needs sample 0 (after crt_reset, an upload
 * or an edit; else CRT_ESTATE).  Every call that zeroes or replaces the accumulator (crt_reset, crt_write_accum,
 * crt_upload_scene, crt_set_tile, crt_set_row_bands, the scene edits) returns to the uniform state; crt_build_accel keeps it.
 * In the adaptive state crt_trace, crt_sample_count, crt_read_latest_rgba8, crt_latest_sample, crt_read_sample_rgba8 and
 * crt_denoise return CRT_ESTATE; crt_read_accum / crt_read_rgba8 / crt_bind_output / counters keep working, and
 * crt_denoise_adaptive (below) is the preview filter of this state.
 * CRT_ESTATE also under a crt_comm_partition whose 8x8 tiles are not the frame's (strips, bands that are no multiple of 8
 * rows; "The frame of a partition" below), and without a scene / accel structure or with a stale tree.  CRT_EINVAL (the
 * context unchanged) for samples == 0, a negative or non-finite threshold, or max_samples != 0 && max_samples < min_samples. */
typedef struct {
    uint32_t samples;      /* samples added to every ACTIVE tile by this call, >= 1                    */
    uint32_t min_samples;  /* a tile below this count is active whatever its error                      */
    uint32_t max_samples;  /* a tile at or above this count is never active; 0 = no limit               */
    float threshold;       /* converged when the tile's error <= threshold; finite and >= 0              */
} crt_adaptive_params;
/* NULL = the defaults (crt_adaptive_defaults).  *active_tiles (may be NULL) = tiles sampled by this call; 0 = nothing
 * enqueued.  A call that fails after some of its samples were enqueued leaves the counts behind the accumulator: the
 * context then refuses crt_trace_adaptive / crt_read_adaptive (CRT_ESTATE) until crt_reset. */
int crt_trace_adaptive(crt_ctx *ctx, const crt_adaptive_params *params, uint32_t *active_tiles);
/* The defaults {samples 64, min_samples 32, max_samples 4096, threshold 0.01}: the bindings start from what this returns
 * (DESIGN.md 6c has the measurements they were chosen by).  No context needed. */
int crt_adaptive_defaults(crt_adaptive_params *out);
/* Per 8x8 tile of the context's rectangle, row-major, tiles_x = ceil(tw/8), tiles_y = ceil(th/8):
 * counts = samples the tile holds, errors = the tile's error E as the NEXT crt_trace_adaptive will judge it.
 * Either pointer may be NULL.  A sync point.  CRT_ESTATE in the uniform state. */
int crt_read_adaptive(crt_ctx *ctx, uint32_t *counts, float *errors);

/* ------------------------------------------------------------------ Denoised preview of an adaptive render
 * crt_denoise_adaptive is crt_denoise for the ADAPTIVE state (DESIGN.md 6d defines it): the same a-trous filter, guides
 * and G-buffer, with each pixel averaged by its tile's count, and with the colour edge-stopping weight scaled by the
 * pixels' own noise instead of a fixed sigma_color.  The variance v of a pixel is the square of the pixel error of
 * "Adaptive sampling" (the standard error of its mean luminance times the slope of the exposure curve; v = 1 below 2
 * samples or where that square is not finite); the colour term of a tap q of pixel p is
 * |T(c_p) - T(c_q)|^2 / (sigma_variance^2 (v~_p + v~_q) + (0.5/255)^2), v~ a 3x3 blur of v, and v is carried through
 * the filter (v' = sum w^2 v / (sum w)^2), so a pixel that has converged is left alone and later passes narrow by
 * themselves.  Below about 8 samples per pixel the variance estimate is itself too noisy and crt_denoise on a uniform
 * render is a little better (DESIGN.md 6d has the numbers): crt_denoise stays the preview of the first frames.
 * A sync point like crt_read_rgba8.  It only READS the accumulator, the second moments and the counts: accumulator,
 * rgba8 framebuffer, counts, errors, counters and the adaptive state stay as they are, and the next crt_trace_adaptive
 * continues bit for bit.  CRT_ESTATE in the uniform state (crt_denoise filters a uniform render; crt_trace_adaptive with
 * min_samples == max_samples gives this filter a uniform one), after a crt_trace_adaptive that failed part way, without
 * a scene or accel structure, with a stale tree, or under a row-band partition (crt_denoise_adaptive_frame filters the
 * gathered frame instead).  A crt_set_tile rectangle is filtered on its own. */
typedef struct {
    uint32_t iterations;    /* 0..10, step 2^i in pass i; 0 = the plain per-tile average, as crt_read_rgba8 */
    float sigma_variance;   /* colour edge-stopping scale in standard errors; > 0 and finite */
    float sigma_normal;     /* as crt_denoise_params */
    float sigma_plane;
} crt_denoise_adaptive_params;
/* The defaults {5, 8.0, 0.5, 0.3}.  No context and no GPU needed. */
int crt_denoise_adaptive_defaults(crt_denoise_adaptive_params *out);
/* NULL params = the defaults.  rgb_out: tw*th*4 floats (linear rgb; channel 3 = the pixel's var_out) or NULL;
 * rgba8_out: tw*th*4 bytes or NULL; var_out: tw*th floats, the variance left after filtering (display units squared),
 * or NULL.  CRT_EINVAL (the context unchanged) for iterations > 10 or a sigma that is not positive and finite. */
int crt_denoise_adaptive(crt_ctx *ctx, const crt_denoise_adaptive_params *params, float *rgb_out, uint8_t *rgba8_out,
                         float *var_out);

/* ------------------------------------------------------------------ Adaptive sampling judged by the filtered preview
 * crt_trace_adaptive_filtered is crt_trace_adaptive with the tile's error taken from what crt_denoise_adaptive leaves
 * (DESIGN.md 6k): an adaptive render that is shown through that filter keeps sampling only where the FILTERED image is
 * still noisy.  For filter parameters D (NULL = crt_denoise_adaptive_defaults) and tile t holding n_t samples:
 *   v'_p  is, bit for bit, what crt_denoise_adaptive(ctx, D, ..., var_out) returns for pixel p in the same state;
 *   E'_t  = sqrt(max over the tile's in-frame pixels of v'_p): a NaN counts as +inf, the square root is one IEEE
 *           operation taken once, of the maximum; E'_t = +inf where n_t < 2;
 *   ACTIVE iff (max_samples == 0 || n_t < max_samples) && (n_t < min_samples || !(E'_t <= threshold)).
 * E' is in the display units of E, so `threshold` keeps its meaning and crt_adaptive_defaults stays the NULL default;
 * the filter averages noise away, so E' <= about E and a given threshold stops earlier.  min_samples matters more than
 * under crt_trace_adaptive: below about 8 samples per pixel the variance estimate that guides the filter is itself too
 * noisy (see crt_denoise_adaptive), and a tile that stops there stops on an unreliable E'.
 * E' of a tile depends on its neighbours through the filter, so a tile that was at rest may become active again.
 * What it buys (DESIGN.md 6k has the numbers): on the Cornell box, large smooth surfaces, the filtered preview has
 * 0.75 times the error of crt_trace_adaptive's at the same 30 samples per pixel.  On S2 (atrium250k, small triangles
 * everywhere) it buys NOTHING: both rules lie on one error-against-samples curve within 5 %, the new one needs more
 * rounds, and its selection costs 1.14 ms a call at 1920x1080 against 0.05 ms (the filter's K = 5 launches; under 2 % of
 * a 64-sample round).  crt_trace_adaptive stays the rule to start from.
 * State machine, batches, commit, the failed-part-way state and the "adaptive_temporal" / sample-offset rules are
 * crt_trace_adaptive's; the two calls may be mixed within one adaptive state.  The call that enters the adaptive state
 * runs no filter (every tile is active); every later one enqueues the filter's launches on the context's stream before
 * the selection and reads back the same 4 bytes.  It only READS the denoise state: the temporal history stays untouched.
 * A crt_set_tile rectangle is filtered and selected on its own.
 * Beyond crt_trace_adaptive's refusals: CRT_ESTATE where crt_denoise_adaptive refuses, namely under row bands and hence
 * under every crt_comm_partition; CRT_EINVAL for filter parameters crt_denoise_adaptive rejects; CRT_ENOMEM when a filter
 * buffer cannot be allocated.  In all three cases nothing is enqueued and the context, counts and accumulator stay as
 * they were. */
int crt_trace_adaptive_filtered(crt_ctx *ctx, const crt_adaptive_params *params, const crt_denoise_adaptive_params *filter,
                                uint32_t *active_tiles);
/* crt_read_adaptive with errors = E' as the NEXT crt_trace_adaptive_filtered with this filter will judge it (counts are
 * crt_read_adaptive's; crt_read_adaptive keeps returning E).  A sync point that only reads.  CRT_ESTATE in the uniform
 * state, after a call that failed part way, and where the filter refuses; CRT_EINVAL for the filter's parameters. */
int crt_read_adaptive_filtered(crt_ctx *ctx, const crt_denoise_adaptive_params *filter, uint32_t *counts, float *errors);

/* ------------------------------------------------------------------ The frame of a partition: adaptive sampling and previews
 * Across a partition the three families work together:
 *
 * crt_trace_adaptive works under a partition made with band_rows > 0 and band_rows % 8 == 0: every local 8x8 tile is then
 * one of the frame's, the last tile row partial exactly where the image's is.  Each rank selects, traces and commits its
 * own tiles as an unpartitioned context does for those tiles (*active_tiles is the rank's own number; a rank without an
 * active tile enqueues nothing and still takes part in the gathers), and the assembled frame is the unpartitioned
 * context's bit for bit.  Contiguous strips and other bands keep refusing (CRT_ESTATE).  Rows are not rebalanced between
 * ranks as tiles retire.
 *
 * crt_gather(ctx, CRT_GATHER_PREVIEW [| CRT_GATHER_RGBA8]) ships what the frame-level calls below need.  Unlike the other
 * two flags it is a sync point for this context: it finishes what is in flight, as crt_read_adaptive does, then posts on
 * the context's stream the gather of the accumulator (the CRT_GATHER_ACCUM one: crt_read_frame_accum sees it too) and,
 * in the adaptive state, those of the second moment Q (4 bytes per pixel) and of the tile counts (4 bytes per tile; the
 * tile grid is partitioned by crt_layout_rows(ceil(H/8), band_rows/8, world, rank)).  The state, the uniform sample count
 * and the epoch of the context's frame state are recorded with it.  With CRT_COMM_LOCAL a rank whose state or sample
 * count differs from a peer's that has posted the same gather gets CRT_EINVAL ("the ranks disagree") and posts nothing;
 * once it holds what its peers hold it gathers again.  CRT_ESTATE after a crt_trace_adaptive that failed part way.
 *
 * The three calls below work on ANY rank, over the whole W x H frame of the latest PREVIEW gather, with this rank's own
 * replica of the scene and tree; the outputs are W x H (crt_read_frame_adaptive: the frame's tile grid, ceil(W/8) x
 * ceil(H/8), row-major; either pointer may be NULL; the errors are crt_read_adaptive's kernel run over the assembled
 * accumulator, Q and counts).  crt_denoise_frame is crt_denoise, crt_denoise_adaptive_frame is crt_denoise_adaptive, of
 * the frame: the same launches over a frame-sized view, so they equal what one unpartitioned context returns after the
 * same calls, bit for bit -- under strips too, where they remove the seams of the per-strip filter.  They own frame-sized
 * guide and colour buffers apart from the per-context filters'; the frame's G-buffer is built on first use and kept until
 * the scene, the tree, the camera or the partition changes.  There is no temporal history at frame level:
 * crt_denoise_temporal, crt_denoise_svgf and crt_read_motion stay per context (and keep refusing under row bands).
 * All three are sync points that only read: accumulator, strips, counts, counters, the adaptive state and the per-context
 * denoise state stay as they are, and the next crt_trace / crt_trace_adaptive continues bit for bit.
 * They refuse, with nothing enqueued and nothing written: CRT_ESTATE without a communicator or with a stale partition;
 * without a PREVIEW gather since crt_comm_partition; while a peer of a local group has not posted its PREVIEW gather; when
 * the gathered state is not the one the call is for (crt_denoise_frame: uniform; the other two: adaptive); when the
 * context's frame state was zeroed or replaced since the gather (crt_reset, crt_set_camera, an edit, crt_write_accum:
 * "gather again"), or the accumulator alone was gathered again; without a scene or tree, or with a stale tree;
 * crt_denoise_frame at n == 0.  CRT_EINVAL for what the per-context filters reject (iterations > 10, a bad sigma).
 * CRT_ENOMEM when one of the frame-sized buffers cannot be allocated; the next call tries again.
 * NULL params = the per-context defaults. */
int crt_read_frame_adaptive(crt_ctx *ctx, uint32_t *counts, float *errors);
int crt_denoise_frame(crt_ctx *ctx, const crt_denoise_params *params, float *rgb_out /* W*H*4 floats */, uint8_t *rgba8_out /* W*H*4 */);
int crt_denoise_adaptive_frame(crt_ctx *ctx, const crt_denoise_adaptive_params *params, float *rgb_out, uint8_t *rgba8_out,
                               float *var_out /* W*H floats */);

/* ------------------------------------------------------------------ Sample offset
 * Sample s of pixel (x, y) is seeded by (x, y, s) only, and every frame after a reset draws samples 1..n again: the
 * noise of consecutive frames of a moving camera is the same pattern in screen space, and averaging them over time
 * gains almost nothing.  With offset B the j-th sample of the frame (j = 1, 2, ...) is drawn with the reference's
 * sample index B + j (its seed and its stratum (B + j) % 16); everything that COUNTS samples keeps counting from the
 * reset: crt_sample_count, the tone map's divisor, the indices of the frame ring, the n of crt_denoise.  A frame of n
 * samples is bit for bit the reference's samples B+1 .. B+n summed into a zero accumulator.
 * The offset may be set only at sample 0 in the uniform state (else CRT_ESTATE); it persists over crt_reset and the
 * scene edits, crt_upload_scene returns it to 0, and crt_write_accum(in, s) continues at index B + s + 1.  crt_trace
 * returns CRT_EINVAL if B plus the samples requested since the reset would pass 2^32 - 1.  Wavefront pipeline only: with
 * a non-zero offset crt_trace under "pipeline" = 0 or CRT_ACCEL_NONE, and crt_trace_adaptive, return CRT_ESTATE.
 * Offset 0 (the default) is the behaviour without this call.
 * With option "adaptive_temporal" = 1 (default 0) crt_trace_adaptive takes the offset too: sample j of a tile (j = n_t + 1,
 * n_t + 2, ...) is drawn with the reference's index B + j, while the counts, the tone map's divisor and E keep counting
 * from the reset; each pixel then holds the reference's samples B+1 .. B+n_t of its tile's count n_t, bit for bit.  With
 * B != 0 it is the wavefront pipeline's alone (CRT_ESTATE under "pipeline" = 0 or CRT_ACCEL_NONE, as crt_trace), and
 * CRT_EINVAL, the context unchanged, if B plus the samples that the crt_trace_adaptive calls of this adaptive state have
 * requested, this call's included, would pass 2^32 - 1 (that sum bounds every tile's count).  The offset is still set at
 * sample 0 in the uniform state: crt_set_camera, crt_set_sample_offset, then the adaptive rounds. */
int crt_set_sample_offset(crt_ctx *ctx, uint32_t offset);
int crt_sample_offset(crt_ctx *ctx, uint32_t *out);

/* ------------------------------------------------------------------ Temporal reuse across camera moves
 * Every camera move zeroes the accumulator, so crt_denoise filters each frame of an orbit from that frame's few samples
 * alone.  crt_denoise_temporal first blends the frame with the previous frame's result, reprojected through the first-hit
 * G-buffer -- the temporal half of SVGF (Schied et al. 2017; DESIGN.md 6e defines it operation by operation) -- and then
 * runs crt_denoise's a-trous passes on the blend.  Give consecutive frames distinct samples (crt_set_sample_offset):
 * with the same samples every frame there is nothing to gain.
 * The context keeps two history slots over its rectangle, PREVIOUS and CURRENT: the blended linear rgb before any
 * spatial filter with its weight Hw in samples, that frame's G-buffer and keys, and its camera.  A FRAME is the span
 * between two events that zero the accumulator.  The first crt_denoise_temporal of a new frame promotes CURRENT to
 * PREVIOUS; further calls in the same frame (after more samples, say) blend against the same PREVIOUS and overwrite
 * CURRENT, so calling twice is idempotent.  History survives crt_set_camera, crt_reset, crt_build_accel and a
 * crt_refit_accel with no primitive update before it; it is dropped by crt_upload_scene, crt_set_tile,
 * crt_set_row_bands, crt_comm_partition, crt_update_primitives, crt_transform_primitives, crt_update_lights,
 * crt_write_accum and crt_denoise_temporal_reset.
 * Moving geometry: with option "temporal_motion" = 1 (default 0) crt_update_primitives and crt_transform_primitives keep
 * the history, and the next
 * crt_denoise_temporal reprojects every pixel whose primitive's record changed through that primitive's previous record
 * (DESIGN.md 6f): the hit keeps its coordinates in the primitive (a patch's or triangle's edge coordinates, a sphere's
 * direction from the centre), x_p and n_p become the position x~ and normal n~ they had in the old pose, and x~, n~ take
 * x_p's, n_p's place in the projection and in the taps' tests.  A pixel whose record is bitwise unchanged takes the path
 * below exactly; one whose emission or reflectance index changed, or whose old record is degenerate, takes no history.
 * crt_update_lights drops the history in both modes (it changes what every surface receives), and lighting that changed
 * because something else moved (a shadow sliding over a static floor) is stale history until the blend outweighs it --
 * unless option "temporal_clip_pct" is on ("Clipped history" below): it clips such history, and keeps it across
 * crt_update_lights.
 * Setting the option back to 0 after such an edit drops the history.
 * Per pixel p with first hit x_p, normal n_p and key: no history is taken where there is no PREVIOUS, at a miss, on
 * glass (view-dependent) or where the pixel's own colour is not finite.  Otherwise x_p is projected into the previous
 * camera; each of the four bilinear taps q there is reused iff it lies inside the rectangle, has the same key, holds
 * finite history, |n_p - n_q|^2 <= normal_tol^2 and |n_p . (x_q - x_p)| <= plane_tol * r_p, r_p the larger of the
 * pixel's footprints at x_p in the two cameras.  With h and Hp the weighted means of the taps' colour and weight,
 * Hp capped at max_history: c = (n c_new + Hp h) / (n + Hp), Hw = n + Hp; without an accepted tap c = c_new, Hw = n.
 * A sync point like crt_denoise, and it only READS the accumulator and the sample count: accumulator, rgba8
 * framebuffer, counters and frame ring stay as they are and the next crt_trace continues bit for bit.  CRT_ESTATE where
 * crt_denoise returns it (no scene or tree, a stale tree, sample 0, row bands, the adaptive state).  A crt_set_tile
 * rectangle is filtered on its own.
 * The adaptive state: with option "adaptive_temporal" = 1 (default 0) crt_denoise_temporal, crt_denoise_svgf,
 * crt_read_motion and crt_debug_read_moments accept the adaptive state, and refuse it after a
 * crt_trace_adaptive that failed part way, as crt_denoise_adaptive does.  The definition is the one above and that of
 * "Variance-guided temporal filter" with one substitution: wherever n stands for pixel p it is n_p, the count of p's 8x8
 * tile as a float -- in c_new = M (accum / n_p) and y = accum.y / n_p, in Hw = n_p + Hp and c = (n_p c_new + Hp h) / Hw, in
 * Mw = n_p + Mp and the merge of the moments, and in F = Mw / n_p.  Taps, tests, weights, caps, passes, slots, promotion,
 * frame notion, "temporal_motion" and outputs are unchanged, and where every tile holds the same count the calls return
 * what they return for a uniform render of that count, bit for bit.  Entering or leaving the adaptive state drops no
 * history: a uniform frame may precede an adaptive one and the reverse.  Setting the option back to 0 makes the calls
 * refuse the adaptive state again and drops nothing.  Row bands keep refusing. */
typedef struct {
    uint32_t iterations;    /* a-trous passes after the blend, 0..10 */
    float sigma_color;      /* as crt_denoise_params */
    float sigma_normal;
    float sigma_plane;
    float max_history;      /* cap, in samples, on the weight of reused history; > 0 and finite */
    float normal_tol;       /* a tap is reused if |n_p - n_q|^2 <= normal_tol^2 ... */
    float plane_tol;        /* ... and |n_p . (x_q - x_p)| <= plane_tol * pixel footprint at x_p */
} crt_denoise_temporal_params;
/* The defaults {5, 1.0, 0.5, 0.3, 64, 0.5, 2.0}.  No context and no GPU needed. */
int crt_denoise_temporal_defaults(crt_denoise_temporal_params *out);
/* NULL params = the defaults.  rgb_out: tw*th*4 floats (linear rgb; channel 3 = Hw) or NULL; rgba8_out: tw*th*4 bytes
 * or NULL; history_out: tw*th floats of Hw (n where nothing was reused) or NULL.  CRT_EINVAL (context and history
 * unchanged) for iterations > 10 or a sigma, tolerance or max_history that is not positive and finite. */
int crt_denoise_temporal(crt_ctx *ctx, const crt_denoise_temporal_params *params, float *rgb_out, uint8_t *rgba8_out,
                         float *history_out);
/* Drop the history: the next crt_denoise_temporal equals crt_denoise. */
int crt_denoise_temporal_reset(crt_ctx *ctx);
/* Motion vectors: per pixel of the rectangle the film position (u, v), in the rectangle's own pixel coordinates, where
 * the blend of the last crt_denoise_temporal looked for that pixel in the PREVIOUS slot (the binary64 value rounded to
 * float; out: tw*th*2 floats) -- what an external denoiser or encoder asks for.  (NaN, NaN) where no position exists:
 * no PREVIOUS slot, a miss, glass, a depth in the previous camera that is <= 0 or not finite, or a map of
 * "temporal_motion" that refuses.  Positions outside the rectangle are reported as they are.  With "temporal_motion" off
 * it is the camera-only reprojection.  A sync point like crt_read_gbuffer, and it only reads.  CRT_ESTATE where
 * crt_denoise_temporal returns it, and when no crt_denoise_temporal has run since the accumulator was last zeroed. */
int crt_read_motion(crt_ctx *ctx, float *out);

/* ------------------------------------------------------------------ Variance-guided temporal filter
 * crt_denoise_temporal's filter does not know how far its input has converged: a pixel holding 64 samples of history is
 * blurred as hard as one holding 4.  crt_denoise_svgf is the same blend followed by crt_denoise_adaptive's variance-guided
 * passes, with the variance taken from the spread of the frame means over time -- SVGF's temporal moments (DESIGN.md 6g
 * defines it operation by operation).  Each history slot gains a second plane (m1, s, Mw, 0) per pixel: the mean
 * luminance, the weighted population variance of the frame means, and the weight in samples behind both.  With
 * y = accum.y / n: a pixel that takes no history, or whose PREVIOUS slot has no moments, starts at m1 = y, s = 0, Mw = n;
 * otherwise, over the accepted taps and weights of the colour blend, h1, hs and Mp (capped at max_history) are the means
 * of the taps' m1, s and Mw, and Mw = n + Mp, m1 = (n y + Mp h1) / Mw, s = (Mp / Mw) hs + n Mp (y - h1)^2 / Mw^2.
 * With F = Mw / n frames behind the pixel its variance in display units is v = g^2 s / (F - 1), g = 2.2 exp(-2.2 max(m1, 0))
 * the exposure curve's slope, where F >= min_frames and v is finite, and v = 1 ("nothing known", as crt_denoise_adaptive
 * below 2 samples) elsewhere: misses, glass and pixels without history.  The passes are crt_denoise_adaptive's on (c, v).
 * The slots, the promotion, the events that keep or drop the history, the frame notion, "temporal_motion" and the
 * contract (a sync point, reads only, CRT_ESTATE in the same places) are crt_denoise_temporal's, and what it leaves in
 * CURRENT's colour plane is bit for bit what crt_denoise_temporal leaves there.  The two calls mix: a
 * crt_denoise_temporal writes CURRENT without moments, and a later crt_denoise_svgf reuses its colour history and starts
 * the moments again (Mw = n).  A failed allocation (CRT_ENOMEM) leaves the slots as they were.
 *
 * Option "svgf_spatial_pct" = P (default 0 = off; 25..10000; anything else is CRT_EINVAL): v = 1 is a very
 * wide colour term, and it is what every pixel carries on the first min_frames - 1 frames after the history was dropped and
 * what every disoccluded pixel carries afterwards.  With P != 0 a pixel whose v is not known from the moments (F <
 * min_frames, or a value that is not finite) and that is neither a miss nor glass takes a spatial estimate instead, from its
 * 7x7 neighbourhood at unit step: over the taps q inside the rectangle with the pixel's key and finite m1, Mw > 0, weighted
 * with the filter's normal and plane terms w_q (no colour term; w = 1 at the centre), A = sum w, mu = sum w Mw_q m1_q /
 * sum w Mw_q, sigma^2 = sum w Mw_q (m1_q - mu)^2 / (A - 1) -- each m1_q is a mean over Mw_q samples, so this is the
 * variance per sample -- and v = (P / 100) g(mu)^2 sigma^2 / Mw_p where A >= 4 and the value is finite, v = 1 elsewhere.
 * Only the v that enters the passes changes (at iterations = 0 that is var_out and rgb_out's channel 3): what the call
 * leaves in CURRENT -- colour, Hw, moments -- is bit for bit what it leaves with P = 0, so the history never depends on the
 * option, the option may change between frames, and the pixels whose v is known keep it bit for bit.
 * crt_denoise_temporal and crt_denoise_adaptive ignore the option.  It costs 0-3 % of quality on frames where most pixels
 * are known and 9 % on the very first frame, and gains up to 24 % on the frames between, on scenes whose surfaces are
 * large against the window; on a finely detailed scene (S2) it made the preview worse at every P measured, and
 * crt_denoise_temporal stays the better preview there: DESIGN.md 6j has the tables. */
typedef struct {
    uint32_t iterations;    /* variance-guided passes after the blend, 0..10 */
    float sigma_variance;   /* as crt_denoise_adaptive_params */
    float sigma_normal;
    float sigma_plane;
    float max_history;      /* as crt_denoise_temporal_params */
    float normal_tol;
    float plane_tol;
    float min_frames;       /* the variance is trusted from this many frames of history on; >= 2 and finite */
} crt_denoise_svgf_params;
/* The defaults {5, 4.0, 0.5, 0.3, 64, 0.5, 2.0, 4.0}.  No context and no GPU needed. */
int crt_denoise_svgf_defaults(crt_denoise_svgf_params *out);
/* NULL params = the defaults.  rgb_out: tw*th*4 floats (linear rgb; channel 3 = the pixel's var_out) or NULL; rgba8_out:
 * tw*th*4 bytes or NULL; history_out: tw*th floats of Hw or NULL; var_out: tw*th floats, the variance left after
 * filtering (v itself at iterations = 0), or NULL.  CRT_EINVAL (context, history and moments unchanged) for
 * iterations > 10, a sigma, tolerance or max_history that is not positive and finite, or min_frames < 2 or not finite. */
int crt_denoise_svgf(crt_ctx *ctx, const crt_denoise_svgf_params *params, float *rgb_out, uint8_t *rgba8_out,
                     float *history_out, float *var_out);
/* Test hook: the moments (m1, s, Mw, 0) of the CURRENT slot, tw*th*4 floats.  CRT_ESTATE unless CURRENT belongs to this
 * frame and carries moments (no crt_denoise_svgf in this frame yet, or a crt_denoise_temporal after it). */
int crt_debug_read_moments(crt_ctx *ctx, float *out);

/* ------------------------------------------------------------------ Clipped history
 * The temporal filters reuse a pixel's history when the SURFACE is the same; they cannot tell when the LIGHTING on it has
 * changed (a shadow that slid on, a light that was dimmed).  Option "temporal_clip_pct" = P (default 0 = off; 25..10000;
 * anything else is CRT_EINVAL and the option keeps its value; DESIGN.md 6l defines it operation by operation) clips the
 * reprojected history to the colour statistics of the frame's own neighbourhood -- variance clipping -- in
 * crt_denoise_temporal and crt_denoise_svgf; every other filter ignores it.  With gamma = (float)P / 100:
 * every pixel p that is neither a miss nor glass and whose own c_new = M (accum / n) is finite has a BOX.  Its taps are the
 * pixels q with |dx|, |dy| <= 3 inside the rectangle (a crt_set_tile rectangle's edges are image borders) whose key equals
 * p's and whose c_new_q (with q's own n in the adaptive state) is finite in all three channels; p itself is one.  Per
 * channel, in binary32, row-major over the taps: N their number, mu = (sum c_q) / N, in a second pass
 * S = sum (c_q - mu)^2, sigma = sqrt(S / N), lo = mu - gamma sigma, hi = mu + gamma sigma.  No geometric weights: a same-key
 * neighbour across a crease only widens the box.  The box is VALID iff N >= 4 and all six bounds are finite.
 * In the blend of "Temporal reuse", a pixel with an accepted tap and a valid box takes h' = min(max(h, lo), hi) per channel
 * for h; taps, tests, Hp, Hw, the moments, the spatial variance estimate, "temporal_motion", crt_read_motion and the
 * promotion of the slots are unchanged, and Hw, moments and motion are bit for bit those of P = 0.  CURRENT keeps the
 * clipped blend, so the next frame's history is already rectified; a relit pixel's moments see a large (y - h1)^2, its v
 * rises, and crt_denoise_svgf's passes blur it more for a few frames: that is intended.
 * Lights: with P != 0 crt_update_lights keeps the history (both slots, the moments, any geometry snapshot); setting the
 * option back to 0 after such an edit drops it, as "temporal_motion" going back to 0 does after a primitive edit.
 * crt_remove_primitives and crt_append_primitives with a new light list keep dropping it.
 * It costs one more pass over the frame (96 bytes per pixel on the device while the option is on; CRT_ENOMEM leaves the
 * slots as they were) and, where nothing changed, some of the history's benefit: a box from 4 samples per pixel is narrower
 * than the noise of its own mean.  DESIGN.md 6l has the tables.  With 0 every call launches what it launches without the
 * option.
 * Test hook: per pixel lo.rgb, N, hi.rgb, valid (1.0 / 0.0) of the last temporal call of this frame, tw*th*8 floats; a
 * pixel without a box reports N = 0, valid = 0.  A sync point, and it only reads.  CRT_ESTATE unless that call ran the box
 * pass (the option on and a usable PREVIOUS slot); CRT_EINVAL for NULL. */
int crt_debug_read_clip_box(crt_ctx *ctx, float *out /* tw*th*8 floats */);

/* Counters accumulate over crt_trace calls while enabled (off by default: the
 * counting kernel variant is slower). */
int crt_enable_counters(crt_ctx *ctx, int on);
int crt_counters(crt_ctx *ctx, uint64_t out[CRT_NCOUNTERS]);
int crt_reset_counters(crt_ctx *ctx);

/* Device time from the start of the LAST crt_trace call to the end of its work
 * (HIP events on the context's stream; finishes the call's parked paths first),
 * and how many kernel launches that was. */
int crt_last_trace_ms(crt_ctx *ctx, float *ms, uint32_t *launches);

/* Device time of the DOMINANT kernel's launches, summed, and their number: the BVH traversal
 * kernel k_wf_trace of the wavefront pipeline -- every launch since the previous query (or
 * since option "time_kernels" was set: 1 brackets each launch with HIP events on the
 * stream it runs on, N > 1 also creates the event pairs for N launches up front) -- or the single trace kernel of the last crt_trace call in the
 * "pipeline"=0 form.  Syncs. */
int crt_last_kernel_ms(crt_ctx *ctx, float *ms, uint32_t *launches);

/* Tuning knobs.  "spp_per_launch": samples fused per batch (0 = default);
 * "pipeline": 1 = wavefront (default), 0 = single megakernel; "wf_pool": path slots
 * (0 = auto: a quarter of a batch, at least "wf_pool_spp" (8) slots per tile pixel, 1 M..24 M); "wf_waves_per_cu": persistent traversal
 * waves per CU and pipe; "wf_pipes": sub-pools on separate streams (1..4); "wf_defer": 0 = every crt_trace
 * call runs its paths to the end; "wf_ring" (2..32 batches in flight), "wf_cohort" (samples per batch that small calls are merged up to), "wf_chunk" (iterations enqueued at
 * a time), "wf_ahead" (iterations in flight per pipe before the call waits), "wf_feed_pct", "wf_finish_at",
 * "wf_flush_at", "wf_side_ppw", "wf_flush_ppw", "wf_tail_walk": pipeline tuning;
 * "quantize", "wf_width" (4 | 8: node width of the wavefront traversal; at crt_build_accel);
 * "wf_trace_form" (2: ray ring + primitive tasks, default; 1: the first traversal kernel); "wf_cull_miss" (1, default:
 * work chunks whose camera rays all miss the tree's root boxes are finished where they are generated and take no path
 * slot; 0: every camera ray goes through the pool; same image and counters either way); "wf_cull_classes" (1, default:
 * where "wf_cull_miss" acts, the tiles whose camera rays miss, or enter, the root's boxes for EVERY sample are classified
 * once per run, and their chunks skip the per-sample test -- and, where they miss, the draws; 0: every chunk is tested
 * per sample; same image, counters and launches either way); "wf_defer_nee" (1, default: a path that
 * Russian roulette ends while its NEE shadow ray is pending finishes in that shade step and frees its slot, the term is
 * added by the next shade launch; 0: the slot is held one more iteration; same image and counters either way, fewer
 * launches with 1); "wf_affinity" (0, default: a shard of a batch's work queue is a contiguous range of
 * work ids; 1: the 64 shards are region-major -- shard 8 g + k hands out the tiles of image region k for the samples
 * congruent to g modulo 8 -- and a traversal wave starts on the ray lists of its own XCD's region; read when a batch is
 * published, adaptive batches always take 0; same image and counters either way; measured on the benchmarked frame: a
 * higher L2 hit rate and no gain in time); "frame_ring" = F (keep the
 * rgba8 frame of each of the last F samples for crt_read_sample_rgba8; 0 = off);
 * "temporal_motion" (0 | 1, anything else is CRT_EINVAL: 1 keeps the history of crt_denoise_temporal across
 * crt_update_primitives, see "Temporal reuse"; costs 80 bytes per primitive on the device once an edit has happened);
 * "adaptive_temporal" (0 | 1, anything else is CRT_EINVAL; default 0: 1 lets crt_trace_adaptive take the sample offset
 * and the temporal filters take the adaptive state, each pixel blended with its own tile's count, see "Sample offset"
 * and "Temporal reuse"; with 0 every call launches what it launches without the option);
 * "svgf_spatial_pct" (0 = off, default | 25..10000, anything else is CRT_EINVAL: crt_denoise_svgf gives the pixels whose
 * variance the temporal moments do not cover yet an estimate from their 7x7 neighbourhood, times that percentage, see
 * "Variance-guided temporal filter"; it drops nothing, and with 0 the call launches what it launches without the option);
 * "temporal_clip_pct" (0 = off, default | 25..10000, anything else is CRT_EINVAL: the temporal filters clamp the reprojected
 * history to the mean +- that percentage of a standard deviation of the frame's own 7x7 neighbourhood, and
 * crt_update_lights keeps the history, see "Clipped history"; back to 0 after a kept light edit drops the history);
 * "denoise_latest_wave_blocks" (0 | 1, anything else is CRT_EINVAL; default 0: 1 runs the passes of crt_denoise_latest in
 * one-wave blocks of 8x8 pixels instead of 16x16 -- the same bits, measured slower beside a live pool);
 * "ploc_radius" (1..32, anything else is CRT_EINVAL; default 8: clusters searched to either side by CRT_ACCEL_PLOC; at
 * crt_build_accel);
 * "refit_rebuild_pct" (0 = off, default | 100..100000, anything else is CRT_EINVAL: crt_refit_accel rebuilds once the
 * refitted tree's cost has passed that percentage of its cost as built, see crt_accel_quality);
 * "time_kernels"; "debug_fail_alloc" = k (test hook: the k-th device allocation from now on reports
 * out of memory); "debug_ploc_max_depth" (1..62, default 62) and "debug_ploc_max_rounds" (>= 1, default 256): test
 * hooks, a CRT_ACCEL_PLOC build deeper than the one or unfinished after the other is abandoned and the same call builds
 * the LBVH.  Setting an option first finishes what is in flight. */
int crt_set_option(crt_ctx *ctx, const char *name, int64_t value);

/* Accel statistics: out[0]=BVH2 inner nodes, [1]=leaves, [2]=max depth, [3]=device bytes,
 * [4]=bytes of node data fetched per child box tested by crt_trace (32: plain boxes, 16:
 * 16-bit quantised), [5]=node width crt_trace walks (2, 4 or 8), [6]=inner nodes of that tree,
 * [7]=builder (0: host binned SAH, 1: GPU LBVH, 2: GPU PLOC). */
int crt_accel_stats(crt_ctx *ctx, uint64_t out[8]);

/* Test hooks: one closest-hit query per ray (rays: n x 8 floats ox,oy,oz,dx,dy,dz,exclude_as_u32_bits,_;  out: n x 8:
 * t, px,py,pz, nx,ny,nz, index_bits (0xFFFFFFFF = miss)) through the SINGLE-RAY walk of the BVH2 under
 * CRT_ACCEL_BVH2 / LBVH / PLOC (the walk of the closest-hit rays of the "pipeline" = 0 form, of the denoise G-buffer and the
 * one k_wf_finish FALLS BACK to -- not k_wf_finish's first walk, the single-ray walk of the quantised 4-wide tree:
 * crt_debug_walk_rays; and not the wide tree the wavefront kernels of crt_trace walk: crt_debug_trace_rays), the
 * reference's loop over every primitive under CRT_ACCEL_NONE; and elementwise evaluation of the device math (fn codes: 0 sin 1 cos 2 exp 3 log2 4 exp2
 * 5 pow 6 sqrt 7 div 8 tan). */
int crt_debug_intersect(crt_ctx *ctx, const float *rays, size_t n, float *out);
/* Test hook: n rays through the traversal kernel crt_trace launches for the context's current tree and options (the
 * same instantiation: node width, quantisation, "wf_trace_form", the counting variant under crt_enable_counters; the
 * context's waves per CU and stack overflow area).  The rays are laid out as one iteration's ray lists -- spread over
 * several shards and all four list classes -- so chunking, the shard scan and the refill run as in production.
 *   rays: n x 12 floats  ox,oy,oz, dx,dy,dz, exclude_as_u32_bits, kind_as_u32_bits (0 extension ray, 1 shadow ray),
 *                        t_light, light_index_as_u32_bits, _, _      (the last four: shadow rays only -- the t of the
 *                        light's own primitive along the ray and that primitive's index, as the shade kernel primes them)
 *   out:  n x 2 uint32   extension ray: t bits, primitive index (0xFFFFFFFF = miss);  shadow ray: 1 = light visible / 0, 0
 *   report (may be NULL): [0] node width of the walked tree (4 | 8), [1] its inner levels, [2] stack entries per lane in
 *                        LDS, [3] levels of the overflow area, [4] capacity per lane = [2] + [3], [5] deepest stack a
 *                        lane reached (counting variant, else 0), [6] kernel: 0, 1, 2 = k_wf_trace on the plain 4-wide /
 *                        quantised 4-wide / quantised 8-wide tree, 3 = k_wf_trace2, [7] 1 = counting variant
 * A walk holds at most (width - 1) x levels entries; crt_build_accel sizes the overflow area so that [4] covers it.
 * A sync point.  CRT_EINVAL for a non-finite ray (crt_trace never lets one walk) or a bad kind / light; CRT_ESTATE
 * without a scene or tree, with a stale tree, and where there is no wavefront tree (CRT_ACCEL_NONE, "pipeline" = 0).
 * The counters of crt_counters are not touched. */
int crt_debug_trace_rays(crt_ctx *ctx, const float *rays, size_t n, uint32_t *out, uint64_t report[8]);
/* Test hook: n rays through the SINGLE-RAY walks as the kernels call them, one lane per ray in 64-lane blocks with
 * k_wf_finish's stack (the non-counting instantiations; the counters of crt_counters are not touched).
 *   walk 0: as k_wf_finish walks its stragglers' rays -- the single-ray walk of the quantised 4-wide tree where that tree
 *           is live and no 8-wide tree is (crt_debug_read_accel header [10] = 1, [11] = 0), repeated on the BVH2 when its
 *           stack would overflow; else the BVH2 walk.  Shadow rays any-hit, primed with the given t_light / light index.
 *   walk 1: as the "pipeline" = 0 kernel walks -- the BVH2 only; a shadow ray tests the light's own primitive itself
 *           (t_light of the ray record is not read) and then walks any-hit.
 *   rays: n x 12 floats, the layout of crt_debug_trace_rays
 *   out:  n x 4 uint32   [0] [1] as crt_debug_trace_rays writes them; [2] flags: bit 0 = the 4-wide tree was walked,
 *                        bit 1 = that walk gave up and the BVH2 walk repeated the ray; [3] walk 1, shadow ray: the bits of
 *                        the t_light the kernel computed (0x7F800000 bits of CRT_INFINITY: the ray misses the light), else 0
 *   report (may be NULL): [0] rays that walked the 4-wide tree, [1] rays that fell back, [2] stack entries per lane,
 *                        [3] inner levels of the 4-wide tree, [4] recorded depth of the BVH2, [5] 1 = walk 0 takes the
 *                        4-wide tree, [6] [7] 0
 * Works under "pipeline" 0 and 1 (the trees are the same).  A sync point.  CRT_EINVAL for a non-finite ray, a bad kind /
 * light or walk; CRT_ESTATE without a scene or tree, with a stale tree and under CRT_ACCEL_NONE. */
int crt_debug_walk_rays(crt_ctx *ctx, int walk, const float *rays, size_t n, uint32_t *out, uint64_t report[8]);
int crt_debug_math(crt_ctx *ctx, int fn, const float *a, const float *b, float *out, size_t n);
/* Test hook: the context's current acceleration structure, copied to the caller with plain device-to-host copies (no
 * kernel runs).  `what` selects one part; *bytes (may be NULL) receives the part's size; out == NULL only reports it.
 *   CRT_ACCEL_PART_HEADER        CRT_ACCEL_HEADER_N doubles (every value is an integer or a float, exact in a double):
 *       [0] accel mode (CRT_ACCEL_NONE | CRT_ACCEL_BVH2: both builders make that structure), [1] builder (0 host SAH, 1 GPU
 *       LBVH, 2 GPU PLOC), [2] nprim, [3] root, [4] root4, [5] root8 (child references; -1: none), [6] [7] [8] inner nodes of the BVH2 /
 *       the 4-wide / the 8-wide tree, [9] [10] [11] 1 = the float 4-wide / quantised 4-wide / quantised 8-wide nodes are
 *       live on the device, [12..14] qbase, [15..17] qscale, [18] hit_pad, [19] tree_pad (the pad the boxes were made with),
 *       [20] recorded depth of the BVH2, [21] of the 4-wide tree (the host collapse's, or the level count of the device
 *       collapse), [22] of the 8-wide tree, [23] wf_depth (inner levels of the tree the wavefront kernels walk),
 *       [24] stack entries a walk can need = (width - 1) x [23], [25] stack entries per lane in LDS, [26] overflow levels
 *       the context asks for, [27] overflow levels allocated now (0 before the first trace call), [28] 1 = the tree is
 *       stale (primitives updated, not refitted), [29] 1 = the all-device route (LBVH or PLOC) built the tree (the host holds
 *       statistics only)
 *   CRT_ACCEL_PART_NODES2        [6] x 16 floats (crt_bvh.h: c0.lo c0.hi c1.lo c1.hi ref0 ref1 - -)
 *   CRT_ACCEL_PART_NODES4        [7] x 32 floats where [9], else empty
 *   CRT_ACCEL_PART_NODES4Q       [7] x 16 dwords where [10], else empty
 *   CRT_ACCEL_PART_NODES8Q       [8] x 32 dwords where [11], else empty
 *   CRT_ACCEL_PART_PRIM          nprim x 12 floats, the leaf-ordered records
 *   CRT_ACCEL_PART_PRIMD         nprim x 4 floats
 *   CRT_ACCEL_PART_SLOT_OF_INDEX nprim uint32
 * Under CRT_ACCEL_NONE only the header, PRIM and SLOT_OF_INDEX are not empty.  Works on a stale tree (it shows the boxes
 * as they are).  A sync point; it only reads: accumulator, sample count, counters and the tree stay as they are.
 * CRT_ESTATE without a scene or accel structure, CRT_EINVAL for an unknown part or capacity below the part's size. */
enum {
    CRT_ACCEL_PART_HEADER = 0, CRT_ACCEL_PART_NODES2 = 1, CRT_ACCEL_PART_NODES4 = 2, CRT_ACCEL_PART_NODES4Q = 3,
    CRT_ACCEL_PART_NODES8Q = 4, CRT_ACCEL_PART_PRIM = 5, CRT_ACCEL_PART_PRIMD = 6, CRT_ACCEL_PART_SLOT_OF_INDEX = 7
};
#define CRT_ACCEL_HEADER_N 32
int crt_debug_read_accel(crt_ctx *ctx, int what, void *out, size_t capacity, size_t *bytes);
/* Traversal-efficiency probes of the counting kernel variant (wave-level): inner iterations,
 * lanes active in them, leaf passes, lanes active in them, leaf loop trips, -, refills, lanes refilled. */
int crt_debug_probes(crt_ctx *ctx, uint64_t out[8]);
/* Test hook: (pixel, sample) pairs that k_wf_gen decided itself since the last crt_reset_counters -- camera rays that miss
 * the tree's root boxes, by whole 8x8 tiles of one sample (option "wf_cull_miss").  Counted with and without
 * crt_enable_counters.  A sync point; work in flight at a crt_reset_counters may count on either side of it. */
int crt_debug_gen_culled(crt_ctx *ctx, uint64_t *out);
/* Test hook: paths that k_wf_shade finished at once since the last crt_reset_counters -- paths that Russian roulette ended
 * while their NEE shadow ray was still pending, whose slot is freed in that step and whose term is added one iteration
 * later (option "wf_defer_nee").  0 with the option off.  Counted with and without crt_enable_counters.
 * A sync point; work in flight at a crt_reset_counters may count on either side of it. */
int crt_debug_deferred_nee(crt_ctx *ctx, uint64_t *out);
/* Test hooks: the class of every 8x8 tile of the tile rectangle (row-major, n_tiles = ceil(tw / 8) * ceil(th / 8) bytes;
 * option "wf_cull_classes"): 1 = the camera rays of every pixel of the tile miss the root's four child
 * boxes for every sample, 2 = they all enter one, 0 = it depends on the sample (or nothing could be shown).
 * crt_debug_tile_classes runs the kernel a run's set-up runs, on the context's current camera, tile rectangle and root node
 * (the inputs of the next run, or of the one this call ends) and copies its table; crt_debug_tile_classes_host evaluates
 * the same definition (csrc/crt_tile_class.h) on the CPU over the same inputs, the root node read back from the device.
 * The two agree exactly.  Sync points; they only read.  CRT_ESTATE without a scene or tree, with a stale tree, and where
 * the wavefront kernels walk no quantised 4-wide tree with an inner root; CRT_EINVAL for another n_tiles. */
int crt_debug_tile_classes(crt_ctx *ctx, uint8_t *out, size_t n_tiles);
int crt_debug_tile_classes_host(crt_ctx *ctx, uint8_t *out, size_t n_tiles);
/* Test hook: how many run set-ups of this context have launched the tile classifier so far (the two reads above do not
 * count).  It stays where it is wherever the classes do nothing: "wf_cull_classes" or "wf_cull_miss" 0, adaptive batches,
 * the 8-wide or unquantised tree, four primitives or fewer.  No sync, nothing is finished. */
int crt_debug_tile_class_setups(crt_ctx *ctx, uint64_t *out);
/* Test hook: how many k_wf_gen launches of this context have handed out region-major work so far (option "wf_affinity",
 * the launches that listed a queue published with the option on).  It stays where it is with the option
 * off and for adaptive batches.  No sync, nothing is finished. */
int crt_debug_mapped_gen_launches(crt_ctx *ctx, uint64_t *out);

#ifdef __cplusplus
}
#endif
#endif /* CRT_H */
