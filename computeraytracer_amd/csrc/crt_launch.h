// crt_launch.h -- every host entry into the device code, declared once: the launchers of the eleven .hip files, the GPU tree
// builders and the level lists of the refit.  The .hip file that defines one and every host unit that calls one include
// this header.  (Parameter structs: crt_device.h.)
#pragma once
#include <hip/hip_runtime.h>

#include <vector>

#include "../../include/crt.h"
#include "crt_bvh.h"
#include "crt_device.h"

namespace crt {

// crt_kernels.hip
hipError_t launch_trace(const TraceParams &P, bool count, bool brute, hipStream_t stream);
hipError_t launch_trace_adaptive(const TraceParams &P, const AsTiles &A, bool count, bool brute, hipStream_t stream);
hipError_t launch_debug_intersect(const DevScene &S, const float *rays, size_t n, float *out, int brute, hipStream_t stream);
hipError_t launch_debug_walk_rays(const DevScene &S, int walk, const float *rays, size_t n, uint32_t *out, hipStream_t stream);
hipError_t launch_debug_math(int fn, const float *a, const float *b, float *out, size_t n, hipStream_t stream);
hipError_t launch_assemble(const void *full, void *frame, uint32_t elem_bytes, uint32_t W, uint32_t H, uint32_t world, uint32_t rows_max,
                           uint32_t band, hipStream_t stream);

// crt_wavefront.hip
hipError_t wf_launch_init(const WfParams &P, hipStream_t s);
hipError_t wf_launch_tea(const WfParams &P, uint32_t *out, hipStream_t s);
hipError_t wf_launch_tile_classes(const WfParams &P, uint32_t *out, hipStream_t s);   // out: (tiles + 15) / 16 words
bool wf_gen_culls(const WfParams &P);
bool wf_gen_mapped(const WfParams &P);
hipError_t wf_launch_shade(const WfParams &P, uint32_t it, hipStream_t s);
hipError_t wf_launch_gen(const WfParams &P, uint32_t it, hipStream_t s, const AsTiles *A);
hipError_t wf_launch_trace(const WfParams &P, uint32_t it, uint32_t trace_blocks, hipStream_t s);
int wf_trace_kernel(const WfParams &P);
hipError_t wf_launch_finish(const WfParams &P, WfFinishSegs G, uint32_t max_paths, hipStream_t s);
hipError_t wf_launch_resolve(const WfParams &P, uint32_t last_sample, hipStream_t s);
hipError_t wf_launch_resolve_adaptive(const WfParams &P, const AsTiles &A, uint32_t call_end, hipStream_t s);

// crt_adaptive.hip
hipError_t as_launch_select(const AsParams &A, bool compact, hipStream_t s);
hipError_t as_launch_select_var(const AsVarParams &V, const AsParams *compact, hipStream_t s);
hipError_t as_launch_commit(uint32_t *counts, const uint32_t *active, uint32_t n_active, uint32_t samples, hipStream_t s);

// crt_lbvh.hip
hipError_t build_lbvh(const float *lo, const float *hi, uint32_t n, Bvh &out, hipStream_t stream);
hipError_t build_lbvh_device(const unsigned char *d_raw, uint32_t n, float hit_pad, float4 *d_prim, float4 *d_primD,
                             uint32_t *d_slot_of_index, float *d_nodes2, uint4 *d_nodes4q, LbvhDeviceResult &res, hipStream_t stream);
// (its stages, which the clustered build of crt_ploc.hip shares: sorted Morton keys, the record gather, the collapse)
template <typename T> struct DevBuf;        // crt_ctx.h: the sort's temporary is the caller's, freed with its scope
hipError_t lbvh_sorted_keys_host(const float *lo, const float *hi, uint32_t n, float *d_lo, float *d_hi, unsigned long long *d_keys,
                                 unsigned long long *d_sorted, DevBuf<char> &sort_tmp, hipStream_t stream);
hipError_t lbvh_sorted_keys_device(const unsigned char *d_raw, uint32_t n, float hit_pad, float *d_lo, float *d_hi, uint32_t *d_cbox,
                                   unsigned long long *d_keys, unsigned long long *d_sorted, DevBuf<char> &sort_tmp, hipStream_t stream);
hipError_t lbvh_launch_gather(const unsigned char *d_raw, const unsigned long long *d_keys, uint32_t n, float4 *d_prim, float4 *d_primD,
                              uint32_t *d_slot_of_index, hipStream_t stream);
hipError_t lbvh_collapse_device(const float *d_nodes2, uint32_t n, uint4 *d_nodes4q, LbvhDeviceResult &res, hipStream_t stream);

// crt_ploc.hip
hipError_t build_ploc(const float *lo, const float *hi, uint32_t n, const PlocOptions &opt, Bvh &out, PlocInfo &info, hipStream_t stream);
hipError_t build_ploc_device(const unsigned char *d_raw, uint32_t n, float hit_pad, const PlocOptions &opt, float4 *d_prim, float4 *d_primD,
                             uint32_t *d_slot_of_index, float *d_nodes2, uint4 *d_nodes4q, LbvhDeviceResult &res, PlocInfo &info,
                             hipStream_t stream);

// crt_refit.hip
hipError_t refit_launch_pad(const unsigned char *raw, uint32_t n, uint32_t *out, hipStream_t s);
hipError_t refit_launch_prims(const unsigned char *raw, uint32_t first, uint32_t count, const uint32_t *slot_of_index, float4 *prim,
                              float4 *primD, hipStream_t s);
hipError_t refit_launch_transform(unsigned char *raw, const uint32_t *start, const crt_prim_transform *ops, uint32_t n_ops, uint32_t total,
                                  const uint32_t *slot_of_index, float4 *prim, float4 *primD, hipStream_t s);
hipError_t refit_launch_compact(const unsigned char *src, unsigned char *dst, const uint32_t *tab, uint32_t n_gaps, uint32_t n_new, hipStream_t s);
hipError_t refit_levels(const void *nodes, uint32_t width, bool quantised, int root, uint32_t cap, int *list, uint32_t *counter,
                        uint32_t *nch, std::vector<uint32_t> &off, hipStream_t s);
hipError_t refit_launch_bvh2(const float4 *prim, float pad, const int *list, const std::vector<uint32_t> &off, float *nodes, hipStream_t s);
hipError_t refit_launch_wide(const float4 *prim, float pad, const int *list, const std::vector<uint32_t> &off, const void *refs,
                             bool quantised, const uint32_t *nch, float *fb, hipStream_t s);
hipError_t refit_launch_quant4(const float *fb, const uint32_t *nch, uint32_t n4, uint4 *nodes4q, const double base[3], const double scale[3],
                               hipStream_t s);

// crt_quality.hip
hipError_t quality_launch(int layout, const void *nodes, uint32_t n, uint32_t root, const float base[3], const float scale[3],
                          double2 *partial, double *out, hipStream_t s);

// crt_denoise.hip
hipError_t dn_launch_gbuffer(const DevScene &S, uint32_t x0, uint32_t y0, uint32_t tw, uint32_t th, float4 *gbuf, uint32_t *key,
                             int brute, hipStream_t stream);
// (each leaves the buffer that holds the result in *out)
hipError_t dn_launch_filter(const DnFilter &F, const float4 *accum, float n, float sigma_color, float4 **out);
// (its two halves, for a caller that splits them across streams -- crt_denoise_latest, DESIGN.md 6m: the snapshot
// accum / n -> F.c[0] on `stream`, then the passes on F.stream; wave_blocks: in one-wave blocks of 8x8 pixels)
hipError_t dn_launch_prepare(const DnFilter &F, const float4 *accum, float n, hipStream_t stream);
hipError_t dn_launch_passes(const DnFilter &F, float sigma_color, bool wave_blocks, float4 **out);
hipError_t dn_launch_filter_adaptive(const DnFilter &F, const float4 *accum, const float *q, const uint32_t *counts, uint2 *kv,
                                     float *var, float sigma_variance, float4 **out);
// (counts: null in the uniform state, where P.n is every pixel's n; else the adaptive state's count per 8x8 tile)
// (box: null, or 2 float4 per pixel for the clip boxes of option "temporal_clip_pct" with its factor gamma, DESIGN.md 6l: the box
// pass runs before the blend where P.h_prev is there, and the blend clamps the reprojected history to it)
hipError_t dn_launch_temporal(const DnFilter &F, DnReprojParams P, const uint32_t *counts, float sigma_color, float4 *box, float gamma,
                              float4 **out);
// (spatial_b: 0, or the factor of option "svgf_spatial_pct")
hipError_t dn_launch_svgf(const DnFilter &F, DnSvgfParams P, const uint32_t *counts, uint2 *kv, float *var, float sigma_variance,
                          float spatial_b, float4 *box, float gamma, float4 **out);
hipError_t dn_launch_motion(const DnReprojParams &P, float2 *out, hipStream_t stream);

// crt_aov.hip
hipError_t aov_launch(const DevScene &S, const AovParams &P, hipStream_t stream);

// crt_matte.hip
hipError_t matte_launch(const DevScene &S, const MatteParams &P, hipStream_t stream);

// crt_query.hip (mode: CRT_QUERY_CLOSEST / CRT_QUERY_ANY; pick: P.xy in place of P.rays; brute: CRT_ACCEL_NONE)
hipError_t query_launch(const DevScene &S, const QueryParams &P, int mode, bool pick, bool brute, hipStream_t stream);

// crt_radiance.hip (brute: CRT_ACCEL_NONE).  radiance_blocks: the grid of a launch of n rays on a device of num_cu compute
// units, min(ceil(n / 64), num_cu * kRadianceWavesPerCu) blocks of 64 lanes; lane g of all of them owns rays g, g + G, ...
uint32_t radiance_blocks(size_t n, uint32_t num_cu);
hipError_t radiance_launch(const DevScene &S, const RadianceParams &P, bool brute, uint32_t num_cu, hipStream_t stream);

}  // namespace crt
