// crt_adaptive.h -- the per-pixel noise estimate of adaptive sampling, shared by the tile selection
// (crt_adaptive.hip) and the variance-guided filter (crt_denoise.hip): one definition, one f32 contract.
#pragma once
#include <hip/hip_runtime.h>

#include "crt_math.h"

namespace crt {

// e of one pixel holding n_t >= 2 samples, S = accum.y, Q = sum of Y^2: every + - * / and sqrt one IEEE operation
// (-ffp-contract=off), exp_ / max_ those of crt_math.h.  Standard error of the mean times the slope of the reference's
// exposure curve T(y) = 1 - exp(-2.2 y) at the mean.
__device__ __forceinline__ float pixel_error(float S, float Q, uint32_t n_t)
{
    const float n = (float)n_t;
    const float m = S / n;
    float v = Q / n - m * m;
    v = max_(v, 0.0f);
    const float se = sqrt_(v / (float)(n_t - 1u));
    return (2.2f * exp_(-2.2f * max_(m, 0.0f))) * se;
}

}  // namespace crt
