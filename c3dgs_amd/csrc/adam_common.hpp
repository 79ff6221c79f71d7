// adam_common.hpp -- the per-element arithmetic of the Adam kernels (adam.hip: every element; sparse_adam.hip: the elements of
// the listed rows), torch's _single_tensor_adam in its order. Both files are built with -ffp-contract=off, so the two kernels
// round alike and agree bit for bit on the same element.
#pragma once
#include <hip/hip_runtime.h>

namespace c3dgs {

__device__ __forceinline__ void adam_one(float& p, float g, float& m, float& v, float w1, float beta2, float w2, float eps,
                                         float neg_step, float bc2_sqrt)
{
    m = w1 < 0.5f ? m + w1 * (g - m) : g - (g - m) * (1.f - w1);          // at::lerp
    v = v * beta2;
    v = v + w2 * g * g;                                                    // addcmul: a + alpha * b * c
    const float denom = sqrtf(v) / bc2_sqrt + eps;
    p = p + neg_step * (m / denom);                                        // addcdiv: a + alpha * (b / c)
}

} // namespace c3dgs
