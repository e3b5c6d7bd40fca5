// Adam (torch.optim.Adam defaults, single-tensor operation order): the per-element update and the scalars it runs under.
// Shared by the arena passes (optim_impl.h's range_pass, behind adam.hip, optim.hip and groups.hip) and the GEMM epilogue that applies the update to
// linear5.weight straight from the weight gradient's accumulators (gemm_f32.hip: gemm_f32_epi_kernel), so that every site
// compiles the same expressions and produces the same bits.
#pragma once
#include <math.h>
#include <stdint.h>

#include "common.h"

namespace goalnet {

__device__ __forceinline__ void adam1(float& p, float g, float& m, float& v, float b2, float omb1, float omb2,
                                      float eps, float step_size, float bc2_sqrt, float gs) {
    g *= gs;
    m = m + omb1 * (g - m);                    // exp_avg.lerp_(grad, 1 - beta1)
    v = v * b2 + (omb2 * g) * g;               // exp_avg_sq.mul_(beta2).addcmul_(grad, grad, value = 1 - beta2)
    const float denom = sqrtf(v) / bc2_sqrt + eps;
    p = p - step_size * (m / denom);           // param.addcdiv_(exp_avg, denom, value = -step_size)
}

// AMSGrad: torch's _single_tensor_adam(amsgrad=True). m and v as in adam1; the denominator comes from the running maximum of v.
__device__ __forceinline__ void adam1_amsgrad(float& p, float g, float& m, float& v, float& vmax, float b2, float omb1, float omb2,
                                              float eps, float step_size, float bc2_sqrt, float gs) {
    g *= gs;
    m = m + omb1 * (g - m);
    v = v * b2 + (omb2 * g) * g;
    vmax = (vmax >= v || vmax != vmax) ? vmax : v;   // torch.maximum(max_exp_avg_sq, exp_avg_sq): a NaN on either side stays (not fmaxf)
    const float denom = sqrtf(vmax) / bc2_sqrt + eps;
    p = p - step_size * (m / denom);
}

// The scalars torch's _single_tensor_adam computes as python floats (doubles), computed in fp64 for the 1-based step count ti.
struct AdamScalars { float step_size, bc2_sqrt, b2, omb1, omb2; };

__device__ __forceinline__ AdamScalars adam_scalars(double lr, double beta1, double beta2, int64_t ti) {
    const double t = (double)ti;
    AdamScalars s;
    s.step_size = (float)(lr / (1.0 - pow(beta1, t)));
    s.bc2_sqrt = (float)sqrt(1.0 - pow(beta2, t));
    s.b2 = (float)beta2; s.omb1 = (float)(1.0 - beta1); s.omb2 = (float)(1.0 - beta2);
    return s;
}

}  // namespace goalnet
