// An exponential moving average of the weights behind the fused step, and the exchange of two arenas (include/goalnet_ema.h,
// DESIGN.md §4.15). One pass over the trainable ranges, 12 bytes per parameter: read p, read and write e. Whether the pass copies,
// averages or leaves e alone, and the weight it averages with, come from the device step counter — evaluated by every thread where
// adam_scalars / sched_lr evaluate theirs — so a captured graph follows the count. Block-to-range mapping, tail and the
// host's range checks are ranges.h's.
#include <math.h>

#include "../../include/goalnet_ema.h"
#include "ranges.h"

using namespace goalnet;

namespace {

enum { EMA_SKIP = 0, EMA_COPY = 1, EMA_AVERAGE = 2 };

// what step t does to the average, and with which weight: fp64, uniform over the grid (optim.EmaOptions.weight_at is this expression)
__device__ __forceinline__ int ema_plan(const goalnet_ema_opts& o, int64_t t, float* w) {
    if (t <= o.start_step) return EMA_COPY;
    const int64_t u = t - o.start_step;
    if (u % o.every != 0) return EMA_SKIP;
    const int64_t k = u / o.every - 1;                    // averaging updates before this one
    double d = o.decay;
    if (o.warmup) {
        const double dw = (double)(1 + k) / (double)(10 + k);
        d = dw < d ? dw : d;
    }
    *w = (float)(1.0 - d);
    return EMA_AVERAGE;
}

__device__ __forceinline__ float ema1(float e, float p, float w) { return fmaf(w, p - e, e); }

__global__ __launch_bounds__(256) void ema_ranges_kernel(const float* __restrict__ p, float* __restrict__ e, RangeMap rs, int nranges,
                                                        goalnet_ema_opts o, const int64_t* __restrict__ step_dev, int64_t step_bias,
                                                        const int64_t* __restrict__ bad_step) {
    const int64_t t = *step_dev + step_bias;              // the step that has just been applied: what goalnet_grad_finite_check stamps
    if (bad_step && *bad_step == t) return;
    float w = 1.0f;
    const int plan = ema_plan(o, t, &w);
    if (plan == EMA_SKIP) return;
    const BlockShare b = block_share(rs, nranges);
    if (plan == EMA_COPY) {
        for_share(
            b, [&](int64_t i) { reinterpret_cast<uint4*>(e)[i] = reinterpret_cast<const uint4*>(p)[i]; },
            [&](int64_t i) { reinterpret_cast<uint32_t*>(e)[i] = reinterpret_cast<const uint32_t*>(p)[i]; });
        return;
    }
    for_share(
        b,
        [&](int64_t i) {
            const float4 pp = reinterpret_cast<const float4*>(p)[i];
            float4 ee = reinterpret_cast<float4*>(e)[i];
            ee.x = ema1(ee.x, pp.x, w);
            ee.y = ema1(ee.y, pp.y, w);
            ee.z = ema1(ee.z, pp.z, w);
            ee.w = ema1(ee.w, pp.w, w);
            reinterpret_cast<float4*>(e)[i] = ee;
        },
        [&](int64_t i) { e[i] = ema1(e[i], p[i], w); });
}

__global__ __launch_bounds__(256) void swap_ranges_kernel(uint32_t* __restrict__ a, uint32_t* __restrict__ b, RangeMap rs, int nranges) {
    for_share(
        block_share(rs, nranges),
        [&](int64_t i) {
            const uint4 x = reinterpret_cast<uint4*>(a)[i], y = reinterpret_cast<uint4*>(b)[i];
            reinterpret_cast<uint4*>(a)[i] = y;
            reinterpret_cast<uint4*>(b)[i] = x;
        },
        [&](int64_t i) {
            const uint32_t x = a[i], y = b[i];
            a[i] = y;
            b[i] = x;
        });
}

}  // namespace

extern "C" {

int goalnet_ema_update_dev_ranges(const float* p, float* e, const goalnet_adam_range* ranges, int count, const goalnet_ema_opts* opts,
                                  const int64_t* step, int64_t step_bias, const int64_t* bad_step, void* stream) {
    GN_REQUIRE(p && e && step, GOALNET_E_NULL, "ema_update_dev_ranges: null pointer");
    RangeMap rs;
    const int rc = map_ranges("ema_update_dev_ranges", ranges, count, RANGE_BLOCKS_MAX, &rs);
    if (rc != 0) return rc;
    GN_REQUIRE(opts, GOALNET_E_NULL, "ema_update_dev_ranges: null options");
    GN_REQUIRE(isfinite(opts->decay) && opts->decay >= 0.0 && opts->decay < 1.0, GOALNET_E_VALUE, "ema_update_dev_ranges: decay must be in [0, 1)");
    GN_REQUIRE(opts->every >= 1, GOALNET_E_VALUE, "ema_update_dev_ranges: every must be >= 1");
    GN_REQUIRE(opts->start_step >= 0, GOALNET_E_VALUE, "ema_update_dev_ranges: start_step must be >= 0");
    GN_REQUIRE(p != e, GOALNET_E_VALUE, "ema_update_dev_ranges: the average and the weights are the same arena");
    GN_REQUIRE(aligned16(p) && aligned16(e), GOALNET_E_ALIGN, "ema_update_dev_ranges: arenas must be 16-byte aligned");
    GN_REQUIRE((reinterpret_cast<uintptr_t>(step) & 7u) == 0 && (reinterpret_cast<uintptr_t>(bad_step) & 7u) == 0, GOALNET_E_ALIGN,
               "ema_update_dev_ranges: counters must be 8-byte aligned");
    hipLaunchKernelGGL(ema_ranges_kernel, dim3((unsigned)rs.first_block[count]), dim3(256), 0, (hipStream_t)stream, p, e, rs, count, *opts, step,
                       step_bias, bad_step);
    GN_LAUNCH_CHECK("ema_update_dev_ranges");
    return 0;
}

int goalnet_swap_ranges(float* a, float* b, const goalnet_adam_range* ranges, int count, void* stream) {
    GN_REQUIRE(a && b, GOALNET_E_NULL, "swap_ranges: null pointer");
    RangeMap rs;
    const int rc = map_ranges("swap_ranges", ranges, count, RANGE_BLOCKS_MAX, &rs);
    if (rc != 0) return rc;
    GN_REQUIRE(a != b, GOALNET_E_VALUE, "swap_ranges: the two arenas are the same");
    GN_REQUIRE(aligned16(a) && aligned16(b), GOALNET_E_ALIGN, "swap_ranges: arenas must be 16-byte aligned");
    hipLaunchKernelGGL(swap_ranges_kernel, dim3((unsigned)rs.first_block[count]), dim3(256), 0, (hipStream_t)stream,
                       reinterpret_cast<uint32_t*>(a), reinterpret_cast<uint32_t*>(b), rs, count);
    GN_LAUNCH_CHECK("swap_ranges");
    return 0;
}

}  // extern "C"
