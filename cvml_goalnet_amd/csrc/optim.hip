// Optimizer options on the fused step (include/goalnet_optim.h): weight decay (coupled as torch.optim.Adam's,
// decoupled as torch.optim.AdamW's), clipping by the global gradient norm (torch.nn.utils.clip_grad_norm_) and a learning-rate
// schedule evaluated on the device from the step counter, so that a captured graph follows it. The per-element update and its
// scalars are adam.h's (adam1, adam_scalars), included: a range that no option touches runs adam_ranges_kernel's own loop
// (adam.hip; both are optim_impl.h's range_pass) and gives its bits. Block-to-range mapping and tail are ranges.h's.
#include "optim_impl.h"

using namespace goalnet;

namespace {

__global__ void sched_lr_kernel(goalnet_optim_opts o, const int64_t* __restrict__ step, double* __restrict__ lr_out) {
    if (blockIdx.x == 0 && threadIdx.x == 0) *lr_out = sched_lr(o, o.lr, *step);
}

struct OptimSteps {
    int64_t skipped[GOALNET_ADAM_RANGES_MAX];
    uint64_t decay;                                      // bit r: weight decay applies to range r
};

__global__ __launch_bounds__(256) void optim_ranges_kernel(float* __restrict__ p, const float* __restrict__ g, float* __restrict__ m,
                                                          float* __restrict__ v, RangeMap rs, OptimSteps st, int nranges, goalnet_optim_opts o,
                                                          const int64_t* __restrict__ step_dev, float gs,
                                                          const double* __restrict__ sumsq, uint2* __restrict__ shadow, int64_t sh_b4,
                                                          int64_t sh_e4, int sh_f16, const int64_t* __restrict__ bad_step) {
    const int64_t e = *step_dev;                          // e + 1: the step's own count, what goalnet_grad_finite_check stamps
    if (bad_step && *bad_step == e + 1) return;
    const BlockShare b = block_share(rs, nranges);
    optim_block(p, g, m, v, nullptr, b, st.skipped[b.r], ((st.decay >> b.r) & 1u) != 0, o, o.lr, o.beta1, o.beta2, o.eps, o.weight_decay, false, e,
                gs, sumsq, {shadow, sh_b4, sh_e4, sh_f16});
}

// ---- sum of squares over the ranges: fixed shares, fixed order ------------------------------------------------------------------------
constexpr int SUMSQ_BLOCKS_MAX = 1024;                   // per range: 1024 x 256 threads x 16 B in flight saturate the HBM

// the block's total in thread 0: lanes by butterfly, then the four waves in order
__device__ __forceinline__ double block_sum_d(double a) {
    __shared__ double s_w[4];
    a = wave_sum_d(a);
    if ((threadIdx.x & 63) == 0) s_w[threadIdx.x >> 6] = a;
    __syncthreads();
    return ((s_w[0] + s_w[1]) + s_w[2]) + s_w[3];
}

__global__ __launch_bounds__(256) void sumsq_partials_kernel(const float* __restrict__ g, RangeMap rs, int nranges,
                                                            double* __restrict__ partials) {
    double a0 = 0.0, a1 = 0.0, a2 = 0.0, a3 = 0.0;
    for_share(
        block_share(rs, nranges),
        [&](int64_t i) {
            const float4 gg = reinterpret_cast<const float4*>(g)[i];
            a0 = fma((double)gg.x, (double)gg.x, a0);    // the product is exact in fp64: one rounding per term
            a1 = fma((double)gg.y, (double)gg.y, a1);
            a2 = fma((double)gg.z, (double)gg.z, a2);
            a3 = fma((double)gg.w, (double)gg.w, a3);
        },
        [&](int64_t i) {
            const double x = (double)g[i];
            a0 = fma(x, x, a0);
        });
    const double tot = block_sum_d((a0 + a1) + (a2 + a3));
    if (threadIdx.x == 0) partials[blockIdx.x] = tot;
}

__global__ __launch_bounds__(256) void sumsq_finish_kernel(const double* __restrict__ partials, int nparts, double* __restrict__ sumsq) {
    double a = 0.0;
    for (int i = threadIdx.x; i < nparts; i += 256) a += partials[i];
    const double tot = block_sum_d(a);
    if (threadIdx.x == 0) *sumsq = tot;
}

// the ranges of the sum of squares: goalnet_optim_range's rules, `skipped` among them
int sumsq_ranges(const char* who, const goalnet_optim_range* ranges, int count, RangeMap* rs) {
    const int rc = map_ranges(who, ranges, count, SUMSQ_BLOCKS_MAX, rs);
    return rc != 0 ? rc : copy_skipped(who, ranges, count, nullptr);
}

}  // namespace

int goalnet::launch_sched_lr(const char* who, const goalnet_optim_opts& o, const int64_t* step, double* lr_out, void* stream) {
    hipLaunchKernelGGL(sched_lr_kernel, dim3(1), dim3(64), 0, (hipStream_t)stream, o, step, lr_out);
    GN_LAUNCH_CHECK(who);
    return 0;
}

extern "C" {

size_t goalnet_grad_sumsq_ws_bytes(const goalnet_optim_range* ranges, int count) {
    RangeMap rs;
    if (sumsq_ranges("grad_sumsq_ws_bytes", ranges, count, &rs) != 0) return 0;
    return sizeof(double) * (size_t)rs.first_block[count];
}

int goalnet_grad_sumsq(const float* g, const goalnet_optim_range* ranges, int count, double* sumsq, void* ws, size_t ws_bytes,
                       void* stream) {
    GN_REQUIRE(g && sumsq && ws, GOALNET_E_NULL, "grad_sumsq: null pointer");
    RangeMap rs;
    const int rc = sumsq_ranges("grad_sumsq", ranges, count, &rs);
    if (rc != 0) return rc;
    GN_REQUIRE(aligned16(g), GOALNET_E_ALIGN, "grad_sumsq: the arena must be 16-byte aligned");
    GN_REQUIRE((reinterpret_cast<uintptr_t>(ws) & 7u) == 0 && (reinterpret_cast<uintptr_t>(sumsq) & 7u) == 0, GOALNET_E_ALIGN,
               "grad_sumsq: workspace and result must be 8-byte aligned");
    const int nblocks = rs.first_block[count];
    GN_REQUIRE(ws_bytes >= sizeof(double) * (size_t)nblocks, GOALNET_E_WORKSPACE, "grad_sumsq: workspace too small: %zu < %zu", ws_bytes,
               sizeof(double) * (size_t)nblocks);
    hipLaunchKernelGGL(sumsq_partials_kernel, dim3((unsigned)nblocks), dim3(256), 0, (hipStream_t)stream, g, rs, count, (double*)ws);
    GN_LAUNCH_CHECK("grad_sumsq");
    hipLaunchKernelGGL(sumsq_finish_kernel, dim3(1), dim3(256), 0, (hipStream_t)stream, (const double*)ws, nblocks, sumsq);
    GN_LAUNCH_CHECK("grad_sumsq");
    return 0;
}

int goalnet_optim_step_dev_ranges(float* p, const float* g, float* m, float* v, const goalnet_optim_range* ranges, int count,
                                  const goalnet_optim_opts* opts, const int64_t* step, float grad_scale, const double* sumsq,
                                  void* shadow_16, int64_t shadow_begin, int64_t shadow_count, int f16, const int64_t* bad_step,
                                  void* stream) {
    const char* who = "optim_step_dev_ranges";
    GN_REQUIRE(p && g && m && v && step, GOALNET_E_NULL, "%s: null pointer", who);
    RangeMap rs;
    OptimSteps st;
    int rc = map_ranges(who, ranges, count, RANGE_BLOCKS_MAX, &rs);
    if (rc == 0) rc = copy_skipped(who, ranges, count, st.skipped);
    if (rc == 0) rc = check_opts(who, opts);
    if (rc == 0) rc = check_step_args(who, p, g, m, v, opts, sumsq, shadow_16, shadow_begin, shadow_count);
    if (rc != 0) return rc;
    st.decay = 0;
    for (int r = 0; r < count; ++r) st.decay |= (uint64_t)(ranges[r].decay != 0) << r;
    hipLaunchKernelGGL(optim_ranges_kernel, dim3((unsigned)rs.first_block[count]), dim3(256), 0, (hipStream_t)stream, p, g, m, v, rs, st, count,
                       *opts, step, grad_scale, sumsq, (uint2*)shadow_16, shadow_begin >> 2, shadow_16 ? (shadow_begin + shadow_count) >> 2 : 0,
                       f16, bad_step);
    GN_LAUNCH_CHECK(who);
    return 0;
}

int goalnet_optim_lr(const goalnet_optim_opts* opts, const int64_t* step, double* lr_out, void* stream) {
    GN_REQUIRE(step && lr_out, GOALNET_E_NULL, "optim_lr: null pointer");
    const int rc = check_opts("optim_lr", opts);
    if (rc != 0) return rc;
    return launch_sched_lr("optim_lr", *opts, step, lr_out, stream);
}

}  // extern "C"
