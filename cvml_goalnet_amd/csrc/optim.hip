// Optimizer options on the fused step (include/goalnet_optim.h): weight decay (coupled as torch.optim.Adam's,
// decoupled as torch.optim.AdamW's), clipping by the global gradient norm (torch.nn.utils.clip_grad_norm_) and a learning-rate
// schedule evaluated on the device from the step counter, so that a captured graph follows it. The per-element update and its
// scalars are adam.h's (adam1, adam_scalars), included: a range that no option touches runs adam_ranges_kernel's own loop
// (small.hip) and gives its bits. Block-to-range mapping, tail, 16-bit copy and guard are that kernel's too.
#include "optim_impl.h"

using namespace goalnet;

namespace {

__global__ void optim_lr_kernel(goalnet_optim_opts o, const int64_t* __restrict__ step, double* __restrict__ lr_out) {
    if (blockIdx.x == 0 && threadIdx.x == 0) *lr_out = sched_lr(o, *step);
}

struct OptimRanges {
    int64_t begin[GOALNET_ADAM_RANGES_MAX], count[GOALNET_ADAM_RANGES_MAX], skipped[GOALNET_ADAM_RANGES_MAX];
    int first_block[GOALNET_ADAM_RANGES_MAX + 1];
    uint32_t decay;                                      // bit r: weight decay applies to range r
};

__global__ __launch_bounds__(256) void optim_ranges_kernel(float* __restrict__ p, const float* __restrict__ g, float* __restrict__ m,
                                                          float* __restrict__ v, OptimRanges rs, int nranges, goalnet_optim_opts o,
                                                          const int64_t* __restrict__ step_dev, float gs,
                                                          const double* __restrict__ sumsq, uint2* __restrict__ shadow, int64_t sh_b4,
                                                          int64_t sh_e4, int sh_f16, const int64_t* __restrict__ bad_step) {
    const int64_t e = *step_dev, t1 = e + 1;              // t1: the step's own count, what goalnet_grad_finite_check stamps
    if (bad_step && *bad_step == t1) return;
    int r = 0;
    while (r + 1 < nranges && (int)blockIdx.x >= rs.first_block[r + 1]) ++r;
    const int64_t lb = (int)blockIdx.x - rs.first_block[r], nb = rs.first_block[r + 1] - rs.first_block[r];
    const double lr_t = sched_lr(o, e);                   // the global count: every range runs at the same rate
    const AdamScalars sc = adam_scalars(lr_t, o.beta1, o.beta2, t1 - rs.skipped[r]);
    ElemScalars s;
    s.b2 = sc.b2; s.omb1 = sc.omb1; s.omb2 = sc.omb2; s.eps = (float)o.eps; s.step_size = sc.step_size; s.bc2_sqrt = sc.bc2_sqrt;
    s.gs = gs;
    s.coef = 1.0f;
    if (sumsq) {
        const double c = o.max_norm / ((double)gs * sqrt(*sumsq) + 1e-6);
        s.coef = (float)(c < 1.0 ? c : 1.0);
    }
    s.wd = (float)o.weight_decay;
    s.shrink = (float)(1.0 - lr_t * o.weight_decay);
    const bool decay = ((rs.decay >> r) & 1u) != 0 && o.weight_decay > 0.0;
    const int64_t begin = rs.begin[r], n = rs.count[r];
    range_dispatch<false>(decay, o.decoupled != 0, sumsq != nullptr, p, g, m, v, nullptr, begin, n, lb, nb, s, shadow, sh_b4, sh_e4, sh_f16);
}

// ---- sum of squares over the ranges: fixed shares, fixed order ------------------------------------------------------------------------
constexpr int SUMSQ_BLOCKS_MAX = 1024;                   // per range: 1024 x 256 threads x 16 B in flight saturate the HBM

struct SumsqRanges {
    int64_t begin[GOALNET_ADAM_RANGES_MAX], count[GOALNET_ADAM_RANGES_MAX];
    int first_block[GOALNET_ADAM_RANGES_MAX + 1];
};

// the block's total in thread 0: lanes by butterfly, then the four waves in order
__device__ __forceinline__ double block_sum_d(double a) {
    __shared__ double s_w[4];
    a = wave_sum_d(a);
    if ((threadIdx.x & 63) == 0) s_w[threadIdx.x >> 6] = a;
    __syncthreads();
    return ((s_w[0] + s_w[1]) + s_w[2]) + s_w[3];
}

__global__ __launch_bounds__(256) void sumsq_partials_kernel(const float* __restrict__ g, SumsqRanges rs, int nranges,
                                                            double* __restrict__ partials) {
    int r = 0;
    while (r + 1 < nranges && (int)blockIdx.x >= rs.first_block[r + 1]) ++r;
    const int64_t lb = (int)blockIdx.x - rs.first_block[r], nb = rs.first_block[r + 1] - rs.first_block[r];
    const int64_t begin = rs.begin[r], n = rs.count[r], b4 = begin >> 2, n4 = n >> 2;
    double a0 = 0.0, a1 = 0.0, a2 = 0.0, a3 = 0.0;
    for (int64_t j = lb * blockDim.x + threadIdx.x; j < n4; j += nb * blockDim.x) {
        const float4 gg = reinterpret_cast<const float4*>(g)[b4 + j];
        a0 = fma((double)gg.x, (double)gg.x, a0);        // the product is exact in fp64: one rounding per term
        a1 = fma((double)gg.y, (double)gg.y, a1);
        a2 = fma((double)gg.z, (double)gg.z, a2);
        a3 = fma((double)gg.w, (double)gg.w, a3);
    }
    if (lb == 0 && threadIdx.x < (n & 3)) {
        const double x = (double)g[begin + (n4 << 2) + threadIdx.x];
        a0 = fma(x, x, a0);
    }
    const double tot = block_sum_d((a0 + a1) + (a2 + a3));
    if (threadIdx.x == 0) partials[blockIdx.x] = tot;
}

__global__ __launch_bounds__(256) void sumsq_finish_kernel(const double* __restrict__ partials, int nparts, double* __restrict__ sumsq) {
    double a = 0.0;
    for (int i = threadIdx.x; i < nparts; i += 256) a += partials[i];
    const double tot = block_sum_d(a);
    if (threadIdx.x == 0) *sumsq = tot;
}

}  // namespace

extern "C" {

size_t goalnet_grad_sumsq_ws_bytes(const goalnet_optim_range* ranges, int count) {
    SumsqRanges rs;
    if (check_ranges("grad_sumsq_ws_bytes", ranges, count, SUMSQ_BLOCKS_MAX, rs.begin, rs.count, nullptr, nullptr, rs.first_block) != 0) return 0;
    return sizeof(double) * (size_t)rs.first_block[count];
}

int goalnet_grad_sumsq(const float* g, const goalnet_optim_range* ranges, int count, double* sumsq, void* ws, size_t ws_bytes,
                       void* stream) {
    GN_REQUIRE(g && sumsq && ws, GOALNET_E_NULL, "grad_sumsq: null pointer");
    SumsqRanges rs;
    const int rc = check_ranges("grad_sumsq", ranges, count, SUMSQ_BLOCKS_MAX, rs.begin, rs.count, nullptr, nullptr, rs.first_block);
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
    GN_REQUIRE(p && g && m && v && step, GOALNET_E_NULL, "optim_step_dev_ranges: null pointer");
    OptimRanges rs;
    int rc = check_ranges("optim_step_dev_ranges", ranges, count, OPTIM_BLOCKS_MAX, rs.begin, rs.count, rs.skipped, &rs.decay, rs.first_block);
    if (rc != 0) return rc;
    rc = check_opts("optim_step_dev_ranges", opts);
    if (rc != 0) return rc;
    rc = check_step_args("optim_step_dev_ranges", p, g, m, v, opts, sumsq, shadow_16, shadow_begin, shadow_count);
    if (rc != 0) return rc;
    hipLaunchKernelGGL(optim_ranges_kernel, dim3((unsigned)rs.first_block[count]), dim3(256), 0, (hipStream_t)stream, p, g, m, v, rs, count, *opts,
                       step, grad_scale, sumsq, (uint2*)shadow_16, shadow_begin >> 2, shadow_16 ? (shadow_begin + shadow_count) >> 2 : 0, f16,
                       bad_step);
    GN_LAUNCH_CHECK("optim_step_dev_ranges");
    return 0;
}

int goalnet_optim_lr(const goalnet_optim_opts* opts, const int64_t* step, double* lr_out, void* stream) {
    GN_REQUIRE(step && lr_out, GOALNET_E_NULL, "optim_lr: null pointer");
    const int rc = check_opts("optim_lr", opts);
    if (rc != 0) return rc;
    hipLaunchKernelGGL(optim_lr_kernel, dim3(1), dim3(64), 0, (hipStream_t)stream, *opts, step, lr_out);
    GN_LAUNCH_CHECK("optim_lr");
    return 0;
}

}  // extern "C"
