// The fused Adam step (torch.optim.Adam defaults, single-tensor operation order): one pass over the flat parameter arena at
// 28 B/parameter (HBM-bound; it was 57 % of the reference's step at its own sub-batch size), over the whole arena or over a list of
// its ranges, and the overflow check of precision = "fp16" that guards it. The per-element update (adam1) and the step's scalars
// (adam_scalars) live in adam.h: the weight-gradient GEMM's epilogue runs the same code. The loop with the 16-bit copy is
// optim_impl.h's range_pass in its plain mode, the one the optimizer launches (optim.hip, groups.hip) run for a range that no option
// touches; the walk of a block over its share of a range is ranges.h's.
#include "optim_impl.h"

using namespace goalnet;

namespace {

// One kernel for both whole-arena entry points (host step count / device step counter) so that they produce the same bits: the
// one-range case of adam_ranges_kernel, every block of the grid on the range [0, n).
__global__ __launch_bounds__(256) void adam_kernel(float* __restrict__ p, const float* __restrict__ g, float* __restrict__ m,
                                                  float* __restrict__ v, int64_t n, double lr, double beta1, double beta2,
                                                  float eps, const int64_t* __restrict__ step_dev, int64_t step_host, float gs,
                                                  uint2* __restrict__ shadow, int64_t sh_b4, int64_t sh_e4, int sh_f16,
                                                  const int64_t* __restrict__ bad_step) {
    const int64_t ti = step_dev ? *step_dev + step_host : step_host;               // device counter + bias, or the host count
    // precision = "fp16": goalnet_grad_finite_check stamped this step as overflowed -> the whole update is skipped
    if (bad_step && *bad_step == ti) return;
    const BlockShare b = {0, 0, n, (int64_t)blockIdx.x, (int64_t)gridDim.x};
    range_pass<MODE_PLAIN, false>(p, g, m, v, nullptr, b, elem_scalars(adam_scalars(lr, beta1, beta2, ti), eps, gs),
                                  {shadow, sh_b4, sh_e4, sh_f16});
}

// The same update over the ranges of a RangeMap in ONE launch. Range r runs under its own step count *step + 1 - skipped[r]
// (torch.optim.Adam counts steps per parameter and skips those without a gradient); element for element the arithmetic is
// adam_kernel's, so the result equals that kernel run range by range.
struct SkippedSteps { int64_t skipped[GOALNET_ADAM_RANGES_MAX]; };

__global__ __launch_bounds__(256) void adam_ranges_kernel(float* __restrict__ p, const float* __restrict__ g, float* __restrict__ m,
                                                         float* __restrict__ v, RangeMap rs, SkippedSteps sk, int nranges, double lr,
                                                         double beta1, double beta2, float eps, const int64_t* __restrict__ step_dev,
                                                         float gs, uint2* __restrict__ shadow, int64_t sh_b4, int64_t sh_e4, int sh_f16,
                                                         const int64_t* __restrict__ bad_step) {
    const int64_t t1 = *step_dev + 1;                     // the step's own count: what goalnet_grad_finite_check stamps
    if (bad_step && *bad_step == t1) return;
    const BlockShare b = block_share(rs, nranges);
    range_pass<MODE_PLAIN, false>(p, g, m, v, nullptr, b, elem_scalars(adam_scalars(lr, beta1, beta2, t1 - sk.skipped[b.r]), eps, gs),
                                  {shadow, sh_b4, sh_e4, sh_f16});
}

// any non-finite value in g -> *bad_step = max(*bad_step, this step's 1-based count): the fused Adam of this step then returns
// without touching anything (adam_kernel); any number of blocks may write. The step's last launch
// (goalnet_counters_add4_guarded, stepstate.hip) keeps the step count where it is for a stamped step and clears the stamp.
__global__ __launch_bounds__(256) void grad_finite_check_kernel(const float* __restrict__ g, int64_t n, const int64_t* __restrict__ step,
                                                               int64_t step_bias, int64_t* __restrict__ bad_step,
                                                               int64_t* __restrict__ skipped) {
    bool bad = false;
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x) {
        const float v = g[i];
        bad |= (__float_as_uint(v) & 0x7f800000u) == 0x7f800000u;       // inf or nan: exponent all ones (FLT_MAX is finite)
    }
    if (__any(bad) && (threadIdx.x & 63) == 0) {
        const unsigned long long t = (unsigned long long)(*step + step_bias);
        const unsigned long long old = atomicMax(reinterpret_cast<unsigned long long*>(bad_step), t);
        if (old != t && skipped) atomicAdd(reinterpret_cast<unsigned long long*>(skipped), 1ull);       // first reporter of this step
    }
}

int adam_launch(const char* who, float* p, const float* g, float* m, float* v, int64_t n, double lr, double beta1, double beta2, double eps,
                const int64_t* step_dev, int64_t step_host, float grad_scale, void* stream, void* shadow = nullptr, int64_t sh_begin = 0,
                int64_t sh_count = 0, int sh_f16 = 0, const int64_t* bad_step = nullptr, int max_blocks = RANGE_BLOCKS_MAX) {
    GN_REQUIRE(p && g && m && v, GOALNET_E_NULL, "%s: null pointer", who);
    GN_REQUIRE(n > 0, GOALNET_E_SHAPE, "%s: bad count", who);
    GN_REQUIRE(aligned16(p) && aligned16(g) && aligned16(m) && aligned16(v), GOALNET_E_ALIGN, "%s: arenas must be 16-byte aligned", who);
    hipLaunchKernelGGL(adam_kernel, dim3((unsigned)blocks_for(n >> 2, max_blocks)), dim3(256), 0, (hipStream_t)stream, p, g, m, v, n, lr, beta1,
                       beta2, (float)eps, step_dev, step_host, grad_scale, (uint2*)shadow, sh_begin >> 2, (sh_begin + sh_count) >> 2, sh_f16,
                       bad_step);
    GN_LAUNCH_CHECK(who);
    return 0;
}

}  // namespace

extern "C" {

/* goalnet_adam_step_dev on at most max_blocks blocks of 256 threads: a BACKGROUND pass. The 10-frame step runs the update of
 * linear5.weight (90 % of the bytes) on its own stream under the rest of backward; on the default 8192 blocks it takes every CU and
 * all of the HBM bandwidth and the latency-bound kernels of the backward chain queue behind it, on ~128 blocks it streams at a
 * third of the bandwidth and leaves the chain alone. */
int goalnet_adam_step_dev_blocks(float* p, const float* g, float* m, float* v, int64_t n, double lr, double beta1, double beta2,
                                 double eps, const int64_t* step, int64_t step_bias, float grad_scale, int max_blocks, void* stream) {
    GN_REQUIRE(step, GOALNET_E_NULL, "adam_step_dev_blocks: null pointer");
    GN_REQUIRE(max_blocks >= 1 && max_blocks <= 65535, GOALNET_E_SHAPE, "adam_step_dev_blocks: 1..65535 blocks");
    return adam_launch("adam_step_dev_blocks", p, g, m, v, n, lr, beta1, beta2, eps, step, step_bias, grad_scale, stream, nullptr, 0, 0, 0, nullptr,
                       max_blocks);
}

int goalnet_adam_step_dev_shadow(float* p, const float* g, float* m, float* v, int64_t n, double lr, double beta1, double beta2,
                                 double eps, const int64_t* step, int64_t step_bias, float grad_scale, void* shadow_bf16,
                                 int64_t shadow_begin, int64_t shadow_count, int f16, void* stream) {
    GN_REQUIRE(step && shadow_bf16, GOALNET_E_NULL, "adam_step_dev_shadow: null pointer");
    const int rc = check_shadow("adam_step_dev_shadow", shadow_bf16, shadow_begin, shadow_count, n);
    if (rc != 0) return rc;
    return adam_launch("adam_step_dev_shadow", p, g, m, v, n, lr, beta1, beta2, eps, step, step_bias, grad_scale, stream, shadow_bf16,
                       shadow_begin, shadow_count, f16);
}

/* precision = "fp16" (loss-scaled gradients): the same two entry points with an overflow guard — the update is skipped when
 * goalnet_grad_finite_check stamped this step (*bad_step == *step + step_bias). shadow may be NULL. */
int goalnet_adam_step_dev_guarded(float* p, const float* g, float* m, float* v, int64_t n, double lr, double beta1, double beta2,
                                  double eps, const int64_t* step, int64_t step_bias, float grad_scale, void* shadow_16,
                                  int64_t shadow_begin, int64_t shadow_count, int f16, const int64_t* bad_step, void* stream) {
    GN_REQUIRE(step && bad_step, GOALNET_E_NULL, "adam_step_dev_guarded: null pointer");
    const int rc = check_shadow("adam_step_dev_guarded", shadow_16, shadow_begin, shadow_count, n);
    if (rc != 0) return rc;
    return adam_launch("adam_step_dev_guarded", p, g, m, v, n, lr, beta1, beta2, eps, step, step_bias, grad_scale, stream, shadow_16,
                       shadow_begin, shadow_16 ? shadow_count : 0, f16, bad_step);
}

/* goalnet_adam_step_dev[_guarded] over a list of arena ranges in one launch; range r runs under the count *step + 1 - skipped[r] */
int goalnet_adam_step_dev_ranges(float* p, const float* g, float* m, float* v, const goalnet_adam_range* ranges, int count, double lr,
                                 double beta1, double beta2, double eps, const int64_t* step, float grad_scale, void* shadow_16,
                                 int64_t shadow_begin, int64_t shadow_count, int f16, const int64_t* bad_step, void* stream) {
    const char* who = "adam_step_dev_ranges";
    GN_REQUIRE(p && g && m && v && ranges && step, GOALNET_E_NULL, "%s: null pointer", who);
    RangeMap rs;
    SkippedSteps sk;
    int rc = map_ranges(who, ranges, count, RANGE_BLOCKS_MAX, &rs);
    if (rc == 0) rc = copy_skipped(who, ranges, count, sk.skipped);
    if (rc != 0) return rc;
    GN_REQUIRE(aligned16(p) && aligned16(g) && aligned16(m) && aligned16(v), GOALNET_E_ALIGN, "%s: arenas must be 16-byte aligned", who);
    rc = check_shadow(who, shadow_16, shadow_begin, shadow_count, -1);
    if (rc != 0) return rc;
    hipLaunchKernelGGL(adam_ranges_kernel, dim3((unsigned)rs.first_block[count]), dim3(256), 0, (hipStream_t)stream, p, g, m, v, rs, sk, count, lr,
                       beta1, beta2, (float)eps, step, grad_scale, (uint2*)shadow_16, shadow_begin >> 2,
                       shadow_16 ? (shadow_begin + shadow_count) >> 2 : 0, f16, bad_step);
    GN_LAUNCH_CHECK(who);
    return 0;
}

int goalnet_grad_finite_check(const float* g, int64_t n, const int64_t* step, int64_t step_bias, int64_t* bad_step, int64_t* skipped,
                              void* stream) {
    GN_REQUIRE(g && step && bad_step, GOALNET_E_NULL, "grad_finite_check: null pointer");
    GN_REQUIRE(n > 0, GOALNET_E_SHAPE, "grad_finite_check: bad count");
    hipLaunchKernelGGL(grad_finite_check_kernel, dim3((unsigned)blocks_for(n, 1024)), dim3(256), 0, (hipStream_t)stream, g, n, step, step_bias,
                       bad_step, skipped);
    GN_LAUNCH_CHECK("grad_finite_check");
    return 0;
}

int goalnet_adam_step(float* p, const float* g, float* m, float* v, int64_t n, double lr, double beta1,
                      double beta2, double eps, int step, float grad_scale, void* stream) {
    GN_REQUIRE(step >= 1, GOALNET_E_SHAPE, "adam_step: step is 1-based");
    return adam_launch("adam_step", p, g, m, v, n, lr, beta1, beta2, eps, nullptr, step, grad_scale, stream);
}

int goalnet_adam_step_dev(float* p, const float* g, float* m, float* v, int64_t n, double lr, double beta1, double beta2,
                          double eps, const int64_t* step, int64_t step_bias, float grad_scale, void* stream) {
    GN_REQUIRE(step, GOALNET_E_NULL, "adam_step_dev: null step counter");
    return adam_launch("adam_step_dev", p, g, m, v, n, lr, beta1, beta2, eps, step, step_bias, grad_scale, stream);
}

}  // extern "C"
