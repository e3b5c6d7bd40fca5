// Optimizer options on the fused step (include/goalnet_optim.h): weight decay (coupled as torch.optim.Adam's,
// decoupled as torch.optim.AdamW's), clipping by the global gradient norm (torch.nn.utils.clip_grad_norm_) and a learning-rate
// schedule evaluated on the device from the step counter, so that a captured graph follows it. The per-element update and its
// scalars are adam.h's (adam1, adam_scalars), included: a range that no option touches runs adam_ranges_kernel's own loop
// (small.hip) and gives its bits. Block-to-range mapping, tail, 16-bit copy and guard are that kernel's too.
#include <hip/hip_bf16.h>
#include <math.h>

#include "../../include/goalnet_optim.h"
#include "adam.h"
#include "common.h"

using namespace goalnet;

namespace {

// ---- the schedule: fp64, one evaluation per thread next to adam_scalars' pow -------------------------------------------------------
__device__ __forceinline__ double sched_lr(const goalnet_optim_opts& o, int64_t e) {
    if (e < o.warmup) return o.lr * (double)(e + 1) / (double)o.warmup;
    if (o.schedule == GOALNET_SCHED_COSINE) {
        const int64_t T = o.total - o.warmup, e1 = e - o.warmup;
        return o.min_lr + (o.lr - o.min_lr) * (1.0 + cos(M_PI * (double)(e1 < T ? e1 : T) / (double)T)) / 2.0;
    }
    if (o.schedule == GOALNET_SCHED_STEP) return o.lr * pow(o.gamma, (double)((e - o.warmup) / o.period));
    return o.lr;
}

__global__ void optim_lr_kernel(goalnet_optim_opts o, const int64_t* __restrict__ step, double* __restrict__ lr_out) {
    if (blockIdx.x == 0 && threadIdx.x == 0) *lr_out = sched_lr(o, *step);
}

// four updated parameters as binary16 (f16 != 0) or bfloat16, packed for one 8-byte store into the 16-bit copy (small.hip's pack4_16)
__device__ __forceinline__ uint2 pack4_16(const float4& pp, int f16) {
    if (f16) {
        const _Float16 a = (_Float16)pp.x, b = (_Float16)pp.y, c = (_Float16)pp.z, d = (_Float16)pp.w;
        return make_uint2((unsigned)__builtin_bit_cast(unsigned short, a) | ((unsigned)__builtin_bit_cast(unsigned short, b) << 16),
                          (unsigned)__builtin_bit_cast(unsigned short, c) | ((unsigned)__builtin_bit_cast(unsigned short, d) << 16));
    }
    const __hip_bfloat16 a = __float2bfloat16(pp.x), b = __float2bfloat16(pp.y), c = __float2bfloat16(pp.z), d = __float2bfloat16(pp.w);
    return make_uint2((unsigned)*reinterpret_cast<const unsigned short*>(&a) | ((unsigned)*reinterpret_cast<const unsigned short*>(&b) << 16),
                      (unsigned)*reinterpret_cast<const unsigned short*>(&c) | ((unsigned)*reinterpret_cast<const unsigned short*>(&d) << 16));
}

struct OptimRanges {
    int64_t begin[GOALNET_ADAM_RANGES_MAX], count[GOALNET_ADAM_RANGES_MAX], skipped[GOALNET_ADAM_RANGES_MAX];
    int first_block[GOALNET_ADAM_RANGES_MAX + 1];
    uint32_t decay;                                      // bit r: weight decay applies to range r
};

// what a block does to its range's elements beyond Adam: chosen once per block, uniform over it
enum { MODE_PLAIN = 0, MODE_CLIP = 1, MODE_COUPLED = 2, MODE_DECOUPLED = 3 };

struct ElemScalars { float b2, omb1, omb2, eps, step_size, bc2_sqrt, gs, coef, wd, shrink; };

template <int MODE>
__device__ __forceinline__ void optim1(float& p, float g, float& m, float& v, const ElemScalars& s) {
    if (MODE == MODE_PLAIN) {                             // adam_ranges_kernel's expression, grad_scale inside adam1
        adam1(p, g, m, v, s.b2, s.omb1, s.omb2, s.eps, s.step_size, s.bc2_sqrt, s.gs);
        return;
    }
    g *= s.gs;                                            // the unscaled gradient, rounded as torch holds it
    g *= s.coef;                                          // clip_grad_norm_: grads.mul_(coef), 1.0f where clipping is off
    if (MODE == MODE_COUPLED) g = g + s.wd * p;           // grad.add(param, alpha = weight_decay)
    if (MODE == MODE_DECOUPLED) p = p * s.shrink;         // param.mul_(1 - lr * weight_decay)
    adam1(p, g, m, v, s.b2, s.omb1, s.omb2, s.eps, s.step_size, s.bc2_sqrt, 1.0f);
}

template <int MODE>
__device__ __forceinline__ void range_pass(float* __restrict__ p, const float* __restrict__ g, float* __restrict__ m, float* __restrict__ v,
                                           int64_t begin, int64_t n, int64_t lb, int64_t nb, const ElemScalars& s,
                                           uint2* __restrict__ shadow, int64_t sh_b4, int64_t sh_e4, int sh_f16) {
    const int64_t b4 = begin >> 2, n4 = n >> 2;
    for (int64_t j = lb * blockDim.x + threadIdx.x; j < n4; j += nb * blockDim.x) {
        const int64_t i = b4 + j;                         // float4 index in the arena
        float4 pp = reinterpret_cast<float4*>(p)[i];
        const float4 gg = reinterpret_cast<const float4*>(g)[i];
        float4 mm = reinterpret_cast<float4*>(m)[i];
        float4 vv = reinterpret_cast<float4*>(v)[i];
        optim1<MODE>(pp.x, gg.x, mm.x, vv.x, s);
        optim1<MODE>(pp.y, gg.y, mm.y, vv.y, s);
        optim1<MODE>(pp.z, gg.z, mm.z, vv.z, s);
        optim1<MODE>(pp.w, gg.w, mm.w, vv.w, s);
        reinterpret_cast<float4*>(p)[i] = pp;
        reinterpret_cast<float4*>(m)[i] = mm;
        reinterpret_cast<float4*>(v)[i] = vv;
        if (shadow && i >= sh_b4 && i < sh_e4) shadow[i - sh_b4] = pack4_16(pp, sh_f16);
    }
    if (lb == 0 && threadIdx.x < (n & 3)) {
        const int64_t i = begin + (n4 << 2) + threadIdx.x;
        optim1<MODE>(p[i], g[i], m[i], v[i], s);
    }
}

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
    if (decay && o.decoupled) range_pass<MODE_DECOUPLED>(p, g, m, v, begin, n, lb, nb, s, shadow, sh_b4, sh_e4, sh_f16);
    else if (decay) range_pass<MODE_COUPLED>(p, g, m, v, begin, n, lb, nb, s, shadow, sh_b4, sh_e4, sh_f16);
    else if (sumsq) range_pass<MODE_CLIP>(p, g, m, v, begin, n, lb, nb, s, shadow, sh_b4, sh_e4, sh_f16);
    else range_pass<MODE_PLAIN>(p, g, m, v, begin, n, lb, nb, s, shadow, sh_b4, sh_e4, sh_f16);
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

int blocks_for(int64_t n4, int cap) {
    int64_t b = (n4 + 255) / 256;
    if (b > cap) b = cap;
    if (b < 1) b = 1;
    return (int)b;
}

// the checks both entry points share; *total_blocks: blocks of a launch with at most `cap` blocks per range
int check_ranges(const char* who, const goalnet_optim_range* ranges, int count, int cap, int64_t* begin, int64_t* cnt, int64_t* skipped,
                 uint32_t* decay, int* first_block) {
    GN_REQUIRE(ranges, GOALNET_E_NULL, "%s: null pointer", who);
    GN_REQUIRE(count >= 1 && count <= GOALNET_ADAM_RANGES_MAX, GOALNET_E_SHAPE, "%s: 1..%d ranges", who, GOALNET_ADAM_RANGES_MAX);
    int64_t end = 0;
    first_block[0] = 0;
    if (decay) *decay = 0;
    for (int r = 0; r < count; ++r) {
        const goalnet_optim_range& a = ranges[r];
        GN_REQUIRE(a.begin >= 0 && a.count > 0, GOALNET_E_SHAPE, "%s: range %d is empty or starts below 0", who, r);
        GN_REQUIRE(a.skipped >= 0, GOALNET_E_SHAPE, "%s: range %d: negative count of skipped steps", who, r);
        GN_REQUIRE((a.begin & 3) == 0, GOALNET_E_ALIGN, "%s: range %d must begin at a multiple of 4 elements", who, r);
        GN_REQUIRE(a.begin >= end, GOALNET_E_SHAPE, "%s: range %d overlaps its predecessor or is out of order", who, r);
        end = a.begin + a.count;
        begin[r] = a.begin; cnt[r] = a.count;
        if (skipped) skipped[r] = a.skipped;
        if (decay && a.decay) *decay |= 1u << r;
        first_block[r + 1] = first_block[r] + blocks_for(a.count >> 2, cap);
    }
    return 0;
}

int check_opts(const char* who, const goalnet_optim_opts* o) {
    GN_REQUIRE(o, GOALNET_E_NULL, "%s: null options", who);
    GN_REQUIRE(o->weight_decay >= 0.0 && isfinite(o->weight_decay), GOALNET_E_VALUE, "%s: weight_decay must be finite and >= 0", who);
    GN_REQUIRE(!isnan(o->max_norm), GOALNET_E_VALUE, "%s: max_norm is not a number", who);
    GN_REQUIRE(o->schedule >= GOALNET_SCHED_CONSTANT && o->schedule <= GOALNET_SCHED_STEP, GOALNET_E_VALUE, "%s: unknown schedule %d", who,
               o->schedule);
    GN_REQUIRE(o->warmup >= 0, GOALNET_E_VALUE, "%s: warmup must be >= 0", who);
    GN_REQUIRE(o->min_lr >= 0.0 && isfinite(o->min_lr), GOALNET_E_VALUE, "%s: min_lr must be finite and >= 0", who);
    if (o->schedule == GOALNET_SCHED_COSINE)
        GN_REQUIRE(o->total > o->warmup, GOALNET_E_VALUE, "%s: the cosine schedule needs total > warmup", who);
    if (o->schedule == GOALNET_SCHED_STEP)
        GN_REQUIRE(o->period >= 1 && o->gamma > 0.0 && isfinite(o->gamma), GOALNET_E_VALUE, "%s: the step schedule needs period >= 1 and gamma > 0",
                   who);
    return 0;
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
    int rc = check_ranges("optim_step_dev_ranges", ranges, count, 8192, rs.begin, rs.count, rs.skipped, &rs.decay, rs.first_block);
    if (rc != 0) return rc;
    rc = check_opts("optim_step_dev_ranges", opts);
    if (rc != 0) return rc;
    GN_REQUIRE(aligned16(p) && aligned16(g) && aligned16(m) && aligned16(v), GOALNET_E_ALIGN, "optim_step_dev_ranges: arenas must be 16-byte aligned");
    GN_REQUIRE(!(opts->max_norm > 0.0) || sumsq, GOALNET_E_NULL, "optim_step_dev_ranges: max_norm > 0 needs the gradient's sum of squares");
    GN_REQUIRE(opts->max_norm > 0.0 || !sumsq, GOALNET_E_VALUE, "optim_step_dev_ranges: a sum of squares without max_norm > 0");
    GN_REQUIRE(!sumsq || (reinterpret_cast<uintptr_t>(sumsq) & 7u) == 0, GOALNET_E_ALIGN, "optim_step_dev_ranges: sumsq must be 8-byte aligned");
    if (shadow_16) {
        GN_REQUIRE(shadow_begin >= 0 && shadow_count > 0 && (shadow_begin & 3) == 0 && (shadow_count & 3) == 0, GOALNET_E_SHAPE,
                   "optim_step_dev_ranges: the shadowed slice's offset and length must be multiples of 4");
        GN_REQUIRE((reinterpret_cast<uintptr_t>(shadow_16) & 7u) == 0, GOALNET_E_ALIGN, "optim_step_dev_ranges: shadow must be 8-byte aligned");
    }
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
