// What the two optimizer launches share (optim.hip: one set of hyper-parameters; groups.hip: a table of them and
// AMSGrad): the schedule, the per-element expressions, the pass of one block over its share of a range with the tail
// and the 16-bit copy, and the host checks. Both sources compile these lines, so a range that runs under the same scalars gives the
// same bits from either launch.
#pragma once
#include <hip/hip_bf16.h>
#include <math.h>

#include "../../include/goalnet_optim.h"
#include "adam.h"
#include "common.h"

namespace goalnet {

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

// what a block does to its range's elements beyond Adam: chosen once per block, uniform over it
enum { MODE_PLAIN = 0, MODE_CLIP = 1, MODE_COUPLED = 2, MODE_DECOUPLED = 3 };

struct ElemScalars { float b2, omb1, omb2, eps, step_size, bc2_sqrt, gs, coef, wd, shrink; };

// AMS: the update keeps the running maximum of v in vm (adam1_amsgrad); otherwise vm is not looked at
template <int MODE, bool AMS>
__device__ __forceinline__ void optim1(float& p, float g, float& m, float& v, float& vm, const ElemScalars& s) {
    if (MODE == MODE_PLAIN) {                             // adam_ranges_kernel's expression, grad_scale inside adam1
        if (AMS) adam1_amsgrad(p, g, m, v, vm, s.b2, s.omb1, s.omb2, s.eps, s.step_size, s.bc2_sqrt, s.gs);
        else adam1(p, g, m, v, s.b2, s.omb1, s.omb2, s.eps, s.step_size, s.bc2_sqrt, s.gs);
        return;
    }
    g *= s.gs;                                            // the unscaled gradient, rounded as torch holds it
    g *= s.coef;                                          // clip_grad_norm_: grads.mul_(coef), 1.0f where clipping is off
    if (MODE == MODE_COUPLED) g = g + s.wd * p;           // grad.add(param, alpha = weight_decay)
    if (MODE == MODE_DECOUPLED) p = p * s.shrink;         // param.mul_(1 - lr * weight_decay)
    if (AMS) adam1_amsgrad(p, g, m, v, vm, s.b2, s.omb1, s.omb2, s.eps, s.step_size, s.bc2_sqrt, 1.0f);
    else adam1(p, g, m, v, s.b2, s.omb1, s.omb2, s.eps, s.step_size, s.bc2_sqrt, 1.0f);
}

// vmax: the fourth state arena, read and written only under AMS (it may be null otherwise)
template <int MODE, bool AMS>
__device__ __forceinline__ void range_pass(float* __restrict__ p, const float* __restrict__ g, float* __restrict__ m, float* __restrict__ v,
                                           float* __restrict__ vmax, int64_t begin, int64_t n, int64_t lb, int64_t nb, const ElemScalars& s,
                                           uint2* __restrict__ shadow, int64_t sh_b4, int64_t sh_e4, int sh_f16) {
    const int64_t b4 = begin >> 2, n4 = n >> 2;
    for (int64_t j = lb * blockDim.x + threadIdx.x; j < n4; j += nb * blockDim.x) {
        const int64_t i = b4 + j;                         // float4 index in the arena
        float4 pp = reinterpret_cast<float4*>(p)[i];
        const float4 gg = reinterpret_cast<const float4*>(g)[i];
        float4 mm = reinterpret_cast<float4*>(m)[i];
        float4 vv = reinterpret_cast<float4*>(v)[i];
        float4 xx = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
        if (AMS) xx = reinterpret_cast<float4*>(vmax)[i];
        optim1<MODE, AMS>(pp.x, gg.x, mm.x, vv.x, xx.x, s);
        optim1<MODE, AMS>(pp.y, gg.y, mm.y, vv.y, xx.y, s);
        optim1<MODE, AMS>(pp.z, gg.z, mm.z, vv.z, xx.z, s);
        optim1<MODE, AMS>(pp.w, gg.w, mm.w, vv.w, xx.w, s);
        reinterpret_cast<float4*>(p)[i] = pp;
        reinterpret_cast<float4*>(m)[i] = mm;
        reinterpret_cast<float4*>(v)[i] = vv;
        if (AMS) reinterpret_cast<float4*>(vmax)[i] = xx;
        if (shadow && i >= sh_b4 && i < sh_e4) shadow[i - sh_b4] = pack4_16(pp, sh_f16);
    }
    if (lb == 0 && threadIdx.x < (n & 3)) {
        const int64_t i = begin + (n4 << 2) + threadIdx.x;
        float x = 0.0f;
        if (AMS) x = vmax[i];
        optim1<MODE, AMS>(p[i], g[i], m[i], v[i], x, s);
        if (AMS) vmax[i] = x;
    }
}

// one block's pass under the mode its range runs in: decay (coupled or decoupled), else clipping, else plain Adam
template <bool AMS>
__device__ __forceinline__ void range_dispatch(bool decay, bool decoupled, bool clip, float* __restrict__ p, const float* __restrict__ g,
                                               float* __restrict__ m, float* __restrict__ v, float* __restrict__ vmax, int64_t begin,
                                               int64_t n, int64_t lb, int64_t nb, const ElemScalars& s, uint2* __restrict__ shadow,
                                               int64_t sh_b4, int64_t sh_e4, int sh_f16) {
    if (decay && decoupled) range_pass<MODE_DECOUPLED, AMS>(p, g, m, v, vmax, begin, n, lb, nb, s, shadow, sh_b4, sh_e4, sh_f16);
    else if (decay) range_pass<MODE_COUPLED, AMS>(p, g, m, v, vmax, begin, n, lb, nb, s, shadow, sh_b4, sh_e4, sh_f16);
    else if (clip) range_pass<MODE_CLIP, AMS>(p, g, m, v, vmax, begin, n, lb, nb, s, shadow, sh_b4, sh_e4, sh_f16);
    else range_pass<MODE_PLAIN, AMS>(p, g, m, v, vmax, begin, n, lb, nb, s, shadow, sh_b4, sh_e4, sh_f16);
}

// ---- host: the checks the entry points share ------------------------------------------------------------------------------------------
constexpr int OPTIM_BLOCKS_MAX = 8192;                   // per range, in the update launches

inline int blocks_for(int64_t n4, int cap) {
    int64_t b = (n4 + 255) / 256;
    if (b > cap) b = cap;
    if (b < 1) b = 1;
    return (int)b;
}

// Range: goalnet_optim_range or goalnet_group_range (the same ordering, alignment and count rules); *total_blocks: blocks of a launch
// with at most `cap` blocks per range
template <class Range>
inline int check_ranges(const char* who, const Range* ranges, int count, int cap, int64_t* begin, int64_t* cnt, int64_t* skipped,
                        uint32_t* decay, int* first_block) {
    GN_REQUIRE(ranges, GOALNET_E_NULL, "%s: null pointer", who);
    GN_REQUIRE(count >= 1 && count <= GOALNET_ADAM_RANGES_MAX, GOALNET_E_SHAPE, "%s: 1..%d ranges", who, GOALNET_ADAM_RANGES_MAX);
    int64_t end = 0;
    first_block[0] = 0;
    if (decay) *decay = 0;
    for (int r = 0; r < count; ++r) {
        const Range& a = ranges[r];
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

inline int check_opts(const char* who, const goalnet_optim_opts* o) {
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

// what both update launches require of their pointers beyond the ranges and options
inline int check_step_args(const char* who, const void* p, const void* g, const void* m, const void* v, const goalnet_optim_opts* opts,
                           const double* sumsq, const void* shadow_16, int64_t shadow_begin, int64_t shadow_count) {
    GN_REQUIRE(aligned16(p) && aligned16(g) && aligned16(m) && aligned16(v), GOALNET_E_ALIGN, "%s: arenas must be 16-byte aligned", who);
    GN_REQUIRE(!(opts->max_norm > 0.0) || sumsq, GOALNET_E_NULL, "%s: max_norm > 0 needs the gradient's sum of squares", who);
    GN_REQUIRE(opts->max_norm > 0.0 || !sumsq, GOALNET_E_VALUE, "%s: a sum of squares without max_norm > 0", who);
    GN_REQUIRE(!sumsq || (reinterpret_cast<uintptr_t>(sumsq) & 7u) == 0, GOALNET_E_ALIGN, "%s: sumsq must be 8-byte aligned", who);
    if (shadow_16) {
        GN_REQUIRE(shadow_begin >= 0 && shadow_count > 0 && (shadow_begin & 3) == 0 && (shadow_count & 3) == 0, GOALNET_E_SHAPE,
                   "%s: the shadowed slice's offset and length must be multiples of 4", who);
        GN_REQUIRE((reinterpret_cast<uintptr_t>(shadow_16) & 7u) == 0, GOALNET_E_ALIGN, "%s: shadow must be 8-byte aligned", who);
    }
    return 0;
}

}  // namespace goalnet
