// What the update launches share (adam.hip: plain Adam; optim.hip: one set of hyper-parameters and options, DESIGN.md §4.14;
// groups.hip: a table of them and AMSGrad): the schedule, the per-element expressions, the pass of one block over its
// share of a range (ranges.h) with the 16-bit copy, and the host checks. Every source compiles these lines, so a range that runs under
// the same scalars gives the same bits from any of the launches.
#pragma once
#include <hip/hip_bf16.h>
#include <math.h>

#include "../../include/goalnet_optim.h"
#include "adam.h"
#include "ranges.h"

namespace goalnet {

// ---- the schedule: fp64, one evaluation per thread next to adam_scalars' pow -------------------------------------------------------
// lr: the base rate the schedule scales (the options' own, or a parameter group's); o.lr is not read
__device__ __forceinline__ double sched_lr(const goalnet_optim_opts& o, double lr, int64_t e) {
    if (e < o.warmup) return lr * (double)(e + 1) / (double)o.warmup;
    if (o.schedule == GOALNET_SCHED_COSINE) {
        const int64_t T = o.total - o.warmup, e1 = e - o.warmup;
        return o.min_lr + (lr - o.min_lr) * (1.0 + cos(M_PI * (double)(e1 < T ? e1 : T) / (double)T)) / 2.0;
    }
    if (o.schedule == GOALNET_SCHED_STEP) return lr * pow(o.gamma, (double)((e - o.warmup) / o.period));
    return lr;
}

// *lr_out = sched_lr(o, o.lr, *step) on one thread: optim.hip's launch behind goalnet_optim_lr and goalnet_group_lr
int launch_sched_lr(const char* who, const goalnet_optim_opts& o, const int64_t* step, double* lr_out, void* stream);

// four updated parameters as binary16 (f16 != 0) or bfloat16, packed for one 8-byte store into the 16-bit copy
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

// the 16-bit copy of the updated parameters of one slice (the next step's GEMM operand): float4s [b4, e4) of the arena; out may be null
struct Shadow16 {
    uint2* __restrict__ out;
    int64_t b4, e4;
    int f16;
};

// One block's pass over its share (ranges.h). vmax: the fourth state arena, read and written only under AMS (it may be null otherwise)
template <int MODE, bool AMS>
__device__ __forceinline__ void range_pass(float* __restrict__ p, const float* __restrict__ g, float* __restrict__ m, float* __restrict__ v,
                                           float* __restrict__ vmax, const BlockShare& b, const ElemScalars& s, const Shadow16& sh) {
    for_share(
        b,
        [&](int64_t i) {
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
            if (sh.out && i >= sh.b4 && i < sh.e4) sh.out[i - sh.b4] = pack4_16(pp, sh.f16);
        },
        [&](int64_t i) {
            float x = 0.0f;
            if (AMS) x = vmax[i];
            optim1<MODE, AMS>(p[i], g[i], m[i], v[i], x, s);
            if (AMS) vmax[i] = x;
        });
}

// plain Adam's scalars for range_pass<MODE_PLAIN, .>: what the other modes read beyond them is neutral
__device__ __forceinline__ ElemScalars elem_scalars(const AdamScalars& sc, float eps, float gs) {
    return {sc.b2, sc.omb1, sc.omb2, eps, sc.step_size, sc.bc2_sqrt, gs, 1.0f, 0.0f, 1.0f};
}

// one block's pass under the mode its range runs in: decay (coupled or decoupled), else clipping, else plain Adam
template <bool AMS>
__device__ __forceinline__ void range_dispatch(bool decay, bool decoupled, bool clip, float* __restrict__ p, const float* __restrict__ g,
                                               float* __restrict__ m, float* __restrict__ v, float* __restrict__ vmax, const BlockShare& b,
                                               const ElemScalars& s, const Shadow16& sh) {
    if (decay && decoupled) range_pass<MODE_DECOUPLED, AMS>(p, g, m, v, vmax, b, s, sh);
    else if (decay) range_pass<MODE_COUPLED, AMS>(p, g, m, v, vmax, b, s, sh);
    else if (clip) range_pass<MODE_CLIP, AMS>(p, g, m, v, vmax, b, s, sh);
    else range_pass<MODE_PLAIN, AMS>(p, g, m, v, vmax, b, s, sh);
}

// One block of an update launch (optim.hip, groups.hip) under the hyper-parameters of its range: the rate of the step that starts from
// e completed steps, Adam's scalars at the range's own count, the clip coefficient, and the pass in the range's mode. `o` gives the
// schedule, max_norm and decoupled; its own lr, betas, eps and weight_decay are not read.
__device__ __forceinline__ void optim_block(float* __restrict__ p, const float* __restrict__ g, float* __restrict__ m, float* __restrict__ v,
                                            float* __restrict__ vmax, const BlockShare& b, int64_t skipped, bool decays,
                                            const goalnet_optim_opts& o, double lr, double beta1, double beta2, double eps, double weight_decay,
                                            bool amsgrad, int64_t e, float gs, const double* __restrict__ sumsq, const Shadow16& sh) {
    const double lr_t = sched_lr(o, lr, e);               // the global count: every range of a group runs at the same rate
    ElemScalars s = elem_scalars(adam_scalars(lr_t, beta1, beta2, e + 1 - skipped), (float)eps, gs);
    if (sumsq) {                                          // one norm over all ranges, as clip_grad_norm_ over all parameters
        const double c = o.max_norm / ((double)gs * sqrt(*sumsq) + 1e-6);
        s.coef = (float)(c < 1.0 ? c : 1.0);
    }
    s.wd = (float)weight_decay;
    s.shrink = (float)(1.0 - lr_t * weight_decay);
    const bool decay = decays && weight_decay > 0.0;
    if (amsgrad) range_dispatch<true>(decay, o.decoupled != 0, sumsq != nullptr, p, g, m, v, vmax, b, s, sh);
    else range_dispatch<false>(decay, o.decoupled != 0, sumsq != nullptr, p, g, m, v, nullptr, b, s, sh);
}

// ---- host: the checks the entry points share (the ranges' and the shadow's are ranges.h's) --------------------------------------------
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
    return check_shadow(who, shadow_16, shadow_begin, shadow_count, -1);
}

// the steps each range sat out, for the launches whose ranges carry them: none may be negative. skipped[MAX] (nullable: check only)
// receives them, zero beyond `count`
template <class Range>
inline int copy_skipped(const char* who, const Range* ranges, int count, int64_t* skipped) {
    for (int r = 0; r < GOALNET_ADAM_RANGES_MAX; ++r) {
        GN_REQUIRE(r >= count || ranges[r].skipped >= 0, GOALNET_E_SHAPE, "%s: range %d: negative count of skipped steps", who, r);
        if (skipped) skipped[r] = r < count ? ranges[r].skipped : 0;
    }
    return 0;
}

}  // namespace goalnet
