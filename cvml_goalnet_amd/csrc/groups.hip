// Parameter groups and AMSGrad on the fused step (include/goalnet_groups.h): optim.hip's launch with a table of up
// to GOALNET_GROUPS_MAX hyper-parameter sets, one index per range, and a fourth state arena for the running maximum of v. Schedule,
// per-element expressions, block-to-range mapping, tail, 16-bit copy and guard are optim_impl.h's, which optim.hip compiles too: a
// range whose group carries the single-rate call's hyper-parameters and no AMSGrad gives goalnet_optim_step_dev_ranges' bits.
#include "../../include/goalnet_groups.h"
#include "optim_impl.h"

using namespace goalnet;

namespace {

struct GroupRanges {
    int64_t begin[GOALNET_ADAM_RANGES_MAX], count[GOALNET_ADAM_RANGES_MAX], skipped[GOALNET_ADAM_RANGES_MAX];
    int first_block[GOALNET_ADAM_RANGES_MAX + 1];
    uint32_t decay;                                      // bit r: weight decay applies to range r
    uint8_t group[GOALNET_ADAM_RANGES_MAX];              // range r runs under groups.h[group[r]]
};

struct GroupTable { goalnet_group_hyper h[GOALNET_GROUPS_MAX]; };

// HIP passes at most 4 KB of kernel arguments: the three structures by value, 10 pointers / 8-byte integers and 4 ints, with padding
static_assert(sizeof(GroupRanges) + sizeof(GroupTable) + sizeof(goalnet_optim_opts) + 10 * 8 + 4 * 8 <= 4096,
              "group_ranges_kernel's arguments must fit HIP's 4 KB");
static_assert(sizeof(goalnet_group_hyper) == 48 && sizeof(goalnet_group_range) == 32, "the layouts include/goalnet_groups.h documents");

__global__ void group_lr_kernel(goalnet_optim_opts o, const int64_t* __restrict__ step, double* __restrict__ lr_out) {
    if (blockIdx.x == 0 && threadIdx.x == 0) *lr_out = sched_lr(o, *step);
}

__global__ __launch_bounds__(256) void group_ranges_kernel(float* __restrict__ p, const float* __restrict__ g, float* __restrict__ m,
                                                          float* __restrict__ v, float* __restrict__ vmax, GroupRanges rs, int nranges,
                                                          GroupTable gt, goalnet_optim_opts o, const int64_t* __restrict__ step_dev, float gs,
                                                          const double* __restrict__ sumsq, uint2* __restrict__ shadow, int64_t sh_b4,
                                                          int64_t sh_e4, int sh_f16, const int64_t* __restrict__ bad_step) {
    const int64_t e = *step_dev, t1 = e + 1;              // t1: the step's own count, what goalnet_grad_finite_check stamps
    if (bad_step && *bad_step == t1) return;
    int r = 0;
    while (r + 1 < nranges && (int)blockIdx.x >= rs.first_block[r + 1]) ++r;
    const int64_t lb = (int)blockIdx.x - rs.first_block[r], nb = rs.first_block[r + 1] - rs.first_block[r];
    const goalnet_group_hyper h = gt.h[rs.group[r]];
    o.lr = h.lr;                                          // the schedule scales every group's own rate; min_lr is global
    const double lr_t = sched_lr(o, e);
    const AdamScalars sc = adam_scalars(lr_t, h.beta1, h.beta2, t1 - rs.skipped[r]);
    ElemScalars s;
    s.b2 = sc.b2; s.omb1 = sc.omb1; s.omb2 = sc.omb2; s.eps = (float)h.eps; s.step_size = sc.step_size; s.bc2_sqrt = sc.bc2_sqrt;
    s.gs = gs;
    s.coef = 1.0f;
    if (sumsq) {                                          // one norm over all groups, as clip_grad_norm_ over all parameters
        const double c = o.max_norm / ((double)gs * sqrt(*sumsq) + 1e-6);
        s.coef = (float)(c < 1.0 ? c : 1.0);
    }
    s.wd = (float)h.weight_decay;
    s.shrink = (float)(1.0 - lr_t * h.weight_decay);
    const bool decay = ((rs.decay >> r) & 1u) != 0 && h.weight_decay > 0.0;
    const int64_t begin = rs.begin[r], n = rs.count[r];
    if (h.amsgrad)
        range_dispatch<true>(decay, o.decoupled != 0, sumsq != nullptr, p, g, m, v, vmax, begin, n, lb, nb, s, shadow, sh_b4, sh_e4, sh_f16);
    else
        range_dispatch<false>(decay, o.decoupled != 0, sumsq != nullptr, p, g, m, v, nullptr, begin, n, lb, nb, s, shadow, sh_b4, sh_e4, sh_f16);
}

int check_group(const char* who, const goalnet_group_hyper& h, int k) {
    GN_REQUIRE(isfinite(h.lr) && isfinite(h.beta1) && isfinite(h.beta2) && isfinite(h.eps) && isfinite(h.weight_decay), GOALNET_E_VALUE,
               "%s: group %d holds a value that is not finite", who, k);
    GN_REQUIRE(h.lr >= 0.0, GOALNET_E_VALUE, "%s: group %d: lr must be >= 0", who, k);
    GN_REQUIRE(h.beta1 >= 0.0 && h.beta1 < 1.0 && h.beta2 >= 0.0 && h.beta2 < 1.0, GOALNET_E_VALUE, "%s: group %d: betas must lie in [0, 1)", who, k);
    GN_REQUIRE(h.eps >= 0.0, GOALNET_E_VALUE, "%s: group %d: eps must be >= 0", who, k);
    GN_REQUIRE(h.weight_decay >= 0.0, GOALNET_E_VALUE, "%s: group %d: weight_decay must be >= 0", who, k);
    return 0;
}

}  // namespace

extern "C" {

int goalnet_group_step_dev_ranges(float* p, const float* g, float* m, float* v, float* vmax, const goalnet_group_range* ranges, int count,
                                  const goalnet_group_hyper* groups, int ngroups, const goalnet_optim_opts* opts, const int64_t* step,
                                  float grad_scale, const double* sumsq, void* shadow_16, int64_t shadow_begin, int64_t shadow_count,
                                  int f16, const int64_t* bad_step, void* stream) {
    const char* who = "group_step_dev_ranges";
    GN_REQUIRE(p && g && m && v && step && groups, GOALNET_E_NULL, "%s: null pointer", who);
    GroupRanges rs;
    int rc = check_ranges(who, ranges, count, OPTIM_BLOCKS_MAX, rs.begin, rs.count, rs.skipped, &rs.decay, rs.first_block);
    if (rc != 0) return rc;
    rc = check_opts(who, opts);
    if (rc != 0) return rc;
    GN_REQUIRE(ngroups >= 1 && ngroups <= GOALNET_GROUPS_MAX, GOALNET_E_SHAPE, "%s: 1..%d groups", who, GOALNET_GROUPS_MAX);
    GroupTable gt;
    for (int k = 0; k < GOALNET_GROUPS_MAX; ++k) {
        gt.h[k] = groups[k < ngroups ? k : 0];            // the unused tail repeats the default group: no uninitialised bytes in a graph
        if (k < ngroups && (rc = check_group(who, groups[k], k)) != 0) return rc;
    }
    bool ams = false;
    for (int r = 0; r < count; ++r) {
        GN_REQUIRE(ranges[r].group >= 0 && ranges[r].group < ngroups, GOALNET_E_SHAPE, "%s: range %d: group %d outside 0..%d", who, r,
                   ranges[r].group, ngroups - 1);
        rs.group[r] = (uint8_t)ranges[r].group;
        ams = ams || groups[ranges[r].group].amsgrad != 0;
    }
    for (int r = count; r < GOALNET_ADAM_RANGES_MAX; ++r) rs.group[r] = 0;
    GN_REQUIRE(!ams || vmax, GOALNET_E_VALUE, "%s: a group with amsgrad needs the vmax arena", who);
    rc = check_step_args(who, p, g, m, v, opts, sumsq, shadow_16, shadow_begin, shadow_count);
    if (rc != 0) return rc;
    GN_REQUIRE(aligned16(vmax), GOALNET_E_ALIGN, "%s: arenas must be 16-byte aligned", who);
    hipLaunchKernelGGL(group_ranges_kernel, dim3((unsigned)rs.first_block[count]), dim3(256), 0, (hipStream_t)stream, p, g, m, v,
                       ams ? vmax : nullptr, rs, count, gt, *opts, step, grad_scale, sumsq, (uint2*)shadow_16, shadow_begin >> 2,
                       shadow_16 ? (shadow_begin + shadow_count) >> 2 : 0, f16, bad_step);
    GN_LAUNCH_CHECK("group_step_dev_ranges");
    return 0;
}

int goalnet_group_lr(const goalnet_optim_opts* opts, const goalnet_group_hyper* groups, int g, const int64_t* step, double* lr_out,
                     void* stream) {
    GN_REQUIRE(step && lr_out && groups, GOALNET_E_NULL, "group_lr: null pointer");
    int rc = check_opts("group_lr", opts);
    if (rc != 0) return rc;
    GN_REQUIRE(g >= 0 && g < GOALNET_GROUPS_MAX, GOALNET_E_SHAPE, "group_lr: group %d outside 0..%d", g, GOALNET_GROUPS_MAX - 1);
    rc = check_group("group_lr", groups[g], g);
    if (rc != 0) return rc;
    goalnet_optim_opts o = *opts;
    o.lr = groups[g].lr;
    hipLaunchKernelGGL(group_lr_kernel, dim3(1), dim3(64), 0, (hipStream_t)stream, o, step, lr_out);
    GN_LAUNCH_CHECK("group_lr");
    return 0;
}

}  // extern "C"
