// Parameter groups and AMSGrad on the fused step (include/goalnet_groups.h): optim.hip's launch with a table of up
// to GOALNET_GROUPS_MAX hyper-parameter sets, one index per range, and a fourth state arena for the running maximum of v. Schedule,
// per-element expressions, 16-bit copy and the block's whole pass (optim_block) are optim_impl.h's, which optim.hip compiles too;
// block-to-range mapping and tail are ranges.h's. A range whose group carries the single-rate call's hyper-parameters and no AMSGrad
// gives goalnet_optim_step_dev_ranges' bits.
#include "../../include/goalnet_groups.h"
#include "optim_impl.h"

using namespace goalnet;

namespace {

struct GroupSteps {
    int64_t skipped[GOALNET_ADAM_RANGES_MAX];
    uint64_t decay;                                      // bit r: weight decay applies to range r
    uint8_t group[GOALNET_ADAM_RANGES_MAX];              // range r runs under GroupTable::h[group[r]]
};

struct GroupTable { goalnet_group_hyper h[GOALNET_GROUPS_MAX]; };

// HIP passes at most 4 KB of kernel arguments: the four structures by value (648 + 296 + 384 + 96 bytes), 10 pointers / 8-byte integers
// and 4 ints, with padding
static_assert(sizeof(RangeMap) + sizeof(GroupSteps) + sizeof(GroupTable) + sizeof(goalnet_optim_opts) + 10 * 8 + 4 * 8 <= 4096,
              "group_ranges_kernel's arguments must fit HIP's 4 KB");
static_assert(sizeof(goalnet_group_hyper) == 48 && sizeof(goalnet_group_range) == 32, "the layouts include/goalnet_groups.h documents");

__global__ __launch_bounds__(256) void group_ranges_kernel(float* __restrict__ p, const float* __restrict__ g, float* __restrict__ m,
                                                          float* __restrict__ v, float* __restrict__ vmax, RangeMap rs, GroupSteps st,
                                                          int nranges, GroupTable gt, goalnet_optim_opts o, const int64_t* __restrict__ step_dev,
                                                          float gs, const double* __restrict__ sumsq, uint2* __restrict__ shadow, int64_t sh_b4,
                                                          int64_t sh_e4, int sh_f16, const int64_t* __restrict__ bad_step) {
    const int64_t e = *step_dev;                          // e + 1: the step's own count, what goalnet_grad_finite_check stamps
    if (bad_step && *bad_step == e + 1) return;
    const BlockShare b = block_share(rs, nranges);
    const goalnet_group_hyper h = gt.h[st.group[b.r]];    // the schedule scales every group's own rate; min_lr is global
    optim_block(p, g, m, v, vmax, b, st.skipped[b.r], ((st.decay >> b.r) & 1u) != 0, o, h.lr, h.beta1, h.beta2, h.eps, h.weight_decay,
                h.amsgrad != 0, e, gs, sumsq, {shadow, sh_b4, sh_e4, sh_f16});
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
    RangeMap rs;
    GroupSteps st;
    memset(&st, 0, sizeof st);                            // the entries beyond `count` too: no uninitialised bytes in a graph
    int rc = map_ranges(who, ranges, count, RANGE_BLOCKS_MAX, &rs);
    if (rc == 0) rc = copy_skipped(who, ranges, count, st.skipped);
    if (rc == 0) rc = check_opts(who, opts);
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
        st.group[r] = (uint8_t)ranges[r].group;
        st.decay |= (uint64_t)(ranges[r].decay != 0) << r;
        ams = ams || groups[ranges[r].group].amsgrad != 0;
    }
    GN_REQUIRE(!ams || vmax, GOALNET_E_VALUE, "%s: a group with amsgrad needs the vmax arena", who);
    rc = check_step_args(who, p, g, m, v, opts, sumsq, shadow_16, shadow_begin, shadow_count);
    if (rc != 0) return rc;
    GN_REQUIRE(aligned16(vmax), GOALNET_E_ALIGN, "%s: arenas must be 16-byte aligned", who);
    hipLaunchKernelGGL(group_ranges_kernel, dim3((unsigned)rs.first_block[count]), dim3(256), 0, (hipStream_t)stream, p, g, m, v,
                       ams ? vmax : nullptr, rs, st, count, gt, *opts, step, grad_scale, sumsq, (uint2*)shadow_16, shadow_begin >> 2,
                       shadow_16 ? (shadow_begin + shadow_count) >> 2 : 0, f16, bad_step);
    GN_LAUNCH_CHECK(who);
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
    return launch_sched_lr("group_lr", o, step, lr_out, stream);
}

}  // extern "C"
