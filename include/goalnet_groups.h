/*
 * goalnet_groups.h — the seventh public header of libgoalnet_hip.so: parameter groups and AMSGrad on the fused step (EXTENSION,
 * torch.optim.Adam / AdamW with several param_groups and amsgrad=True; the reference runs one group without it).
 *
 * Additions next to goalnet_optim.h, which stays byte for byte as it is; goalnet_hip.h stays frozen at GOALNET_ABI_VERSION 7.
 * Conventions are those of goalnet_optim.h: 0 = OK, negative = argument error (GOALNET_E_*), positive = hipError_t of the failed
 * launch, goalnet_last_error() gives the text; raw device pointers; `stream` is a hipStream_t passed as void*; no allocation, no
 * synchronisation, every argument check runs before any launch. `ranges`, `groups` and `opts` are HOST structures, copied by value
 * into the kernel arguments: a captured graph bakes them in.
 *
 * Ranges: 1 <= count <= GOALNET_ADAM_RANGES_MAX, begin a multiple of 4, sorted, not overlapping — as goalnet_optim_range, plus
 * `group`, an index into the table of 1 <= ngroups <= GOALNET_GROUPS_MAX hyper-parameter sets. Group 0 is the default group.
 *
 * Schedule, clipping and `decoupled` come from a goalnet_optim_opts; its lr, beta1, beta2, eps and weight_decay are not read (they
 * must still be values goalnet_optim_step_dev_ranges accepts). The rate of group k at e = *step completed steps is
 *   lr_t(k) = the schedule of goalnet_optim.h evaluated with lr := groups[k].lr
 * which is what torch's schedulers do to param_groups: every group is scaled by the same factor, min_lr is global.
 *
 * Update of one element of a range r with k = ranges[r].group, in torch's single-tensor order (fp32 unless noted):
 *   g' = g grad_scale
 *   g' = g' coef                       max_norm > 0: the GLOBAL clip coefficient of goalnet_optim.h, from *sumsq
 *   g' = g' + (float)wd_k p            ranges[r].decay != 0 and wd_k > 0, decoupled == 0
 *   p  = p (float)(1 - lr_t(k) wd_k)   ranges[r].decay != 0 and wd_k > 0, decoupled != 0
 *   m, v as Adam's under beta1_k, beta2_k and the count t_r = *step + 1 - ranges[r].skipped
 *   amsgrad_k == 0:  the update of goalnet_optim_step_dev_ranges. A range whose group carries that call's lr, betas, eps and
 *                    weight_decay gives its bits.
 *   amsgrad_k != 0:  vmax = max(vmax, v), a NaN on either side stays (torch.maximum);
 *                    p -= step_size (m / (sqrtf(vmax) / bc2_sqrt + eps))           (torch's _single_tensor_adam(amsgrad=True))
 * Traffic per parameter: 28 B without AMSGrad (p, m, v read and written, g read), 36 B with it.
 */
#ifndef GOALNET_GROUPS_H
#define GOALNET_GROUPS_H

#include "goalnet_optim.h"

#ifdef __cplusplus
extern "C" {
#endif

#define GOALNET_GROUPS_MAX 8

typedef struct { double lr, beta1, beta2, eps, weight_decay; int32_t amsgrad, pad; } goalnet_group_hyper;

typedef struct { int64_t begin, count, skipped; int32_t decay, group; } goalnet_group_range; /* arena elements; group: index into the table */

/* The update above over the ranges in ONE launch. vmax: the running maximum of v, laid out like v; it may be NULL iff no range's
 * group has amsgrad, and is neither read nor written then. sumsq, shadow_16, shadow_begin, shadow_count, f16 and bad_step as in
 * goalnet_optim_step_dev_ranges: *bad_step == *step + 1 returns before anything is touched, vmax included.
 * Refused before any launch, beyond everything goalnet_optim_step_dev_ranges refuses: ngroups outside 1..GOALNET_GROUPS_MAX and a
 * range's group outside 0..ngroups-1 (GOALNET_E_SHAPE); a group with lr < 0, a beta outside [0, 1), eps < 0, weight_decay < 0 or a
 * value that is not finite, vmax == NULL while a referenced group has amsgrad (GOALNET_E_VALUE). */
int goalnet_group_step_dev_ranges(float* p, const float* g, float* m, float* v, float* vmax, const goalnet_group_range* ranges, int count,
                                  const goalnet_group_hyper* groups, int ngroups, const goalnet_optim_opts* opts, const int64_t* step,
                                  float grad_scale, const double* sumsq, void* shadow_16, int64_t shadow_begin, int64_t shadow_count,
                                  int f16, const int64_t* bad_step, void* stream);

/* *lr_out = lr_t(g) of the step that starts from *step completed steps, for groups[g] with 0 <= g < GOALNET_GROUPS_MAX (the caller's
 * table has at least g + 1 entries): the device function the update runs, on one thread — as goalnet_optim_lr for the single rate */
int goalnet_group_lr(const goalnet_optim_opts* opts, const goalnet_group_hyper* groups, int g, const int64_t* step, double* lr_out,
                     void* stream);

#ifdef __cplusplus
}
#endif
#endif /* GOALNET_GROUPS_H */
