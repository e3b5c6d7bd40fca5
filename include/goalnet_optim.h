/*
 * goalnet_optim.h — the fourth public header of libgoalnet_hip.so: optimizer options on the fused step (EXTENSION: the reference
 * runs torch.optim.Adam with its defaults at one learning rate; goalnet_adam_step_dev_ranges of goalnet_hip.h stays that update).
 *
 * Like goalnet_loss.h and goalnet_epoch.h these are additions next to goalnet_hip.h, which stays frozen at GOALNET_ABI_VERSION 7.
 * Conventions are those of goalnet_hip.h: 0 = OK, negative = argument error (GOALNET_E_*), positive = hipError_t of the failed
 * launch, goalnet_last_error() gives the text; raw device pointers and explicit dims; `stream` is a hipStream_t passed as void*; no
 * allocation, no synchronisation, every argument check runs before any launch. `ranges` and `opts` are HOST structures, copied by
 * value into the kernel arguments: a captured graph bakes them in.
 *
 * Ranges: 1 <= count <= GOALNET_ADAM_RANGES_MAX, begin a multiple of 4, sorted, not overlapping — as goalnet_adam_range, plus `decay`.
 *
 * Learning rate of the step that starts from e = *step completed steps (fp64; step t = e + 1 runs at the rate after t - 1 ticks of a
 * torch scheduler):
 *   e < warmup                        lr (e + 1) / warmup                                       (every schedule)
 *   GOALNET_SCHED_CONSTANT            lr
 *   GOALNET_SCHED_COSINE              min_lr + (lr - min_lr) (1 + cos(pi min(e', T) / T)) / 2,   e' = e - warmup, T = total - warmup >= 1
 *   GOALNET_SCHED_STEP                lr gamma^floor(e' / period)
 *
 * Update of one element of a range r, in torch's single-tensor order (fp32 unless noted):
 *   g' = g grad_scale
 *   g' = g' coef                       max_norm > 0:  coef = (float)min(1, max_norm / (grad_scale sqrt(*sumsq) + 1e-6)) in fp64
 *                                      (torch.nn.utils.clip_grad_norm_)
 *   g' = g' + (float)weight_decay p    ranges[r].decay != 0, decoupled == 0      (torch.optim.Adam(weight_decay=))
 *   p  = p (float)(1 - lr_t weight_decay)   ranges[r].decay != 0, decoupled != 0 (torch.optim.AdamW)
 *   Adam on (p, g', m, v) at the rate lr_t under the count t_r = *step + 1 - ranges[r].skipped: the update of goalnet_adam_step_dev_ranges
 * With weight_decay = 0, max_norm <= 0, warmup = 0 and GOALNET_SCHED_CONSTANT the result IS goalnet_adam_step_dev_ranges', bit for bit.
 */
#ifndef GOALNET_OPTIM_H
#define GOALNET_OPTIM_H

#include "goalnet_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

#ifndef GOALNET_E_VALUE
#define GOALNET_E_VALUE (-5) /* argument value out of the supported set (as in goalnet_loss.h) */
#endif

#define GOALNET_SCHED_CONSTANT 0
#define GOALNET_SCHED_COSINE 1
#define GOALNET_SCHED_STEP 2

typedef struct { int64_t begin, count, skipped; int32_t decay, pad; } goalnet_optim_range; /* arena elements; decay != 0: weight decay applies */

typedef struct {
    double lr, beta1, beta2, eps, weight_decay, max_norm /* <= 0: no clipping */, min_lr, gamma;
    int64_t warmup, total, period;
    int32_t decoupled, schedule;
} goalnet_optim_opts;

/* workspace of goalnet_grad_sumsq: one double per block of its first launch; 0 for ranges the entry point refuses */
size_t goalnet_grad_sumsq_ws_bytes(const goalnet_optim_range* ranges, int count);

/* *sumsq = sum of g[i]^2 over the ranges, in fp64 (the square of an fp32 value is exact there). One pass over the ranges with 16-byte
 * loads: every block sums its fixed share and writes one partial to ws (8-byte aligned, at least goalnet_grad_sumsq_ws_bytes); a
 * second one-block launch adds the partials in a fixed order. No atomics: the same data gives the same bits on every run. */
int goalnet_grad_sumsq(const float* g, const goalnet_optim_range* ranges, int count, double* sumsq, void* ws, size_t ws_bytes,
                       void* stream);

/* The update above over the ranges in ONE launch. sumsq: NULL iff opts->max_norm <= 0. shadow_16 (nullable), shadow_begin,
 * shadow_count, f16 and bad_step (nullable) as in goalnet_adam_step_dev_ranges: the 16-bit copy of the updated
 * arena[shadow_begin, shadow_begin + shadow_count), and the guard — *bad_step == *step + 1 returns before anything is touched.
 * Refused with GOALNET_E_VALUE: weight_decay < 0 or not finite, an unknown schedule, warmup < 0, min_lr < 0, cosine with
 * total <= warmup, step with period < 1 or gamma <= 0, sumsq against max_norm. */
int goalnet_optim_step_dev_ranges(float* p, const float* g, float* m, float* v, const goalnet_optim_range* ranges, int count,
                                  const goalnet_optim_opts* opts, const int64_t* step, float grad_scale, const double* sumsq,
                                  void* shadow_16, int64_t shadow_begin, int64_t shadow_count, int f16, const int64_t* bad_step,
                                  void* stream);

/* *lr_out = the learning rate of the step that starts from *step completed steps: the device function the update runs, on one thread */
int goalnet_optim_lr(const goalnet_optim_opts* opts, const int64_t* step, double* lr_out, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* GOALNET_OPTIM_H */
