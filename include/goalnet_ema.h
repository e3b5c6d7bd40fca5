/*
 * goalnet_ema.h — the fifth public header of libgoalnet_hip.so: an exponential moving average of the weights that follows the fused
 * step on the device, and the exchange of two arenas (EXTENSION: the reference evaluates and saves its last iterate).
 *
 * Like goalnet_loss.h, goalnet_epoch.h and goalnet_optim.h these are additions next to goalnet_hip.h, which stays frozen at
 * GOALNET_ABI_VERSION 7. Conventions are those of goalnet_optim.h: 0 = OK, negative = argument error (GOALNET_E_*), positive =
 * hipError_t of the failed launch, goalnet_last_error() gives the text; raw device pointers; `stream` is a hipStream_t passed as void*;
 * no allocation, no synchronisation, every argument check runs before any launch. `ranges` and `opts` are HOST structures, copied by
 * value into the kernel arguments: a captured graph bakes them in.
 *
 * Ranges: goalnet_adam_range of goalnet_hip.h under its rules — 1 <= count <= GOALNET_ADAM_RANGES_MAX, begin a multiple of 4, sorted,
 * not overlapping; `skipped` is not read (the average has one count, the global one).
 *
 * The update of one element, with t = *step + step_bias, the 1-based optimizer step that has just been applied:
 *   bad_step != NULL and *bad_step == t     nothing is touched (an fp16 step whose Adam was skipped does not move the average)
 *   t <= start_step                         e = p, bit for bit                      (the average tracks the weights)
 *   u = t - start_step, u % every != 0      nothing is written
 *   otherwise                               k = u / every - 1                        (averaging updates before this one)
 *                                           d = warmup ? min(decay, (1 + k) / (10 + k)) : decay            in fp64
 *                                           w = (float)(1 - d)
 *                                           e = fma(w, p - e, e)                     in fp32 (torch.lerp's form for a weight < 1/2)
 * The decision and w are uniform over the grid: every thread evaluates them from the device counter, so a replayed graph walks t.
 */
#ifndef GOALNET_EMA_H
#define GOALNET_EMA_H

#include "goalnet_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

#ifndef GOALNET_E_VALUE
#define GOALNET_E_VALUE (-5) /* argument value out of the supported set (as in goalnet_loss.h) */
#endif

typedef struct { double decay; int64_t every, start_step; int32_t warmup, pad; } goalnet_ema_opts;

/* The update above over the ranges of the arenas p (read) and e (read, written) in ONE launch: 16-byte loads and stores, 12 bytes of
 * traffic per element, nothing outside [begin, begin + count) of any range is written. bad_step is nullable.
 * Refused with GOALNET_E_VALUE: decay outside [0, 1) or not finite, every < 1, start_step < 0. */
int goalnet_ema_update_dev_ranges(const float* p, float* e, const goalnet_adam_range* ranges, int count, const goalnet_ema_opts* opts,
                                  const int64_t* step, int64_t step_bias, const int64_t* bad_step, void* stream);

/* a[i] <-> b[i] over the ranges, exactly (the bits travel as integers), in ONE launch; twice is the identity. a and b must not overlap. */
int goalnet_swap_ranges(float* a, float* b, const goalnet_adam_range* ranges, int count, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* GOALNET_EMA_H */
