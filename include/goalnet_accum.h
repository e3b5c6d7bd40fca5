/*
 * goalnet_accum.h — the sixth public header of libgoalnet_hip.so: gradient accumulation over the sub-batches of a window, so that the
 * fused step applies one optimizer update per k micro-steps (EXTENSION: the reference steps once per sub-batch).
 *
 * Like goalnet_loss.h, goalnet_epoch.h, goalnet_optim.h and goalnet_ema.h this is an addition next to goalnet_hip.h, which stays frozen
 * at GOALNET_ABI_VERSION 7. Conventions are those of goalnet_ema.h: 0 = OK, negative = argument error (GOALNET_E_*), positive =
 * hipError_t of the failed launch, goalnet_last_error() gives the text; raw device pointers; `stream` is a hipStream_t passed as void*;
 * no allocation, no synchronisation, every argument check runs before any launch. `ranges` is a HOST array, copied by value into the
 * kernel arguments: a captured graph bakes it in, as it bakes `scale` and `first`.
 *
 * Ranges: goalnet_adam_range of goalnet_hip.h under its rules — 1 <= count <= GOALNET_ADAM_RANGES_MAX, begin a multiple of 4, sorted,
 * not overlapping; `skipped` is not read.
 *
 * One element, in fp32, each operation rounded on its own (the product is NOT contracted into a fused multiply-add):
 *   first != 0      acc = g * scale                   acc is not read: the first micro-step of a window overwrites it
 *   first == 0      acc = acc + g * scale
 * which is what the two torch operations `t = g * scale; acc = acc + t` compute, bit for bit.
 */
#ifndef GOALNET_ACCUM_H
#define GOALNET_ACCUM_H

#include "goalnet_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

#ifndef GOALNET_E_VALUE
#define GOALNET_E_VALUE (-5) /* argument value out of the supported set (as in goalnet_loss.h) */
#endif

/* The update above over the ranges of the arenas g (read) and acc (written; read too unless `first`) in ONE launch: 16-byte loads and
 * stores, 8 (first) or 12 bytes of traffic per element, nothing outside [begin, begin + count) of any range is written.
 * Refused with GOALNET_E_VALUE: a scale that is not finite or is <= 0, acc == g. */
int goalnet_grad_accum_dev_ranges(float* acc, const float* g, const goalnet_adam_range* ranges, int count, float scale, int first,
                                  void* stream);

#ifdef __cplusplus
}
#endif
#endif /* GOALNET_ACCUM_H */
