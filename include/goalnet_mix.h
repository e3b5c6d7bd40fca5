/*
 * goalnet_mix.h — the eighth public header of libgoalnet_hip.so: audio augmentation and mixup for a shuffled, augmented pass over a
 * video that is resident on the device (EXTENSION of goalnet_epoch.h's pass; there is no reference code).
 *
 * Additions next to goalnet_hip.h, which stays frozen at GOALNET_ABI_VERSION 7; the older headers do not gain these names.
 * Conventions are those of goalnet_epoch.h: 0 = OK, negative = argument error (GOALNET_E_*), positive = hipError_t of the failed
 * launch, goalnet_last_error() gives the text; raw device pointers and explicit dims; `stream` is a hipStream_t passed as void*; no
 * allocation, no synchronisation, every argument check runs before any launch.
 *
 * The second plan table of a pass over n frames is n rows of GOALNET_PLAN2_WORDS 32-bit words (48 bytes per row, 16-byte aligned).
 * Row i belongs to row i of the plan (goalnet_epoch.h) and describes the i-th frame the pass consumes:
 *     { a_shift, t0, tw, c0, cw, gain, partner, lambda, nkey lo, nkey hi, 0, 0 }      gain, lambda: the bits of an fp32
 * Draws (csrc/rng.h; host twin cvml_goalnet_amd/synth.py), option k of pass `index`:
 *     key_k     = stream_key(seed, GOALNET_TID_PLAN2 + 16 * index + k)
 *     bits_k(r) = element r of that stream, r = plan[i].src, the SOURCE frame
 *     u24(r)    = bits_k(r) >> 40,  u(r) = float(u24) * 2^-24
 *   k = 0  a_shift   ((u24 * (2 S + 1)) >> 24) - S,  S = max_shift                       (integers only)
 *   k = 1  tw        (u24 * (T + 1)) >> 24,  T = time_mask                                in [0, T]
 *   k = 2  t0        (u24 * (B - tw + 1)) >> 24                                           t0 + tw <= B
 *   k = 3  cw        (u24 * (M + 1)) >> 24,  M = coeff_mask <= C - 1
 *   k = 4  c0        1 + ((u24 * (C - cw)) >> 24)                                         1 <= c0, c0 + cw <= C
 *   k = 5  gain      lo + fmaf(span, u, 0),  lo = 1 - g, span = (1 + g) - lo              (each one fp32 operation)
 *   k = 6  nkey      the 64 bits of element r; all zero when noise = 0
 *   k = 7  partner   q = (u24 * n) >> 24, a POSITION in this plan
 *   k = 8  lambda    lo + fmaf(span, u, 0),  lo = 1 - strength, span = 1 - lo
 *   k = 9  apply     u < p                                                                 (fp32 compare)
 * A frame is mixed when mixup is on (strength > 0 and p > 0), `apply` holds, q != i and the drawn lambda is not exactly 1.0f; the row
 * then holds {q, lambda}. Every other row holds partner = i and lambda = 1.0f: a row is mixed if and only if its lambda bits differ
 * from 1.0f's. An option that is switched off writes its identity: 0 for the integers (t0 and c0 included), 1.0f for the gain.
 *
 * Mixing a row i with partner position q, mu = 1.0f - lambda (one fp32 subtraction):
 *     out = fmaf(A, lambda, 0) + fmaf(Bv, mu, 0)           two rounded products, one rounded sum, no fusion across them
 * A is row i's fully augmented value, Bv row q's fully augmented, UNMIXED value read through plan[q] and plan2[q] (its own flip,
 * shift, colour and audio draws; no recursion). An unmixed row is a bitwise copy of A and its partner word is not consulted.
 * A row is left unwritten, and nothing is dereferenced through it, when its plan index, or a mixed row's partner, lies outside
 * [0, plan_rows), or when either src lies outside the table. Both plans hold at least plan_rows rows.
 */
#ifndef GOALNET_MIX_H
#define GOALNET_MIX_H

#include "goalnet_epoch.h"

#ifdef __cplusplus
extern "C" {
#endif

#define GOALNET_TID_PLAN2 3221225472 /* 3 * 2^30, above every GOALNET_TID_PLAN + 8 * index + k; synth.TID_PLAN2; index < 2^26 */
#define GOALNET_PLAN2_WORDS 12
#define GOALNET_PLAN2_MAX_INDEX 67108864 /* 2^26 */

/* launch-level flags of goalnet_audio_gather_aug */
#define GOALNET_AUDIO_GAIN 1
#define GOALNET_AUDIO_NOISE 2
#define GOALNET_AUDIO_MIX 4

/* plan2[n][12] of pass `index` from the finished plan[n][8] of the same pass (only its src column is read); the audio table the
 * pass will be applied to is (rows, C, B). 1 <= n <= GOALNET_EPOCH_MAX_N, C >= 1, B >= 1, 0 <= max_shift <= GOALNET_MAX_SHIFT,
 * 0 <= time_mask <= B, 0 <= coeff_mask <= C - 1, 0 <= gain < 1, 0 <= noise (finite), 0 <= strength <= 1, 0 <= p <= 1,
 * index < 2^26. One thread per row, integer and single fp32 operations only: the same bits for any launch geometry. One launch. */
int goalnet_epoch_plan2(int32_t* plan2, const int32_t* plan, int n, uint64_t seed, uint32_t index, int C, int B, int max_shift,
                        int time_mask, int coeff_mask, float gain, float noise, float strength, float p, void* stream);

/* out[i, c, t] of the (nrows, C, B) block from the (table_rows, C, B) fp32 table, rows plan / plan2[*cursor + cursor_bias + i]:
 *   1. v = table[src, c, clamp(t - a_shift, 0, B - 1)]                                   (edge-replicate)
 *   2. flags & GOALNET_AUDIO_GAIN:   v = fmaf(v, gain, 0)
 *   3. flags & GOALNET_AUDIO_NOISE:  v = v + nz,  nz = lo + fmaf(span, u_e, 0),  lo = -noise, span = noise - lo,
 *                                    u_e = float(mix64(nkey + (e + 1) * GAMMA) >> 40) * 2^-24,  e = c * B + t
 *   4. c >= 1 and (t0 <= t < t0 + tw or c0 <= c < c0 + cw):  v = +0.0                    (coefficient 0 is never masked)
 *   5. flags & GOALNET_AUDIO_MIX and the row is mixed: the mix above with the partner's steps 1-4
 * With no flag set, values are moved as 32-bit words. `noise` is a launch constant (>= 0, finite); the per-frame key lives in the
 * row, so one captured launch serves every pass. C * B < 2^31. One launch. */
int goalnet_audio_gather_aug(const float* table, int64_t table_rows, float* out, const int32_t* plan, const int32_t* plan2,
                             int plan_rows, int C, int B, int nrows, const int64_t* cursor, int64_t cursor_bias, int flags,
                             float noise, void* stream);

/* goalnet_frames_gather_aug (goalnet_epoch.h) plus plan2 and the mix: both rows go through flip, shift and — with the same
 * launch-level `colour` flag — gain / bias / clamp before they are mixed. One launch. */
int goalnet_frames_gather_mix(const float* table, int64_t table_rows, float* out, const int32_t* plan, const int32_t* plan2,
                              int plan_rows, int C, int H, int W, int nrows, const int64_t* cursor, int64_t cursor_bias, int colour,
                              void* stream);

/* fp32 row tables through the plan with the mix, up to GOALNET_ROWCOPY_MAX segments in one launch (labels, loss weights):
 *     dst[i, w] = mix(table[plan[c + i].src, w], table[plan[q].src, w]),   c = *cursor + cursor_bias,   i < nrows, w < row_elems */
typedef struct {
    const float* table; float* dst; int64_t row_elems; int nrows; const int64_t* cursor; int64_t cursor_bias; int64_t table_rows;
} goalnet_rowmix;
int goalnet_rows_mix_indexed(const goalnet_rowmix* segs, int count, const int32_t* plan, const int32_t* plan2, int plan_rows,
                             void* stream);

#ifdef __cplusplus
}
#endif
#endif /* GOALNET_MIX_H */
