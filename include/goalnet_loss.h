/*
 * goalnet_loss.h — the second public header of libgoalnet_hip.so: losses for the regression head that can be selected on the
 * fused train step (EXTENSION: the reference has one loss, goalnet_mse_bcast of goalnet_hip.h, which stays the default).
 *
 * Why a second header: goalnet_hip.h is frozen at GOALNET_ABI_VERSION 7 (its entry points, the ctypes table that mirrors it and
 * the contract tests are tied one-to-one). The entry points below are additions that change none of the existing ones; a
 * consumer that needs them includes this header next to goalnet_hip.h and links the same library.
 *
 * Conventions are those of goalnet_hip.h: 0 = OK, negative = argument error (GOALNET_E_*), positive = hipError_t of the failed
 * launch, goalnet_last_error() gives the text; raw fp32 device pointers and explicit dims; `stream` is a hipStream_t passed as
 * void*; no allocation, no synchronisation, every argument check runs before any launch.
 *
 * Arithmetic. p = predictions (n), y = labels (n), w = optional per-frame weights (n), default all ones:
 *   GOALNET_LOSS_MSE        l_i = (p_i - y_i)^2                                   l_i' = 2 (p_i - y_i)
 *   GOALNET_LOSS_L1         l_i = |p_i - y_i|                                     l_i' = sign(p_i - y_i), 0 at 0
 *   GOALNET_LOSS_SMOOTH_L1  d = p_i - y_i, beta = param > 0:
 *                           l_i = |d| < beta ? d^2 / (2 beta) : |d| - beta / 2    l_i' = |d| < beta ? d / beta : sign(d)
 *       loss = 1/n sum_i w_i l_i,  dpred_i = w_i l_i' / n
 *   GOALNET_LOSS_RANK       pairwise logistic (RankNet): S = {(i, j): y_i > y_j}, P = |S|,
 *       loss = 1/P sum_S softplus(-(p_i - p_j)),  softplus(-x) = max(-x, 0) + log1p(exp(-|x|))
 *       dpred_i = 1/P (sum_{j: y_j > y_i} sigmoid(p_i - p_j) - sum_{j: y_i > y_j} sigmoid(p_j - p_i))
 *       Tied pairs contribute nothing. P = 0 (n = 1, all labels equal): loss = 0 and dpred = 0. Takes no weights.
 *   GOALNET_LOSS_MSE_BCAST  goalnet_mse_bcast itself (same code, same bits). Takes no weights.
 * Every sum is accumulated in double and reduced in a fixed order (no floating-point atomics): the same inputs give the same
 * bits on every run, and the stand-alone entry point and the tail of goalnet_mlp_fwd_loss run the same code on the same rows.
 */
#ifndef GOALNET_LOSS_H
#define GOALNET_LOSS_H

#include "goalnet_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

#define GOALNET_E_VALUE (-5) /* argument value out of the supported set (loss kind, beta, weights with a loss that takes none) */

#define GOALNET_LOSS_MSE_BCAST 0
#define GOALNET_LOSS_MSE 1
#define GOALNET_LOSS_L1 2
#define GOALNET_LOSS_SMOOTH_L1 3
#define GOALNET_LOSS_RANK 4

#define GOALNET_FRAME_LOSS_MAX_N 65536

/* workspace of goalnet_frame_loss: 24 n bytes for GOALNET_LOSS_RANK with 1 <= n <= 65536 (per row: the loss partial and the
 * unscaled gradient as doubles, the pair count as int64), 0 for every other kind and for arguments the entry point refuses */
size_t goalnet_frame_loss_ws_bytes(int kind, int n);

/* loss[0] and dpred[n] of `kind` for pred[n] against labels[n]; 1 <= n <= 65536. weights[n] nullable (pointwise kinds only);
 * param = beta of GOALNET_LOSS_SMOOTH_L1 (> 0), ignored by the other kinds. loss and dpred are each nullable, not both.
 * Pointwise kinds and GOALNET_LOSS_MSE_BCAST: one block, no workspace (ws may be NULL). GOALNET_LOSS_RANK: O(n^2), one wave per
 * row i with its lanes striding over j, four rows per block; per-row partials go to ws (16-byte aligned, at least
 * goalnet_frame_loss_ws_bytes), a second one-block launch sums them in a fixed order and scales dpred by 1/P. */
int goalnet_frame_loss(int kind, double param, const float* pred, const float* labels, const float* weights, int n,
                       float* loss, float* dpred, void* ws, size_t ws_bytes, void* stream);

/* goalnet_mlp_fwd (goalnet_hip.h) with a selectable loss in its tail: labels (nullable) -> loss[0], dout[n] of
 * goalnet_frame_loss(loss_kind, loss_param, out, labels, weights) in the same launch — same code, same bits; GOALNET_LOSS_RANK runs
 * inside the one block that holds the <= 16 rows and needs no workspace. With GOALNET_LOSS_MSE_BCAST and no weights this IS
 * goalnet_mlp_fwd. */
int goalnet_mlp_fwd_loss(const float* cat, int64_t ldcat, int K0, const float* const* w, const float* const* b,
                         const float* const* mask, const int64_t* ldmask, float* const* h, float* const* mult,
                         float* logit, float* out, const float* labels, float* loss, float* dout,
                         int loss_kind, double loss_param, const float* weights, int n, int* sync, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* GOALNET_LOSS_H */
