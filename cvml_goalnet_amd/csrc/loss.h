// The selectable losses of the regression head (include/goalnet_loss.h; EXTENSION) as the work of ONE block of
// 256 threads, next to mse_bcast_block (mse.h): goalnet_frame_loss's kernels (loss.hip) and the tail of the fused fusion-MLP
// forward (mlp.hip) run the same code, so the loss and dL/dpred do not depend on which of the two produced them.
//   pointwise kinds: loss = 1/n sum_i w_i l_i, dpred_i = w_i l_i' / n — one strided pass, doubles, summed wave -> block in a fixed order
//   rank: rank_row is the work of ONE wave for one row i (lanes stride over j), rank_finish sums the rows' partials in a fixed
//         order, produces loss and P and scales the gradient by 1/P. frame_loss_block runs both inside the block (<= 16 rows: the
//         MLP tail); loss.hip tiles rank_row over blocks with the partials in a lent workspace and runs rank_finish in a second launch.
// No floating-point atomics anywhere. Contraction is switched off in the arithmetic so that two instantiations cannot differ by an fma.
#pragma once
#include <math.h>

#include "../../include/goalnet_loss.h"
#include "common.h"
#include "mse.h"

namespace goalnet {

constexpr int RANK_BLOCK_ROWS = 16;       // rows frame_loss_block's in-block rank serves (the fused MLP's limit)

// host: the argument rules every entry point with a loss shares (goalnet_loss.h). 0 or a negative code with the error text set.
static inline int loss_args_ok(const char* who, int kind, double param, const float* weights) {
    GN_REQUIRE(kind >= GOALNET_LOSS_MSE_BCAST && kind <= GOALNET_LOSS_RANK, GOALNET_E_VALUE, "%s: unknown loss kind %d", who, kind);
    GN_REQUIRE(kind != GOALNET_LOSS_SMOOTH_L1 || param > 0.0, GOALNET_E_VALUE, "%s: smooth_l1 needs beta > 0", who);      // refuses NaN too
    GN_REQUIRE(!weights || (kind != GOALNET_LOSS_RANK && kind != GOALNET_LOSS_MSE_BCAST), GOALNET_E_VALUE,
               "%s: the rank and the broadcast loss take no weights", who);
    return 0;
}

// the block's sum of `mine` in a fixed order (lanes by xor-shuffles, then waves 0..3); every thread gets it. red: 4 doubles of LDS
__device__ __forceinline__ double block_sum_d(double mine, double* red) {
    mine = wave_sum_d(mine);
    __syncthreads();                                   // an earlier sum through `red` has been read
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = mine;
    __syncthreads();
    return ((red[0] + red[1]) + red[2]) + red[3];
}

__device__ __forceinline__ void pointwise_loss_block(int kind, double beta, const float* __restrict__ pred, const float* __restrict__ labels,
                                                     const float* __restrict__ weights, int N, float* __restrict__ loss, float* __restrict__ dpred) {
#pragma clang fp contract(off)
    __shared__ double red[4];
    const double n = (double)N;
    double s = 0.0;
    for (int i = threadIdx.x; i < N; i += 256) {
        const double d = (double)pred[i] - (double)labels[i];
        const double w = weights ? (double)weights[i] : 1.0;
        const double a = fabs(d), sg = d > 0.0 ? 1.0 : d < 0.0 ? -1.0 : 0.0;
        double l, dl;
        if (kind == GOALNET_LOSS_MSE) { l = d * d; dl = 2.0 * d; }
        else if (kind == GOALNET_LOSS_L1) { l = a; dl = sg; }
        else if (a < beta) { l = 0.5 * d * d / beta; dl = d / beta; }
        else { l = a - 0.5 * beta; dl = sg; }
        s += w * l;
        if (dpred) dpred[i] = (float)(w * dl / n);
    }
    s = block_sum_d(s, red);
    if (loss && threadIdx.x == 0) loss[0] = (float)(s / n);
}

// ONE wave: row i of the pairwise logistic loss. With x = p_i - p_j and e = exp(-|x|):
//   y_i > y_j, the pair (i, j): softplus(-x) = max(-x, 0) + log1p(e) joins the loss, -sigmoid(-x) the gradient of p_i
//   y_j > y_i, the pair (j, i): its margin is -x, +sigmoid(x) joins the gradient of p_i
// Every lane returns l = the row's loss partial (0 unless want_loss), g = its UNSCALED gradient, c = its pair count.
__device__ __forceinline__ void rank_row(const float* __restrict__ pred, const float* __restrict__ labels, int N, int i, bool want_loss,
                                         double& l, double& g, int& c) {
#pragma clang fp contract(off)
    const double pi = (double)pred[i];
    const float yi = labels[i];
    double ls = 0.0, gs = 0.0;
    int cnt = 0;
    for (int j = threadIdx.x & 63; j < N; j += 64) {
        const float yj = labels[j];
        const bool hi = yi > yj, lo = yj > yi;
        if (!hi && !lo) continue;                       // a tie (or a NaN label): no pair
        const double x = pi - (double)pred[j];
        const double e = exp(-fabs(x));
        const double big = 1.0 / (1.0 + e), small = e / (1.0 + e);      // sigmoid(|x|), sigmoid(-|x|)
        if (hi) {
            ++cnt;
            if (want_loss) ls += fmax(-x, 0.0) + log1p(e);
            gs -= x >= 0.0 ? small : big;
        } else {
            gs += x >= 0.0 ? big : small;
        }
    }
    l = wave_sum_d(ls);
    g = wave_sum_d(gs);
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) cnt += __shfl_xor(cnt, o, 64);
    c = cnt;
}

// ONE block: the rows' partials rl / rg / rc (N each; LDS or a workspace) -> loss = sum rl / P, dpred_i = rg_i / P, P = sum rc
__device__ __forceinline__ void rank_finish(const double* rl, const double* rg, const long long* rc, int N, float* __restrict__ loss,
                                            float* __restrict__ dpred) {
#pragma clang fp contract(off)
    __shared__ double red[4];
    __shared__ long long redc[4];
    double s = 0.0;
    long long c = 0;
    for (int i = threadIdx.x; i < N; i += 256) { s += rl[i]; c += rc[i]; }
    s = block_sum_d(s, red);
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) c += __shfl_xor(c, o, 64);
    if ((threadIdx.x & 63) == 0) redc[threadIdx.x >> 6] = c;
    __syncthreads();
    const long long P = redc[0] + redc[1] + redc[2] + redc[3];
    if (loss && threadIdx.x == 0) loss[0] = P > 0 ? (float)(s / (double)P) : 0.f;
    if (dpred)
        for (int i = threadIdx.x; i < N; i += 256) dpred[i] = P > 0 ? (float)(rg[i] / (double)P) : 0.f;
}

// ONE block of 256 threads: any kind for the N rows it sees (rank: N <= RANK_BLOCK_ROWS). loss / dpred nullable.
__device__ __forceinline__ void frame_loss_block(int kind, double param, const float* __restrict__ pred, const float* __restrict__ labels,
                                                 const float* __restrict__ weights, int N, float* __restrict__ loss, float* __restrict__ dpred) {
    if (kind == GOALNET_LOSS_MSE_BCAST) {
        mse_bcast_block(pred, labels, N, loss, dpred);
    } else if (kind != GOALNET_LOSS_RANK) {
        pointwise_loss_block(kind, param, pred, labels, weights, N, loss, dpred);
    } else {
        __shared__ double rl[RANK_BLOCK_ROWS], rg[RANK_BLOCK_ROWS];
        __shared__ long long rc[RANK_BLOCK_ROWS];
        for (int i = threadIdx.x >> 6; i < N && i < RANK_BLOCK_ROWS; i += 4) {
            double l, g;
            int c;
            rank_row(pred, labels, N, i, loss != nullptr, l, g, c);
            if ((threadIdx.x & 63) == 0) { rl[i] = l; rg[i] = g; rc[i] = c; }
        }
        __syncthreads();
        rank_finish(rl, rg, rc, N < RANK_BLOCK_ROWS ? N : RANK_BLOCK_ROWS, loss, dpred);
    }
}

}  // namespace goalnet
