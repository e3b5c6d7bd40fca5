// goalnet_frame_loss (include/goalnet_loss.h): the selectable losses of the regression head as stand-alone launches — what a
// train step of more than 16 frames and VideoTrainer.eval_video run; at <= 16 frames the same code rides in the fused MLP's tail
// (mlp.hip). Pointwise kinds: one block (loss.h). Rank: O(n^2), one wave per row, four rows per block; each row's loss partial,
// unscaled gradient and pair count go to the workspace, and a one-block launch sums them in a fixed order (rank_finish).
#include "common.h"
#include "loss.h"

using namespace goalnet;

namespace {

__global__ __launch_bounds__(256) void frame_loss_kernel(int kind, double param, const float* __restrict__ pred, const float* __restrict__ labels,
                                                         const float* __restrict__ weights, int N, float* __restrict__ loss, float* __restrict__ dpred) {
    if (kind == GOALNET_LOSS_MSE_BCAST) mse_bcast_block(pred, labels, N, loss, dpred);
    else pointwise_loss_block(kind, param, pred, labels, weights, N, loss, dpred);
}

__global__ __launch_bounds__(256) void rank_rows_kernel(const float* __restrict__ pred, const float* __restrict__ labels, int N, int want_loss,
                                                        double* __restrict__ rl, double* __restrict__ rg, long long* __restrict__ rc) {
    const int i = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (i >= N) return;                                 // whole waves leave: rank_row has no block-level barrier
    double l, g;
    int c;
    rank_row(pred, labels, N, i, want_loss != 0, l, g, c);
    if ((threadIdx.x & 63) == 0) { rl[i] = l; rg[i] = g; rc[i] = c; }
}

__global__ __launch_bounds__(256) void rank_finish_kernel(const double* __restrict__ rl, const double* __restrict__ rg, const long long* __restrict__ rc,
                                                          int N, float* __restrict__ loss, float* __restrict__ dpred) {
    rank_finish(rl, rg, rc, N, loss, dpred);
}

}  // namespace

extern "C" {

size_t goalnet_frame_loss_ws_bytes(int kind, int n) {
    return (kind == GOALNET_LOSS_RANK && n >= 1 && n <= GOALNET_FRAME_LOSS_MAX_N) ? (size_t)n * 24 : 0;
}

int goalnet_frame_loss(int kind, double param, const float* pred, const float* labels, const float* weights, int n,
                       float* loss, float* dpred, void* ws, size_t ws_bytes, void* stream) {
    GN_REQUIRE(pred && labels, GOALNET_E_NULL, "frame_loss: null pointer");
    GN_REQUIRE(loss || dpred, GOALNET_E_NULL, "frame_loss: neither a loss nor a dpred destination");
    GN_REQUIRE(n >= 1 && n <= GOALNET_FRAME_LOSS_MAX_N, GOALNET_E_SHAPE, "frame_loss: 1..65536 rows");
    if (const int rc = loss_args_ok("frame_loss", kind, param, weights)) return rc;
    hipStream_t st = (hipStream_t)stream;
    if (kind != GOALNET_LOSS_RANK) {
        hipLaunchKernelGGL(frame_loss_kernel, dim3(1), dim3(256), 0, st, kind, param, pred, labels, weights, n, loss, dpred);
        GN_LAUNCH_CHECK("frame_loss");
        return 0;
    }
    GN_REQUIRE(ws, GOALNET_E_NULL, "frame_loss: the rank loss needs a workspace");
    GN_REQUIRE(aligned16(ws), GOALNET_E_ALIGN, "frame_loss: the workspace must be 16-byte aligned");
    GN_REQUIRE(ws_bytes >= goalnet_frame_loss_ws_bytes(kind, n), GOALNET_E_WORKSPACE, "frame_loss: workspace too small");
    double* rl = (double*)ws;
    double* rg = rl + n;
    long long* rc = (long long*)(rg + n);
    hipLaunchKernelGGL(rank_rows_kernel, dim3((n + 3) / 4), dim3(256), 0, st, pred, labels, n, loss ? 1 : 0, rl, rg, rc);
    GN_LAUNCH_CHECK("frame_loss (rank rows)");
    hipLaunchKernelGGL(rank_finish_kernel, dim3(1), dim3(256), 0, st, rl, rg, rc, n, loss, dpred);
    GN_LAUNCH_CHECK("frame_loss (rank finish)");
    return 0;
}

}  // extern "C"
