// Rank correlation of importance vectors with annotator scores, on the device: Kendall's tau-b and Spearman's rho with ties, for
// every (prediction row b, annotator a) pair of one video in one call. EXTENSION, PARITY UNPINNED (no reference code): the
// reference reports the knapsack F-score only; the oracle is scipy.stats.kendalltau (variant b) / spearmanr through fixtures and
// the project's numpy restatement (tests/rankcorr_ref.py). Everything up to the last two divisions is exact
// integer arithmetic, so the results do not depend on the grid, the tile or the order in which blocks arrive.
//
//   pairs      grid (ceil(n / 256), A, B): thread i walks every j, x_b and y_a staged in LDS 1024 elements at a time (all lanes read
//              one address: a broadcast). It counts #less / #equal of x and of y (the rank of i), #equal in both and
//              sum_j sgn(x_i - x_j) sgn(y_i - y_j) over the FULL square, which holds every unordered pair twice; then
//              d = 2 #less + #equal - n (twice the average rank minus n + 1: an integer with mean zero) gives dx dy, dx^2, dy^2.
//              Eight int64 sums are reduced over the wavefront (shuffles), over the block (LDS) and leave as ONE integer atomicAdd
//              per count and block: integer adds commute, the result is reproducible.
//   finalize   one block per b: halves the doubled pair counts in place, forms tau and rho in float64, and one thread sums the defined
//              ones in annotator order.
// Comparisons are IEEE < and == on the float32 values (-0.0 ties with 0.0; a NaN is less than, greater than and equal to nothing,
// itself included), which is also how the padding works: slots past n and threads past n hold NaN and add nothing.
#include "common.h"

#include <cmath>

using namespace goalnet;

namespace {

constexpr int RC_THREADS = 256;       // i-tile: one i per thread
constexpr int RC_TILE = 1024;         // j-tile staged in LDS
constexpr int RC_MAX_N = 65536;       // |sum d d| <= n^3 < 2^63, per-thread counters < 2^31
constexpr int RC_MAX_A = 128;         // the limit of goalnet_mean_annotations
constexpr int RC_MAX_B = 65535;       // gridDim.z, as goalnet_postprocess_batch
constexpr int RC_COUNTS = 8;          // S, tx, ty, txy, cxy, cxx, cyy, bad

__global__ __launch_bounds__(RC_THREADS) void rankcorr_pairs_kernel(const float* __restrict__ x, int64_t ldx, int x_repeat,
                                                                    const float* __restrict__ y, int64_t ldy, int y_stride,
                                                                    int n_annotators, int n, int64_t* __restrict__ counts) {
    __shared__ __attribute__((aligned(16))) float xs[RC_TILE];
    __shared__ __attribute__((aligned(16))) float ys[RC_TILE];
    __shared__ long long red[RC_THREADS / 64][RC_COUNTS];
    const int b = blockIdx.z, a = blockIdx.y;
    const float* xr = x + (size_t)b * (size_t)ldx;
    const float* yr = y + (size_t)a * (size_t)ldy;
    const int i = blockIdx.x * RC_THREADS + threadIdx.x;
    const bool live = i < n;
    const float xi = live ? xr[i / x_repeat] : NAN;
    const float yi = live ? yr[(int64_t)i * y_stride] : NAN;
    int ltx = 0, eqx = 0, lty = 0, eqy = 0, eqxy = 0, s = 0;
    for (int j0 = 0; j0 < n; j0 += RC_TILE) {
        const int cnt = min(RC_TILE, n - j0);
        const int cnt4 = (cnt + 3) & ~3;                            // <= RC_TILE: the tile is a multiple of 4
        __syncthreads();                                            // the previous tile has been read
        for (int t = threadIdx.x; t < cnt4; t += RC_THREADS) {
            const int j = j0 + t;                                   // j < n where t < cnt
            xs[t] = t < cnt ? xr[j / x_repeat] : NAN;
            ys[t] = t < cnt ? yr[(int64_t)j * y_stride] : NAN;
        }
        __syncthreads();
        for (int t = 0; t < cnt4; t += 4) {
            const float4 xv = *reinterpret_cast<const float4*>(&xs[t]);
            const float4 yv = *reinterpret_cast<const float4*>(&ys[t]);
            const float xj[4] = {xv.x, xv.y, xv.z, xv.w}, yj[4] = {yv.x, yv.y, yv.z, yv.w};
#pragma unroll
            for (int u = 0; u < 4; ++u) {
                const int lx = xj[u] < xi, gx = xi < xj[u], ex = xj[u] == xi;
                const int ly = yj[u] < yi, gy = yi < yj[u], ey = yj[u] == yi;
                ltx += lx;
                eqx += ex;
                lty += ly;
                eqy += ey;
                eqxy += ex & ey;
                s += (lx - gx) * (ly - gy);
            }
        }
    }
    // a thread past n holds NaN: every counter is zero, its own "equal to itself" included
    const int selfx = xi == xi, selfy = yi == yi;
    const long long dx = live ? 2LL * ltx + eqx - n : 0, dy = live ? 2LL * lty + eqy - n : 0;
    long long v[RC_COUNTS];
    v[0] = s;                                                       // 2 S
    v[1] = eqx - selfx;                                             // 2 tx: the j != i that tie with i
    v[2] = eqy - selfy;
    v[3] = eqxy - (selfx & selfy);
    v[4] = dx * dy;
    v[5] = dx * dx;
    v[6] = dy * dy;
    v[7] = live && !(isfinite(xi) && isfinite(yi));
#pragma unroll
    for (int c = 0; c < RC_COUNTS; ++c) {
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) v[c] += __shfl_xor(v[c], o, 64);
    }
    if ((threadIdx.x & 63) == 0) {
#pragma unroll
        for (int c = 0; c < RC_COUNTS; ++c) red[threadIdx.x >> 6][c] = v[c];
    }
    __syncthreads();
    if (threadIdx.x < RC_COUNTS) {
        const int c = threadIdx.x;
        const long long total = (red[0][c] + red[1][c]) + (red[2][c] + red[3][c]);
        // two's complement: adding the bit pattern of a negative total is the signed add
        atomicAdd(reinterpret_cast<unsigned long long*>(counts + ((size_t)b * n_annotators + a) * RC_COUNTS + c), (unsigned long long)total);
    }
}

__global__ __launch_bounds__(RC_MAX_A) void rankcorr_finalize_kernel(int64_t* __restrict__ counts, int n_annotators, int n,
                                                                     double* __restrict__ tau, double* __restrict__ rho,
                                                                     double* __restrict__ mean, int32_t* __restrict__ n_valid,
                                                                     int32_t* __restrict__ status) {
    __shared__ double st[RC_MAX_A], sr[RC_MAX_A];
    __shared__ int sbad[RC_MAX_A];
    const int b = blockIdx.x, a = threadIdx.x;
    if (a < n_annotators) {
        int64_t* c = counts + ((size_t)b * n_annotators + a) * RC_COUNTS;
        const int64_t S = c[0] / 2, tx = c[1] / 2, ty = c[2] / 2, txy = c[3] / 2;        // the full square holds every pair twice: even
        const int64_t cxy = c[4], cxx = c[5], cyy = c[6], bad = c[7];
        c[0] = S;
        c[1] = tx;
        c[2] = ty;
        c[3] = txy;
        const int64_t n0 = (int64_t)n * (n - 1) / 2;
        double t = NAN, r = NAN;
        if (n >= 2 && n0 != tx && n0 != ty && bad == 0) t = (double)S / sqrt((double)(n0 - tx) * (double)(n0 - ty));
        if (cxx != 0 && cyy != 0 && bad == 0) r = (double)cxy / sqrt((double)cxx * (double)cyy);
        tau[(size_t)b * n_annotators + a] = t;
        rho[(size_t)b * n_annotators + a] = r;
        st[a] = t;
        sr[a] = r;
        sbad[a] = bad > 0;
    }
    __syncthreads();
    if (a != 0) return;
    double sum_t = 0.0, sum_r = 0.0;
    int nt = 0, nr = 0, any_bad = 0;
    for (int k = 0; k < n_annotators; ++k) {                        // annotator order
        if (st[k] == st[k]) { sum_t += st[k]; ++nt; }
        if (sr[k] == sr[k]) { sum_r += sr[k]; ++nr; }
        any_bad |= sbad[k];
    }
    mean[2 * (size_t)b] = nt ? sum_t / (double)nt : NAN;
    mean[2 * (size_t)b + 1] = nr ? sum_r / (double)nr : NAN;
    n_valid[2 * (size_t)b] = nt;
    n_valid[2 * (size_t)b + 1] = nr;
    status[b] = any_bad;
}

bool aligned8(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 7u) == 0; }

}  // namespace

extern "C" {

int goalnet_rank_corr(const float* x, int64_t ldx, int x_repeat, const float* y, int64_t ldy, int y_stride, int batch, int n_annotators,
                      int n, int64_t* counts, double* tau, double* rho, double* mean, int32_t* n_valid, int32_t* status, void* stream) {
    GN_REQUIRE(x && y && counts && tau && rho && mean && n_valid && status, GOALNET_E_NULL, "rank_corr: null pointer");
    GN_REQUIRE(n >= 1 && n <= RC_MAX_N, GOALNET_E_SHAPE, "rank_corr: need 1 <= n <= %d", RC_MAX_N);
    GN_REQUIRE(n_annotators >= 1 && n_annotators <= RC_MAX_A, GOALNET_E_SHAPE, "rank_corr: need 1 <= n_annotators <= %d", RC_MAX_A);
    GN_REQUIRE(batch >= 1 && batch <= RC_MAX_B, GOALNET_E_SHAPE, "rank_corr: need 1 <= batch <= %d", RC_MAX_B);
    GN_REQUIRE(x_repeat >= 1 && y_stride >= 1, GOALNET_E_SHAPE, "rank_corr: x_repeat and y_stride must be positive");
    GN_REQUIRE(ldx >= ((int64_t)n + x_repeat - 1) / x_repeat, GOALNET_E_SHAPE, "rank_corr: ldx must be at least ceil(n / x_repeat)");
    GN_REQUIRE(ldy >= (int64_t)(n - 1) * y_stride + 1, GOALNET_E_SHAPE, "rank_corr: ldy must be at least (n - 1) y_stride + 1");
    GN_REQUIRE(aligned8(counts) && aligned8(tau) && aligned8(rho) && aligned8(mean), GOALNET_E_ALIGN,
               "rank_corr: counts, tau, rho and mean must be 8-byte aligned");
    hipStream_t st = (hipStream_t)stream;
    hipError_t e = hipMemsetAsync(counts, 0, (size_t)batch * n_annotators * RC_COUNTS * sizeof(int64_t), st);
    if (e != hipSuccess) {
        set_error("rank_corr: hipMemsetAsync failed: %s", hipGetErrorString(e));
        return (int)e;
    }
    hipLaunchKernelGGL(rankcorr_pairs_kernel, dim3((n + RC_THREADS - 1) / RC_THREADS, n_annotators, batch), dim3(RC_THREADS), 0, st, x, ldx,
                       x_repeat, y, ldy, y_stride, n_annotators, n, counts);
    GN_LAUNCH_CHECK("rank_corr.pairs");
    hipLaunchKernelGGL(rankcorr_finalize_kernel, dim3(batch), dim3(RC_MAX_A), 0, st, counts, n_annotators, n, tau, rho, mean, n_valid,
                       status);
    GN_LAUNCH_CHECK("rank_corr.finalize");
    return 0;
}

}  // extern "C"
