// Kernel Temporal Segmentation (Potapov et al., ECCV 2014) with the linear kernel, on the device: the change points that
// SummaryEvaluator / VideoSummarizer otherwise take from the dataset's HDF5 file. EXTENSION, PARITY UNPINNED (no reference code):
// the reference holds no segmentation code, the oracle is the project's own restatement of the published algorithm
// (tests/kts_ref.py). All arithmetic is float64 on the float32 descriptors converted exactly.
//
//   rowsq     one block per row: ||x_i||, and ||x_i / ||x_i|| ||^2 (or ||x_i||^2 without normalisation), fixed tree
//   prefix    one thread per descriptor column walks the n rows in order: S[i+1] = S[i] + x_i; one more thread scans D the same way
//   scatter   Jt[l-1][t] = J(t, l-1) = (D[l] - D[t]) - ||S[l] - S[t]||^2 / (l - t): a float64 distance-matrix GEMM, 64 x 64 tiles,
//             S staged in LDS; the difference of the prefix sums is taken first and squared after (no norms-minus-dot expansion)
//   dp_row    one launch per k: I[k][l] = min_t I[k-1][t] + Jt[l-1][t], one wavefront per l, ties to the smaller t. The launch
//             boundary is the dependency between rows: no grid barrier, no atomics
//   select    one wavefront: obj(m) = I[m][n] / n + pen(m), first minimum, back-tracking through P, change points in frame units
#include "common.h"

#include <climits>
#include <cmath>

using namespace goalnet;

namespace {

constexpr int KTS_MAX_N = 8192;
constexpr int KTS_MAX_D = 4096;
constexpr int KTS_TILE = 64;          // scatter tile: 64 end indices x 64 start indices per block of 256 threads
constexpr int KTS_KC = 16;            // descriptor columns staged per step
constexpr int KTS_WALK = 16;          // rows fetched ahead of the running sum in the prefix walk

// sum over the block's 256 threads in a fixed tree, returned to every thread
__device__ __forceinline__ double block_sum_256(double v, double* red) {
    v = wave_sum_d(v);
    __syncthreads();                                              // red may still be read from the previous call
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
    __syncthreads();
    return (red[0] + red[1]) + (red[2] + red[3]);
}

__global__ __launch_bounds__(256) void kts_rowsq_kernel(const float* __restrict__ x, int n, int d, int normalize,
                                                       double* __restrict__ nrm, double* __restrict__ rowsq) {
    __shared__ double red[4];
    const int i = blockIdx.x;
    const float* row = x + (size_t)i * d;
    double s = 0.0;
    for (int c = threadIdx.x; c < d; c += 256) { const double v = (double)row[c]; s = fma(v, v, s); }
    const double total = block_sum_256(s, red);
    if (!normalize) {
        if (threadIdx.x == 0) { nrm[i] = 1.0; rowsq[i] = total; }
        return;
    }
    const double norm = sqrt(total);
    double q = 0.0;
    if (norm > 0.0)
        for (int c = threadIdx.x; c < d; c += 256) { const double v = (double)row[c] / norm; q = fma(v, v, q); }
    const double qs = block_sum_256(q, red);
    if (threadIdx.x == 0) { nrm[i] = norm; rowsq[i] = qs; }         // a row of zeros: norm 0, stays zero
}

// column c < d: S[(i+1)][c] = S[i][c] + x_i[c] (normalised); column d: D[i+1] = D[i] + rowsq[i]. Left to right, one thread each.
__global__ __launch_bounds__(64) void kts_prefix_kernel(const float* __restrict__ x, int n, int d, int normalize,
                                                       const double* __restrict__ nrm, const double* __restrict__ rowsq,
                                                       double* __restrict__ S, double* __restrict__ D) {
    const int c = blockIdx.x * 64 + threadIdx.x;
    if (c > d) return;
    double s = 0.0;
    if (c == d) {
        D[0] = 0.0;
        for (int i0 = 0; i0 < n; i0 += KTS_WALK) {
            double v[KTS_WALK];
#pragma unroll
            for (int u = 0; u < KTS_WALK; ++u) v[u] = i0 + u < n ? rowsq[i0 + u] : 0.0;
#pragma unroll
            for (int u = 0; u < KTS_WALK; ++u)
                if (i0 + u < n) { s += v[u]; D[i0 + u + 1] = s; }
        }
        return;
    }
    S[c] = 0.0;
    for (int i0 = 0; i0 < n; i0 += KTS_WALK) {
        double v[KTS_WALK];
#pragma unroll
        for (int u = 0; u < KTS_WALK; ++u) {
            const int i = i0 + u;
            double xv = 0.0;
            if (i < n) {
                xv = (double)x[(size_t)i * d + c];
                if (normalize) { const double nr = nrm[i]; xv = nr > 0.0 ? xv / nr : 0.0; }
            }
            v[u] = xv;
        }
#pragma unroll
        for (int u = 0; u < KTS_WALK; ++u)
            if (i0 + u < n) { s += v[u]; S[(size_t)(i0 + u + 1) * d + c] = s; }
    }
}

// Jt [n][n], row r = l - 1 (end index), column t (start index), written for t <= r only (the DP reads nothing else)
__global__ __launch_bounds__(256) void kts_scatter_kernel(const double* __restrict__ S, const double* __restrict__ D, int n, int d,
                                                         int lmin, int lmax, double* __restrict__ Jt) {
    __shared__ double Ls[KTS_KC][KTS_TILE + 1];                   // S[l] tile, [column][row]; + 1: the transposing store spreads over the banks
    __shared__ double Ts[KTS_KC][KTS_TILE + 1];                   // S[t] tile
    const int r0 = blockIdx.y * KTS_TILE, t0 = blockIdx.x * KTS_TILE;
    if (t0 > r0 + KTS_TILE - 1) return;                            // wholly above the diagonal (uniform over the block)
    const int tx = threadIdx.x & 15, ty = threadIdx.x >> 4;
    const int lr = threadIdx.x >> 4, lc = threadIdx.x & 15;        // staging: 16 rows x 16 columns per pass, 4 passes per tile
    double acc[4][4];
#pragma unroll
    for (int a = 0; a < 4; ++a)
#pragma unroll
        for (int b = 0; b < 4; ++b) acc[a][b] = 0.0;
    for (int k0 = 0; k0 < d; k0 += KTS_KC) {
#pragma unroll
        for (int p = 0; p < 4; ++p) {
            const int row = lr + 16 * p, col = k0 + lc;
            const int l = r0 + row + 1, t = t0 + row;               // S row l <= n, S row t <= n - 1
            Ls[lc][row] = (l <= n && col < d) ? S[(size_t)l * d + col] : 0.0;
            Ts[lc][row] = (t < n && col < d) ? S[(size_t)t * d + col] : 0.0;
        }
        __syncthreads();
#pragma unroll
        for (int kk = 0; kk < KTS_KC; ++kk) {
            double a[4], b[4];
#pragma unroll
            for (int u = 0; u < 4; ++u) { a[u] = Ls[kk][ty + 16 * u]; b[u] = Ts[kk][tx + 16 * u]; }
#pragma unroll
            for (int u = 0; u < 4; ++u)
#pragma unroll
                for (int w = 0; w < 4; ++w) { const double df = a[u] - b[w]; acc[u][w] = fma(df, df, acc[u][w]); }
        }
        __syncthreads();
    }
#pragma unroll
    for (int u = 0; u < 4; ++u) {
        const int r = r0 + ty + 16 * u;
        if (r >= n) continue;
        const double dl = D[r + 1];
#pragma unroll
        for (int w = 0; w < 4; ++w) {
            const int t = t0 + tx + 16 * w;
            if (t > r) continue;                                   // t <= r < n
            const int L = r + 1 - t;
            Jt[(size_t)r * n + t] = (L >= lmin && L <= lmax) ? (dl - D[t]) - acc[u][w] / (double)L : INFINITY;
        }
    }
}

// "smaller value, then smaller t"
__device__ __forceinline__ void kts_better(double& v, int& t, double ov, int ot) {
    if (ov < v || (ov == v && ot < t)) { v = ov; t = ot; }
}

// row k of I [(max_cp+1)][(n+1)] and P: one wavefront per l = 1 .. n, four per block. Row k - 1 is read-only during the launch.
__global__ __launch_bounds__(256) void kts_dp_row_kernel(const double* __restrict__ Jt, int n, int k, int lmin,
                                                        double* __restrict__ I, int32_t* __restrict__ P) {
    const int lane = threadIdx.x & 63;
    const int l = blockIdx.x * 4 + (threadIdx.x >> 6) + 1;
    const size_t ld = (size_t)n + 1;
    if (blockIdx.x == 0 && threadIdx.x == 0) { I[k * ld] = INFINITY; P[k * ld] = -1; }      // column 0: no samples, never read
    if (l > n) return;                                             // whole wavefronts leave together
    const double* jrow = Jt + (size_t)(l - 1) * n;
    if (k == 0) {
        if (lane == 0) { I[l] = jrow[0]; P[l] = -1; }
        return;
    }
    const double* prev = I + (size_t)(k - 1) * ld;
    const long long tlo = (long long)k * lmin;
    const int thi = l - lmin;
    double v = INFINITY;
    int bt = INT_MAX;
    if (tlo <= thi)
        for (int t = (int)tlo + lane; t <= thi; t += 64) {
            const double c = prev[t] + jrow[t];
            if (c < v) { v = c; bt = t; }                          // t rises within a lane: strict "<" keeps the smaller t
        }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        const double ov = __shfl_xor(v, o, 64);
        const int ot = __shfl_xor(bt, o, 64);
        kts_better(v, bt, ov, ot);
    }
    if (lane == 0) {
        I[k * ld + l] = v;
        P[k * ld + l] = v < INFINITY ? bt : -1;
    }
}

// one wavefront. cost / objective [max_cp+1], change_points [(max_cp+1)][2], cps_samples [max_cp]: rows past the chosen m hold -1.
__global__ __launch_bounds__(64) void kts_select_kernel(const double* __restrict__ I, const int32_t* __restrict__ P, int n, int max_cp,
                                                       double vmax, int skip, int full_n, int32_t* __restrict__ change_points,
                                                       int32_t* __restrict__ n_clips, int32_t* __restrict__ cps_samples,
                                                       double* __restrict__ cost, double* __restrict__ objective,
                                                       int32_t* __restrict__ status) {
    const int lane = threadIdx.x;
    const size_t ld = (size_t)n + 1;
    double v = INFINITY;
    int bm = INT_MAX;
    for (int m = lane; m <= max_cp; m += 64) {
        const double c = I[m * ld + n];
        const double pen = m == 0 ? 0.0 : (vmax * (double)m / (2.0 * (double)n)) * (log((double)n / (double)m) + 1.0);
        const double o = c < INFINITY ? c / (double)n + pen : INFINITY;
        cost[m] = c;
        objective[m] = o;
        if (o < v) { v = o; bm = m; }
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        const double ov = __shfl_xor(v, o, 64);
        const int om = __shfl_xor(bm, o, 64);
        kts_better(v, bm, ov, om);
    }
    const bool feasible = v < INFINITY;
    const int m = feasible ? bm : -1;
    for (int r = lane; r <= max_cp; r += 64)
        if (r > m) { change_points[2 * r] = -1; change_points[2 * r + 1] = -1; }
    for (int r = lane; r < max_cp; r += 64)
        if (r >= m) cps_samples[r] = -1;
    if (lane != 0) return;
    status[0] = feasible ? 0 : 1;
    n_clips[0] = m + 1;
    if (!feasible) return;
    int cur = n, end = full_n - 1;                                 // the last clip ends with the video
    for (int k = m; k >= 1; --k) {
        cur = P[k * ld + cur];
        cps_samples[k - 1] = cur;
        change_points[2 * k] = cur * skip;
        change_points[2 * k + 1] = end;
        end = cur * skip - 1;
    }
    change_points[0] = 0;
    change_points[1] = end;
}

size_t kts_align(size_t b) { return (b + 255) / 256 * 256; }

bool kts_dims_ok(int n, int d, int max_cp) { return n >= 1 && n <= KTS_MAX_N && d >= 1 && d <= KTS_MAX_D && max_cp >= 0 && max_cp <= n - 1; }

struct KtsLayout {
    size_t S, D, nrm, rowsq, Jt, I, P, total;
    KtsLayout(int n, int d, int max_cp) {
        const size_t N = (size_t)n, rows = (size_t)max_cp + 1;
        size_t o = 0;
        S = o; o += kts_align((N + 1) * (size_t)d * sizeof(double));
        D = o; o += kts_align((N + 1) * sizeof(double));
        nrm = o; o += kts_align(N * sizeof(double));
        rowsq = o; o += kts_align(N * sizeof(double));
        Jt = o; o += kts_align(N * N * sizeof(double));
        I = o; o += kts_align(rows * (N + 1) * sizeof(double));
        P = o; o += kts_align(rows * (N + 1) * sizeof(int32_t));
        total = o;
    }
};

}  // namespace

extern "C" {

size_t goalnet_kts_ws_bytes(int n, int d, int max_cp) {
    if (!kts_dims_ok(n, d, max_cp)) return 0;
    return KtsLayout(n, d, max_cp).total;
}

int goalnet_kts(const float* x, int n, int d, int normalize, int max_cp, int lmin, int lmax, double vmax, int skip_frames,
                int full_n_frames, int32_t* change_points, int32_t* n_clips, int32_t* cps_samples, double* cost, double* objective,
                int32_t* status, void* ws, size_t ws_bytes, void* stream) {
    GN_REQUIRE(x && change_points && n_clips && cps_samples && cost && objective && status && ws, GOALNET_E_NULL, "kts: null pointer");
    GN_REQUIRE(n >= 1 && n <= KTS_MAX_N && d >= 1 && d <= KTS_MAX_D, GOALNET_E_SHAPE, "kts: need 1 <= n <= %d and 1 <= d <= %d",
               KTS_MAX_N, KTS_MAX_D);
    GN_REQUIRE(max_cp >= 0 && max_cp <= n - 1, GOALNET_E_SHAPE, "kts: need 0 <= max_cp <= n - 1");
    GN_REQUIRE(lmin >= 1 && lmax >= lmin, GOALNET_E_SHAPE, "kts: need 1 <= lmin <= lmax");
    GN_REQUIRE(vmax == vmax, GOALNET_E_SHAPE, "kts: vmax is NaN");
    GN_REQUIRE(skip_frames >= 1, GOALNET_E_SHAPE, "kts: skip_frames must be positive");
    GN_REQUIRE((int64_t)full_n_frames > (int64_t)(n - 1) * skip_frames && (int64_t)full_n_frames <= (int64_t)n * skip_frames,
               GOALNET_E_SHAPE, "kts: full_n_frames must satisfy n = ceil(full_n_frames / skip_frames)");
    GN_REQUIRE(aligned16(ws), GOALNET_E_ALIGN, "kts: the workspace must be 16-byte aligned");
    const KtsLayout lay(n, d, max_cp);
    GN_REQUIRE(ws_bytes >= lay.total, GOALNET_E_WORKSPACE, "kts: workspace too small");
    hipStream_t st = (hipStream_t)stream;
    char* base = (char*)ws;
    double* S = (double*)(base + lay.S);
    double* D = (double*)(base + lay.D);
    double* nrm = (double*)(base + lay.nrm);
    double* rowsq = (double*)(base + lay.rowsq);
    double* Jt = (double*)(base + lay.Jt);
    double* I = (double*)(base + lay.I);
    int32_t* P = (int32_t*)(base + lay.P);
    hipLaunchKernelGGL(kts_rowsq_kernel, dim3(n), dim3(256), 0, st, x, n, d, normalize, nrm, rowsq);
    GN_LAUNCH_CHECK("kts.rowsq");
    hipLaunchKernelGGL(kts_prefix_kernel, dim3((d + 1 + 63) / 64), dim3(64), 0, st, x, n, d, normalize, (const double*)nrm,
                       (const double*)rowsq, S, D);
    GN_LAUNCH_CHECK("kts.prefix");
    const int tiles = (n + KTS_TILE - 1) / KTS_TILE;
    hipLaunchKernelGGL(kts_scatter_kernel, dim3(tiles, tiles), dim3(256), 0, st, (const double*)S, (const double*)D, n, d, lmin, lmax, Jt);
    GN_LAUNCH_CHECK("kts.scatter");
    for (int k = 0; k <= max_cp; ++k) {
        hipLaunchKernelGGL(kts_dp_row_kernel, dim3((n + 3) / 4), dim3(256), 0, st, (const double*)Jt, n, k, lmin, I, P);
        GN_LAUNCH_CHECK("kts.dp_row");
    }
    hipLaunchKernelGGL(kts_select_kernel, dim3(1), dim3(64), 0, st, (const double*)I, (const int32_t*)P, n, max_cp, vmax, skip_frames,
                       full_n_frames, change_points, n_clips, cps_samples, cost, objective, status);
    GN_LAUNCH_CHECK("kts.select");
    return 0;
}

}  // extern "C"
