// The small ops of the hot path: AudBl's two Conv1d layers, the 128 -> 1 head with Sigmoid and 4y+1,
// the broadcast MSE loss, bias-gradient column sums and elementwise helpers (the fused Adam step is adam.hip's).
// The reference's utils.py:203-227 (AudBl), 255-256, 270 (head), main.py:68-70 (loss).
//
// Together they are < 1 % of the model's arithmetic and touch kilobytes to a few
// megabytes: they are written for correctness and determinism, not for a roofline.
#include "common.h"
#include "mse.h"

using namespace goalnet;

namespace {

// ---------------------------------------------------------------------------------------------
// Conv1d (kernel 3), NCL layout.
// ---------------------------------------------------------------------------------------------
// 16 lanes (one DPP row) per output element: the lanes split the input channels, row16_sum adds them in a fixed order.
__global__ __launch_bounds__(256) void conv1d_fwd_kernel(const float* __restrict__ x, const float* __restrict__ w,
                                                        const float* __restrict__ b, int relu, float* __restrict__ y,
                                                        int N, int Cin, int L, int Cout, int Lo, int stride, int pad) {
    const int64_t total = (int64_t)N * Cout * Lo;
    const int g = threadIdx.x & 15;
    const int64_t step = (int64_t)gridDim.x * 16;
    const int64_t rounds = (total + step - 1) / step;          // every lane runs the same number of rounds (DPP needs full rows)
    int64_t i = (int64_t)blockIdx.x * 16 + (threadIdx.x >> 4);
    for (int64_t r = 0; r < rounds; ++r, i += step) {
        const bool ok = i < total;
        const int64_t ic = ok ? i : 0;
        const int lo = (int)(ic % Lo);
        const int co = (int)((ic / Lo) % Cout);
        const int64_t n = ic / ((int64_t)Lo * Cout);
        const float* xs = x + n * Cin * L;
        const float* ws = w + (int64_t)co * Cin * 3;
        float acc = 0.f;
        const int l0 = stride * lo - pad;
        for (int ci = g; ci < Cin; ci += 16) {
#pragma unroll
            for (int k = 0; k < 3; ++k) {
                const int l = l0 + k;
                if ((unsigned)l < (unsigned)L) acc = fmaf(xs[ci * L + l], ws[ci * 3 + k], acc);
            }
        }
        acc = row16_sum(acc) + b[co];
        if (ok && g == 0) y[i] = relu ? fmaxf(acc, 0.f) : acc;
    }
}

// dx[n][ci][l] = sum_{co,k : stride*lo - pad + k = l} dz[n][co][lo] * w[co][ci][k]; 16 lanes split the output channels
__global__ __launch_bounds__(256) void conv1d_dx_kernel(const float* __restrict__ dz, const float* __restrict__ w,
                                                       float* __restrict__ dx, int N, int Cin, int L, int Cout, int Lo,
                                                       int stride, int pad) {
    const int64_t total = (int64_t)N * Cin * L;
    const int g = threadIdx.x & 15;
    const int64_t step = (int64_t)gridDim.x * 16;
    const int64_t rounds = (total + step - 1) / step;
    int64_t i = (int64_t)blockIdx.x * 16 + (threadIdx.x >> 4);
    for (int64_t r = 0; r < rounds; ++r, i += step) {
        const bool ok = i < total;
        const int64_t ic = ok ? i : 0;
        const int l = (int)(ic % L);
        const int ci = (int)((ic / L) % Cin);
        const int64_t n = ic / ((int64_t)L * Cin);
        const float* dzs = dz + n * Cout * Lo;
        float acc = 0.f;
#pragma unroll
        for (int k = 0; k < 3; ++k) {
            const int t = l + pad - k;
            if (t < 0 || t % stride != 0) continue;
            const int lo = t / stride;
            if (lo >= Lo) continue;
            for (int co = g; co < Cout; co += 16) acc = fmaf(dzs[co * Lo + lo], w[((int64_t)co * Cin + ci) * 3 + k], acc);
        }
        acc = row16_sum(acc);
        if (ok && g == 0) dx[i] = acc;
    }
}

// ---- the same two gradients for many frames (N >= 64: the 1024-frame batches of bench.py) -----------------------------
// dX: one thread per output, channels fastest so that a wave reads the weights w[co][ci..ci+63][k] as one 768-B run
__global__ __launch_bounds__(256) void conv1d_dx_big_kernel(const float* __restrict__ dz, const float* __restrict__ w,
                                                           float* __restrict__ dx, int N, int Cin, int L, int Cout, int Lo,
                                                           int stride, int pad) {
    const int64_t total = (int64_t)N * L * Cin;
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (int64_t)gridDim.x * blockDim.x) {
        const int ci = (int)(i % Cin);
        const int l = (int)((i / Cin) % L);
        const int64_t n = i / ((int64_t)Cin * L);
        const float* dzs = dz + n * Cout * Lo;
        float acc = 0.f;
#pragma unroll
        for (int k = 0; k < 3; ++k) {
            const int t = l + pad - k;
            if (t < 0 || t % stride != 0) continue;
            const int lo = t / stride;
            if (lo >= Lo) continue;
            for (int co = 0; co < Cout; ++co) acc = fmaf(dzs[co * Lo + lo], w[((int64_t)co * Cin + ci) * 3 + k], acc);
        }
        dx[(n * Cin + ci) * L + l] = acc;
    }
}

// dW: block = 4 x 4 (co, ci) pairs x 16 frame lanes; every lane walks its frames (fp32 per frame, fp64 across frames), the 16
// lane totals of a pair are added in a fixed order. The block re-uses each dz / x row 4 times from L1.
__global__ __launch_bounds__(256) void conv1d_dw_big_kernel(const float* __restrict__ x, const float* __restrict__ dz,
                                                           float* __restrict__ dw, double* __restrict__ part, int N, int Cin, int L,
                                                           int Cout, int Lo, int stride, int pad) {
    __shared__ double red[16][16][3];
    const int pair = threadIdx.x >> 4, lanef = threadIdx.x & 15;
    const int cig = (Cin + 3) / 4;
    const int co = (blockIdx.x / cig) * 4 + (pair >> 2), ci = (blockIdx.x % cig) * 4 + (pair & 3);
    // blockIdx.y = slice of the frames (gridDim.y > 1: fp64 partial sums to `part`, added in slice order by
    // conv1d_dw_sum_kernel; with one slice a lane walked N / 16 frames: 0.42 ms at 1024 frames for 0.2 GFLOP)
    const int n0 = (int)((int64_t)N * blockIdx.y / gridDim.y), n1 = (int)((int64_t)N * (blockIdx.y + 1) / gridDim.y);
    double a0 = 0.0, a1 = 0.0, a2 = 0.0;
    if (co < Cout && ci < Cin) {
        for (int n = n0 + lanef; n < n1; n += 16) {
            const float* xs = x + ((int64_t)n * Cin + ci) * L;
            const float* ds = dz + ((int64_t)n * Cout + co) * Lo;
            float s0 = 0.f, s1 = 0.f, s2 = 0.f;
            for (int lo = 0; lo < Lo; ++lo) {
                const float d = ds[lo];
                const int l0 = stride * lo - pad;
                if ((unsigned)(l0) < (unsigned)L) s0 = fmaf(d, xs[l0], s0);
                if ((unsigned)(l0 + 1) < (unsigned)L) s1 = fmaf(d, xs[l0 + 1], s1);
                if ((unsigned)(l0 + 2) < (unsigned)L) s2 = fmaf(d, xs[l0 + 2], s2);
            }
            a0 += s0; a1 += s1; a2 += s2;
        }
    }
    red[pair][lanef][0] = a0; red[pair][lanef][1] = a1; red[pair][lanef][2] = a2;
    __syncthreads();
    if (lanef < 3 && co < Cout && ci < Cin) {
        double t = 0.0;
#pragma unroll
        for (int j = 0; j < 16; ++j) t += red[pair][j][lanef];
        const int64_t o = ((int64_t)co * Cin + ci) * 3 + lanef;
        if (gridDim.y == 1) dw[o] = (float)t;
        else part[(int64_t)blockIdx.y * Cout * Cin * 3 + o] = t;
    }
}

__global__ __launch_bounds__(256) void conv1d_dw_sum_kernel(const double* __restrict__ part, int slices, int64_t n, float* __restrict__ dw) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    double t = 0.0;
    for (int s = 0; s < slices; ++s) t += part[(int64_t)s * n + i];
    dw[i] = (float)t;
}

// dw[co][ci][k] = sum_{n,lo} dz[n][co][lo] * x[n][ci][stride*lo - pad + k]; one block per (co, ci), the 256
// threads split the frames, fp64 block reduction (deterministic).
__global__ __launch_bounds__(256) void conv1d_dw_kernel(const float* __restrict__ x, const float* __restrict__ dz,
                                                       float* __restrict__ dw, int N, int Cin, int L, int Cout, int Lo,
                                                       int stride, int pad) {
    __shared__ double red[4][3];
    const int co = blockIdx.x / Cin, ci = blockIdx.x % Cin;
    double a0 = 0.0, a1 = 0.0, a2 = 0.0;
    for (int n = threadIdx.x; n < N; n += 256) {
        const float* xs = x + ((int64_t)n * Cin + ci) * L;
        const float* ds = dz + ((int64_t)n * Cout + co) * Lo;
        float s0 = 0.f, s1 = 0.f, s2 = 0.f;
        for (int lo = 0; lo < Lo; ++lo) {
            const float d = ds[lo];
            const int l0 = stride * lo - pad;
            if ((unsigned)(l0) < (unsigned)L) s0 = fmaf(d, xs[l0], s0);
            if ((unsigned)(l0 + 1) < (unsigned)L) s1 = fmaf(d, xs[l0 + 1], s1);
            if ((unsigned)(l0 + 2) < (unsigned)L) s2 = fmaf(d, xs[l0 + 2], s2);
        }
        a0 += s0; a1 += s1; a2 += s2;
    }
    a0 = wave_sum_d(a0); a1 = wave_sum_d(a1); a2 = wave_sum_d(a2);
    const int wv = threadIdx.x >> 6;
    if ((threadIdx.x & 63) == 0) { red[wv][0] = a0; red[wv][1] = a1; red[wv][2] = a2; }
    __syncthreads();
    if (threadIdx.x < 3)
        dw[(int64_t)blockIdx.x * 3 + threadIdx.x] =
            (float)(red[0][threadIdx.x] + red[1][threadIdx.x] + red[2][threadIdx.x] + red[3][threadIdx.x]);
}

// db[co] = sum_{n,lo} dz[n][co][lo]; one block per co
__global__ __launch_bounds__(256) void conv1d_db_kernel(const float* __restrict__ dz, float* __restrict__ db, int N, int Cout, int Lo) {
    __shared__ double red[4];
    const int co = blockIdx.x;
    double a = 0.0;
    for (int n = threadIdx.x; n < N; n += 256) {
        const float* ds = dz + ((int64_t)n * Cout + co) * Lo;
        float s = 0.f;
        for (int lo = 0; lo < Lo; ++lo) s += ds[lo];
        a += s;
    }
    a = wave_sum_d(a);
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = a;
    __syncthreads();
    if (threadIdx.x == 0) db[co] = (float)(red[0] + red[1] + red[2] + red[3]);
}

// ---- few frames (N < 64: the reference's 10-frame sub-batches): the whole backward of one Conv1d layer in ONE launch.
// y (nullable) is the layer's own ReLU output: the effective output gradient is dz * (y > 0), so no separate ReLU-backward pass.
// Blocks [0, nA): weight + bias gradient. A block owns 256 / Cin output channels x all Cin input channels, one (co, ci) pair
// per thread; the gated dz rows of its channels sit in LDS, x is read through L1 / L2 (36 KB in all). Per frame the taps are
// summed in fp32, across frames in fp64, frames in index order (conv1d_dw_kernel's arithmetic).
// Blocks [nA, ...): data gradient, 16 lanes per output element splitting the output channels (conv1d_dx_kernel).
__global__ __launch_bounds__(256) void conv1d_bwd_small_kernel(const float* __restrict__ x, const float* __restrict__ dz,
                                                              const float* __restrict__ y, const float* __restrict__ w,
                                                              float* __restrict__ dx, float* __restrict__ dw, float* __restrict__ db,
                                                              int N, int Cin, int L, int Cout, int Lo, int stride, int pad, int nA) {
    extern __shared__ float dzs[];                        // part A: [N][cpb][Lo]
    if ((int)blockIdx.x < nA) {
        const int cpb = 256 / Cin;
        const int co0 = blockIdx.x * cpb;
        const int tot = N * cpb * Lo;
        for (int i = threadIdx.x; i < tot; i += 256) {
            const int lo = i % Lo, cl = (i / Lo) % cpb, n = i / (Lo * cpb);
            float v = 0.f;
            if (co0 + cl < Cout) {
                const int64_t o = ((int64_t)n * Cout + co0 + cl) * Lo + lo;
                v = dz[o];
                if (y && !(y[o] > 0.f)) v = 0.f;
            }
            dzs[i] = v;
        }
        __syncthreads();
        const int cl = threadIdx.x / Cin, ci = threadIdx.x - cl * Cin;
        if (cl < cpb && co0 + cl < Cout) {
            double a0 = 0.0, a1 = 0.0, a2 = 0.0;
            for (int n = 0; n < N; ++n) {
                const float* xs = x + ((int64_t)n * Cin + ci) * L;
                const float* ds = dzs + (n * cpb + cl) * Lo;
                float s0 = 0.f, s1 = 0.f, s2 = 0.f;
                for (int lo = 0; lo < Lo; ++lo) {
                    const float d = ds[lo];
                    const int l0 = stride * lo - pad;
                    if ((unsigned)(l0) < (unsigned)L) s0 = fmaf(d, xs[l0], s0);
                    if ((unsigned)(l0 + 1) < (unsigned)L) s1 = fmaf(d, xs[l0 + 1], s1);
                    if ((unsigned)(l0 + 2) < (unsigned)L) s2 = fmaf(d, xs[l0 + 2], s2);
                }
                a0 += s0; a1 += s1; a2 += s2;
            }
            float* o = dw + ((int64_t)(co0 + cl) * Cin + ci) * 3;
            o[0] = (float)a0; o[1] = (float)a1; o[2] = (float)a2;
        }
        if ((int)threadIdx.x < cpb && co0 + (int)threadIdx.x < Cout) {
            double a = 0.0;
            for (int n = 0; n < N; ++n) {
                const float* ds = dzs + (n * cpb + threadIdx.x) * Lo;
                float t = 0.f;
                for (int lo = 0; lo < Lo; ++lo) t += ds[lo];
                a += t;
            }
            db[co0 + threadIdx.x] = (float)a;
        }
        return;
    }
    const int64_t total = (int64_t)N * Cin * L;
    const int g = threadIdx.x & 15;
    const int64_t step = (int64_t)(gridDim.x - nA) * 16;
    const int64_t rounds = (total + step - 1) / step;
    int64_t i = (int64_t)(blockIdx.x - nA) * 16 + (threadIdx.x >> 4);
    for (int64_t r = 0; r < rounds; ++r, i += step) {
        const bool ok = i < total;
        const int64_t ic = ok ? i : 0;
        const int l = (int)(ic % L);
        const int ci = (int)((ic / L) % Cin);
        const int64_t n = ic / ((int64_t)L * Cin);
        const float* dzr = dz + n * Cout * Lo;
        const float* yr = y ? y + n * Cout * Lo : nullptr;
        float acc = 0.f;
#pragma unroll
        for (int k = 0; k < 3; ++k) {
            const int t = l + pad - k;
            if (t < 0 || t % stride != 0) continue;
            const int lo = t / stride;
            if (lo >= Lo) continue;
            for (int co = g; co < Cout; co += 16) {
                float d = dzr[co * Lo + lo];
                if (yr && !(yr[co * Lo + lo] > 0.f)) d = 0.f;
                acc = fmaf(d, w[((int64_t)co * Cin + ci) * 3 + k], acc);
            }
        }
        acc = row16_sum(acc);
        if (ok && g == 0) dx[i] = acc;
    }
}

__global__ __launch_bounds__(256) void relu_bwd_kernel(const float* __restrict__ dy, const float* __restrict__ y,
                                                      float* __restrict__ dz, int64_t n) {
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x)
        dz[i] = y[i] > 0.f ? dy[i] : 0.f;
}

__global__ __launch_bounds__(256) void mul_kernel(const float* __restrict__ x, int64_t ldx, const float* __restrict__ m, int64_t ldm,
                                                 float* __restrict__ y, int64_t ldy, int M, int J) {
    const int64_t total = (int64_t)M * J;
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (int64_t)gridDim.x * blockDim.x) {
        const int64_t r = i / J;
        const int c = (int)(i - r * J);
        y[r * ldy + c] = x[r * ldx + c] * m[r * ldm + c];
    }
}

// out[j] = sum_m x[m][j]: block = 32 columns x 8 row lanes, fp64 accumulation
__global__ __launch_bounds__(256) void colsum_kernel(const float* __restrict__ x, int64_t ldx, int M, int J, float* __restrict__ out) {
    __shared__ double red[8][33];
    const int cx = threadIdx.x & 31, ry = threadIdx.x >> 5;
    const int col = blockIdx.x * 32 + cx;
    double a = 0.0;
    if (col < J)
        for (int m = ry; m < M; m += 8) a += (double)x[(int64_t)m * ldx + col];
    red[ry][cx] = a;
    __syncthreads();
    if (ry == 0 && col < J) {
        double s = 0.0;
#pragma unroll
        for (int i = 0; i < 8; ++i) s += red[i][cx];
        out[col] = (float)s;
    }
}

// ---------------------------------------------------------------------------------------------
// head: z = h . w + b ; out = 4 * sigmoid(z) + 1.  One wave per frame.
// ---------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void head_fwd_kernel(const float* __restrict__ h, int64_t ldh, const float* __restrict__ w,
                                                      const float* __restrict__ b, float* __restrict__ logit,
                                                      float* __restrict__ out, int N, int K) {
    const int lane = threadIdx.x & 63;
    const int n = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (n >= N) return;
    float acc = 0.f;
    for (int k = lane; k < K; k += 64) acc = fmaf(h[(int64_t)n * ldh + k], w[k], acc);
    acc = wave_sum(acc);
    if (lane == 0) {
        const float z = acc + b[0];
        if (logit) logit[n] = z;
        out[n] = 4.f / (1.f + expf(-z)) + 1.f;
    }
}

__device__ __forceinline__ float dlogit_of(float dout, float out) {
    // d/dz (4*sigmoid(z) + 1) = 4 s (1 - s), s = (out - 1) / 4
    const float s = (out - 1.f) * 0.25f;
    return dout * 4.f * s * (1.f - s);
}

__global__ __launch_bounds__(256) void head_bwd_dh_kernel(const float* __restrict__ dout, const float* __restrict__ out,
                                                         const float* __restrict__ w, const float* __restrict__ mult, int64_t ldmult,
                                                         float* __restrict__ dh, int64_t lddh, int N, int K) {
    const int64_t total = (int64_t)N * K;
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (int64_t)gridDim.x * blockDim.x) {
        const int64_t n = i / K;
        const int k = (int)(i - n * K);
        float v = dlogit_of(dout[n], out[n]) * w[k];
        if (mult) v *= mult[n * ldmult + k];
        dh[n * lddh + k] = v;
    }
}

// dw[k] = sum_n dlogit[n] h[n][k]; db = sum_n dlogit[n] (column K). Block = 64 columns x 16 row groups: a wave reads 64
// consecutive k of one row, every thread sums its rows in fp64, the 16 group totals of a column are added in a fixed order.
// (One thread per column walking all rows took 316 us at 1024 rows: a thousand dependent round trips.)
__global__ __launch_bounds__(1024) void head_bwd_dw_kernel(const float* __restrict__ dout, const float* __restrict__ out,
                                                          const float* __restrict__ h, int64_t ldh, float* __restrict__ dw,
                                                          float* __restrict__ db, int N, int K) {
    __shared__ double red[16][64];
    const int c = threadIdx.x & 63, rg = threadIdx.x >> 6;
    const int k = blockIdx.x * 64 + c;
    double a = 0.0;
    if (k <= K)
        for (int n = rg; n < N; n += 16) {
            const float g = dlogit_of(dout[n], out[n]);
            a += (double)(k < K ? g * h[(int64_t)n * ldh + k] : g);
        }
    red[rg][c] = a;
    __syncthreads();
    if (rg != 0 || k > K) return;
    double t = 0.0;
#pragma unroll
    for (int j = 0; j < 16; ++j) t += red[j][c];
    if (k < K) dw[k] = (float)t;
    else db[0] = (float)t;
}

// loss = 1/n^2 sum_i sum_j (p_i - y_j)^2 = mean_i (p_i^2 - 2 p_i ybar + mean(y^2)); dpred_i = 2/n (p_i - ybar)
__global__ __launch_bounds__(256) void mse_bcast_kernel(const float* __restrict__ pred, const float* __restrict__ labels, int N,
                                                       float* __restrict__ loss, float* __restrict__ dpred) {
    mse_bcast_block(pred, labels, N, loss, dpred);
}

// x *= s (the loss scale of precision = "fp16" on dL/dpred)
__global__ __launch_bounds__(256) void scale_kernel(float* __restrict__ x, int64_t n, float s) {
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x) x[i] *= s;
}

unsigned grid1d(int64_t n, int cap = 4096) {
    int64_t b = (n + 255) / 256;
    if (b > cap) b = cap;
    if (b < 1) b = 1;
    return (unsigned)b;
}

}  // namespace

extern "C" {

int goalnet_conv1d_fwd(const float* x, const float* w, const float* b, int relu, float* y,
                       int N, int Cin, int L, int Cout, int stride, int pad, void* stream) {
    GN_REQUIRE(x && w && b && y, GOALNET_E_NULL, "conv1d_fwd: null pointer");
    GN_REQUIRE(N > 0 && Cin > 0 && L > 0 && Cout > 0 && stride > 0 && pad >= 0 && L + 2 * pad >= 3, GOALNET_E_SHAPE, "conv1d_fwd: bad dims");
    const int Lo = (L + 2 * pad - 3) / stride + 1;
    hipLaunchKernelGGL(conv1d_fwd_kernel, dim3(grid1d((int64_t)N * Cout * Lo * 16)), dim3(256), 0, (hipStream_t)stream, x, w, b, relu, y,
                       N, Cin, L, Cout, Lo, stride, pad);
    GN_LAUNCH_CHECK("conv1d_fwd");
    return 0;
}

constexpr int CONV1D_DW_SLICES = 8;      // frame slices of the many-frame weight gradient

size_t goalnet_conv1d_bwd_ws_bytes(int N, int Cin, int Cout) {
    return N >= 64 * CONV1D_DW_SLICES ? (size_t)CONV1D_DW_SLICES * Cout * Cin * 3 * sizeof(double) : 0;
}

int goalnet_conv1d_bwd(const float* x, const float* dz, const float* w, float* dx, float* dw, float* db,
                       int N, int Cin, int L, int Cout, int stride, int pad, void* ws, size_t ws_bytes, void* stream) {
    GN_REQUIRE(x && dz && w && dw && db, GOALNET_E_NULL, "conv1d_bwd: null pointer");
    GN_REQUIRE(N > 0 && Cin > 0 && L > 0 && Cout > 0 && stride > 0 && pad >= 0 && L + 2 * pad >= 3, GOALNET_E_SHAPE, "conv1d_bwd: bad dims");
    const int Lo = (L + 2 * pad - 3) / stride + 1;
    hipStream_t st = (hipStream_t)stream;
    const bool many = N >= 64;          // few frames (the reference's sub-batches): lanes split the channels; many: lanes split the frames
    const size_t need = goalnet_conv1d_bwd_ws_bytes(N, Cin, Cout);
    // a workspace that is lent must be whole (ws = NULL: no frame slices); both checks precede the first launch
    GN_REQUIRE(!ws || ws_bytes >= need, GOALNET_E_WORKSPACE, "conv1d_bwd: workspace too small");
    GN_REQUIRE(!(ws && need) || (reinterpret_cast<uintptr_t>(ws) & 7u) == 0, GOALNET_E_ALIGN, "conv1d_bwd: workspace must be 8-byte aligned");
    if (dx) {
        if (many)
            hipLaunchKernelGGL(conv1d_dx_big_kernel, dim3(grid1d((int64_t)N * Cin * L)), dim3(256), 0, st, dz, w, dx, N, Cin, L, Cout, Lo, stride, pad);
        else
            hipLaunchKernelGGL(conv1d_dx_kernel, dim3(grid1d((int64_t)N * Cin * L * 16)), dim3(256), 0, st, dz, w, dx, N, Cin, L, Cout, Lo, stride, pad);
        GN_LAUNCH_CHECK("conv1d_bwd.dx");
    }
    if (many) {
        const int slices = need && ws ? CONV1D_DW_SLICES : 1;
        hipLaunchKernelGGL(conv1d_dw_big_kernel, dim3(((Cout + 3) / 4) * ((Cin + 3) / 4), slices), dim3(256), 0, st, x, dz, dw, (double*)ws,
                           N, Cin, L, Cout, Lo, stride, pad);
        if (slices > 1) {
            const int64_t n = (int64_t)Cout * Cin * 3;
            hipLaunchKernelGGL(conv1d_dw_sum_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, st, (const double*)ws, slices, n, dw);
        }
    } else
        hipLaunchKernelGGL(conv1d_dw_kernel, dim3(Cout * Cin), dim3(256), 0, st, x, dz, dw, N, Cin, L, Cout, Lo, stride, pad);
    GN_LAUNCH_CHECK("conv1d_bwd.dw");
    hipLaunchKernelGGL(conv1d_db_kernel, dim3(Cout), dim3(256), 0, st, dz, db, N, Cout, Lo);
    GN_LAUNCH_CHECK("conv1d_bwd.db");
    return 0;
}

/* whether goalnet_conv1d_bwd_small serves the dims: its own dim checks, and the dz rows a weight-gradient block keeps in LDS */
int goalnet_conv1d_bwd_small_ok(int N, int Cin, int L, int Cout, int stride, int pad) {
    if (!(N > 0 && N < 64 && Cin > 0 && Cin <= 256 && L > 0 && Cout > 0 && stride > 0 && pad >= 0 && L + 2 * pad >= 3)) return 0;
    const int64_t Lo = (L + 2 * pad - 3) / stride + 1;
    const int64_t cpb = 256 / Cin;
    return (int64_t)N * cpb * Lo * (int64_t)sizeof(float) <= 48 * 1024;          // the dz rows a weight-gradient block keeps in LDS
}

/* goalnet_conv1d_bwd for few frames (N < 64) in ONE launch, with the ReLU backward of the layer's own output folded in:
 * y (nullable) = the layer's ReLU output, effective dz = dz * (y > 0). dx nullable (first layer). Cin <= 256. */
int goalnet_conv1d_bwd_small(const float* x, const float* dz, const float* y, const float* w, float* dx, float* dw, float* db,
                             int N, int Cin, int L, int Cout, int stride, int pad, void* stream) {
    GN_REQUIRE(x && dz && w && dw && db, GOALNET_E_NULL, "conv1d_bwd_small: null pointer");
    GN_REQUIRE(N > 0 && N < 64 && Cin > 0 && Cin <= 256 && L > 0 && Cout > 0 && stride > 0 && pad >= 0 && L + 2 * pad >= 3, GOALNET_E_SHAPE,
               "conv1d_bwd_small: bad dims (N < 64, Cin <= 256)");
    GN_REQUIRE(goalnet_conv1d_bwd_small_ok(N, Cin, L, Cout, stride, pad), GOALNET_E_SHAPE,
               "conv1d_bwd_small: the dz rows of a block do not fit LDS (ask goalnet_conv1d_bwd_small_ok; use goalnet_relu_bwd + goalnet_conv1d_bwd)");
    const int Lo = (L + 2 * pad - 3) / stride + 1;
    const int cpb = 256 / Cin;
    const size_t lds = (size_t)N * cpb * Lo * sizeof(float);
    const int nA = (Cout + cpb - 1) / cpb;
    const int nB = dx ? (int)grid1d((int64_t)N * Cin * L * 16) : 0;
    hipLaunchKernelGGL(conv1d_bwd_small_kernel, dim3(nA + nB), dim3(256), lds, (hipStream_t)stream, x, dz, y, w, dx, dw, db,
                       N, Cin, L, Cout, Lo, stride, pad, nA);
    GN_LAUNCH_CHECK("conv1d_bwd_small");
    return 0;
}

int goalnet_relu_bwd(const float* dy, const float* y, float* dz, int64_t n, void* stream) {
    GN_REQUIRE(dy && y && dz, GOALNET_E_NULL, "relu_bwd: null pointer");
    GN_REQUIRE(n > 0, GOALNET_E_SHAPE, "relu_bwd: bad count");
    hipLaunchKernelGGL(relu_bwd_kernel, dim3(grid1d(n)), dim3(256), 0, (hipStream_t)stream, dy, y, dz, n);
    GN_LAUNCH_CHECK("relu_bwd");
    return 0;
}

int goalnet_mul(const float* x, int64_t ldx, const float* mult, int64_t ldmult, float* y, int64_t ldy,
                int M, int J, void* stream) {
    GN_REQUIRE(x && mult && y, GOALNET_E_NULL, "mul: null pointer");
    GN_REQUIRE(M > 0 && J > 0, GOALNET_E_SHAPE, "mul: bad dims");
    hipLaunchKernelGGL(mul_kernel, dim3(grid1d((int64_t)M * J)), dim3(256), 0, (hipStream_t)stream, x, ldx, mult, ldmult, y, ldy, M, J);
    GN_LAUNCH_CHECK("mul");
    return 0;
}

int goalnet_colsum(const float* x, int64_t ldx, int M, int J, float* out, void* stream) {
    GN_REQUIRE(x && out, GOALNET_E_NULL, "colsum: null pointer");
    GN_REQUIRE(M > 0 && J > 0, GOALNET_E_SHAPE, "colsum: bad dims");
    hipLaunchKernelGGL(colsum_kernel, dim3((J + 31) / 32), dim3(256), 0, (hipStream_t)stream, x, ldx, M, J, out);
    GN_LAUNCH_CHECK("colsum");
    return 0;
}

int goalnet_head_fwd(const float* h, int64_t ldh, const float* w, const float* b, float* logit, float* out,
                     int N, int K, void* stream) {
    GN_REQUIRE(h && w && b && out, GOALNET_E_NULL, "head_fwd: null pointer");
    GN_REQUIRE(N > 0 && K > 0, GOALNET_E_SHAPE, "head_fwd: bad dims");
    hipLaunchKernelGGL(head_fwd_kernel, dim3((N + 3) / 4), dim3(256), 0, (hipStream_t)stream, h, ldh, w, b, logit, out, N, K);
    GN_LAUNCH_CHECK("head_fwd");
    return 0;
}

int goalnet_head_bwd(const float* dout, const float* out, const float* h, int64_t ldh, const float* w,
                     const float* mult, int64_t ldmult, float* dh, int64_t lddh, float* dw, float* db,
                     int N, int K, void* stream) {
    GN_REQUIRE(dout && out && h && w && dh && dw && db, GOALNET_E_NULL, "head_bwd: null pointer");
    GN_REQUIRE(N > 0 && K > 0 && K < 1024, GOALNET_E_SHAPE, "head_bwd: bad dims (K < 1024)");
    hipStream_t st = (hipStream_t)stream;
    hipLaunchKernelGGL(head_bwd_dh_kernel, dim3(grid1d((int64_t)N * K)), dim3(256), 0, st, dout, out, w, mult, ldmult, dh, lddh, N, K);
    GN_LAUNCH_CHECK("head_bwd.dh");
    hipLaunchKernelGGL(head_bwd_dw_kernel, dim3((K + 1 + 63) / 64), dim3(1024), 0, st, dout, out, h, ldh, dw, db, N, K);
    GN_LAUNCH_CHECK("head_bwd.dw");
    return 0;
}

int goalnet_mse_bcast(const float* pred, const float* labels, int N, float* loss, float* dpred, void* stream) {
    GN_REQUIRE(pred && labels, GOALNET_E_NULL, "mse_bcast: null pointer");
    GN_REQUIRE(N > 0, GOALNET_E_SHAPE, "mse_bcast: bad count");
    hipLaunchKernelGGL(mse_bcast_kernel, dim3(1), dim3(256), 0, (hipStream_t)stream, pred, labels, N, loss, dpred);
    GN_LAUNCH_CHECK("mse_bcast");
    return 0;
}

int goalnet_scale(float* x, int64_t n, float s, void* stream) {
    GN_REQUIRE(x, GOALNET_E_NULL, "scale: null pointer");
    GN_REQUIRE(n > 0, GOALNET_E_SHAPE, "scale: bad count");
    hipLaunchKernelGGL(scale_kernel, dim3(grid1d(n, 8192)), dim3(256), 0, (hipStream_t)stream, x, n, s);
    GN_LAUNCH_CHECK("scale");
    return 0;
}

}  // extern "C"
