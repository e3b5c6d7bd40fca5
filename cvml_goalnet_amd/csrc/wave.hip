// Audio front end (include/goalnet_wave.h; EXTENSION, scipy.signal.resample_poly's arithmetic): interleaved int16 / float32 frames
// -> mono -> polyphase resampling to the feature rate, float64 throughout, one rounding to float32 at the end. One block makes
// WAVE_BLOCK consecutive outputs: it downmixes the input frames they touch ONCE into LDS as doubles (zeros outside the signal),
// then every thread walks its phase row over that window in ascending tap order. The order of one output's fma chain is fixed, so
// the bits are those of the definition for any launch geometry.
#include "common.h"
#include "../../include/goalnet_wave.h"

using namespace goalnet;

namespace {

constexpr int WAVE_BLOCK = 256;               // threads per block = outputs per block
constexpr int64_t WAVE_MAX_GRID = 2147483647; // blocks in grid.x

__host__ __device__ inline int64_t ceil_div64(int64_t a, int64_t b) { return (a + b - 1) / b; }

// the mono sample of frame i: channels summed in order as doubles, divided by C; int16 scaled by 2^-15 (exact)
template <typename T, int CT>
__device__ __forceinline__ double mono_of(const T* __restrict__ x, int64_t i, int C) {
    const int c_n = CT > 0 ? CT : C;
    const T* f = x + i * c_n;
    double s = (double)f[0];
    for (int c = 1; c < c_n; ++c) s += (double)f[c];
    s /= (double)c_n;
    if (sizeof(T) == 2) s *= 0x1p-15;
    return s;
}

template <typename T, int CT>
__global__ __launch_bounds__(WAVE_BLOCK) void wave_identity_kernel(const T* __restrict__ x, int64_t n, int C, float* __restrict__ y) {
    for (int64_t k = (int64_t)blockIdx.x * WAVE_BLOCK + threadIdx.x; k < n; k += (int64_t)gridDim.x * WAVE_BLOCK)
        y[k] = (float)mono_of<T, CT>(x, k, C);
}

// LDS: win[slots] doubles, then (UP1) the one phase row. Slot s holds frame w0 + s, w0 = (t0 div up) - (L - 1); output d of the
// block reads slots ql + L - 1 - j, ql = ((t0 mod up) + d * down) div up <= slots - L.
template <typename T, int CT, bool UP1>
__global__ __launch_bounds__(WAVE_BLOCK) void wave_resample_kernel(const T* __restrict__ x, int64_t n_in, int C, const double* __restrict__ taps,
                                                                   int up, int down, int half_len, int L, float* __restrict__ y, int64_t n_out) {
    extern __shared__ double lds[];
    const int64_t k0 = (int64_t)blockIdx.x * WAVE_BLOCK;
    const int64_t left = n_out - k0;                                   // >= 1: the grid is ceil(n_out / WAVE_BLOCK)
    const int count = left < WAVE_BLOCK ? (int)left : WAVE_BLOCK;
    const int64_t t0 = k0 * down + half_len;                           // < 2^62 + 2^28 by the host's checks
    const int64_t q0 = t0 / up;
    const int64_t r0 = t0 - q0 * up;
    const int slots = (int)((r0 + (int64_t)(count - 1) * down) / up) + L;      // <= floor(255 down / up) + 1 + L <= 4402
    const int64_t w0 = q0 - (L - 1);
    double* win = lds;
    for (int s = threadIdx.x; s < slots; s += WAVE_BLOCK) {
        const int64_t i = w0 + s;
        win[s] = (i >= 0 && i < n_in) ? mono_of<T, CT>(x, i, C) : 0.0;
    }
    const double* row = taps;
    if (UP1) {
        double* trow = lds + slots;
        for (int j = threadIdx.x; j < L; j += WAVE_BLOCK) trow[j] = taps[j];
        row = trow;
    }
    __syncthreads();
    const int d = threadIdx.x;
    if (d >= count) return;
    const int64_t tl = r0 + (int64_t)d * down;
    const int64_t ql = tl / up;
    if (!UP1) row += (tl - ql * up) * L;
    const double* w = win + ql + (L - 1);                              // w[-j] is frame q - j
    double acc = 0.0;
    if (w0 >= 0 && w0 + slots <= n_in) {                               // block-uniform: the whole window lies inside the signal
#pragma unroll 4
        for (int j = 0; j < L; ++j) acc = __builtin_fma(row[j], w[-j], acc);
    } else {
        const int64_t q = q0 + ql;
        for (int j = 0; j < L; ++j) {
            const int64_t i = q - j;
            if (i >= 0 && i < n_in) acc = __builtin_fma(row[j], w[-j], acc);
        }
    }
    y[k0 + d] = (float)acc;
}

template <typename T, int CT>
void launch_wave(const T* x, int64_t n_in, int C, const double* taps, int up, int down, int half_len, int L, float* y, int64_t n_out,
                 hipStream_t st) {
    if (up == 1 && down == 1) {
        int64_t blocks = ceil_div64(n_out, WAVE_BLOCK);
        if (blocks > 65536) blocks = 65536;
        hipLaunchKernelGGL((wave_identity_kernel<T, CT>), dim3((unsigned)blocks), dim3(WAVE_BLOCK), 0, st, x, n_in, C, y);
        return;
    }
    const dim3 grid((unsigned)ceil_div64(n_out, WAVE_BLOCK));
    const int64_t slots = ((int64_t)(up - 1) + (int64_t)(WAVE_BLOCK - 1) * down) / up + L;
    if (up == 1)
        hipLaunchKernelGGL((wave_resample_kernel<T, CT, true>), grid, dim3(WAVE_BLOCK), (size_t)(slots + L) * sizeof(double), st, x, n_in, C, taps,
                           up, down, half_len, L, y, n_out);
    else
        hipLaunchKernelGGL((wave_resample_kernel<T, CT, false>), grid, dim3(WAVE_BLOCK), (size_t)slots * sizeof(double), st, x, n_in, C, taps, up,
                           down, half_len, L, y, n_out);
}

template <typename T>
void launch_wave_c(const T* x, int64_t n_in, int C, const double* taps, int up, int down, int half_len, int L, float* y, int64_t n_out,
                   hipStream_t st) {
    if (C == 1) launch_wave<T, 1>(x, n_in, C, taps, up, down, half_len, L, y, n_out, st);
    else if (C == 2) launch_wave<T, 2>(x, n_in, C, taps, up, down, half_len, L, y, n_out, st);
    else launch_wave<T, 0>(x, n_in, C, taps, up, down, half_len, L, y, n_out, st);
}

int gcd_int(int a, int b) {
    while (b) { const int t = a % b; a = b; b = t; }
    return a;
}

// the ratio's own limits and sizes; 0 or the negative code (message set)
int wave_sizes(const char* who, int up, int down, int64_t n_in, int* half_len, int* L, int64_t* n_out) {
    GN_REQUIRE(up >= 1 && down >= 1 && up <= GOALNET_WAVE_MAX_RATE && down <= GOALNET_WAVE_MAX_RATE, GOALNET_E_VALUE,
               "%s: up and down must lie in 1 .. %d, got %d / %d", who, GOALNET_WAVE_MAX_RATE, up, down);
    GN_REQUIRE((int64_t)down <= (int64_t)GOALNET_WAVE_MAX_RATIO * up, GOALNET_E_VALUE, "%s: down = %d > %d * up = %d: the ratio limit", who, down,
               GOALNET_WAVE_MAX_RATIO, up);
    const int m = up > down ? up : down;
    GN_REQUIRE(n_in >= 0 && n_in < ((int64_t)1 << 62) / m, GOALNET_E_SHAPE, "%s: n_in = %lld: 0 <= n_in and n_in * max(up, down) < 2^62", who,
               (long long)n_in);
    if (up == 1 && down == 1) {
        *half_len = 0;
        *L = 0;
    } else {
        *half_len = 10 * m;
        *L = (int)ceil_div64(2ll * *half_len + 1, up);
    }
    *n_out = ceil_div64(n_in * up, down);
    return 0;
}

}  // namespace

extern "C" {

int goalnet_wave_plan(int sr_in, int sr_out, int64_t n_in, int* up, int* down, int* half_len, int* taps_per_phase, int64_t* n_out) {
    GN_REQUIRE(up && down && half_len && taps_per_phase && n_out, GOALNET_E_NULL, "wave_plan: null result pointer");
    GN_REQUIRE(sr_in >= 1 && sr_out >= 1 && sr_in <= GOALNET_WAVE_MAX_RATE && sr_out <= GOALNET_WAVE_MAX_RATE, GOALNET_E_VALUE,
               "wave_plan: rates must lie in 1 .. %d, got %d -> %d", GOALNET_WAVE_MAX_RATE, sr_in, sr_out);
    const int g = gcd_int(sr_in, sr_out);
    const int u = sr_out / g, d = sr_in / g;
    int h = 0, l = 0;
    int64_t n = 0;
    const int rc = wave_sizes("wave_plan", u, d, n_in, &h, &l, &n);
    if (rc) return rc;
    *up = u; *down = d; *half_len = h; *taps_per_phase = l; *n_out = n;
    return 0;
}

int goalnet_wave_resample(const void* x, int fmt, int64_t n_in, int channels, const double* taps, int up, int down,
                          int half_len, int taps_per_phase, float* y, int64_t n_out, void* stream) {
    GN_REQUIRE(x && y, GOALNET_E_NULL, "wave_resample: null pointer");
    GN_REQUIRE(fmt == GOALNET_WAVE_F32 || fmt == GOALNET_WAVE_S16, GOALNET_E_VALUE, "wave_resample: fmt = %d is neither F32 (0) nor S16 (1)", fmt);
    GN_REQUIRE(channels >= 1 && channels <= GOALNET_WAVE_MAX_CHANNELS, GOALNET_E_SHAPE, "wave_resample: channels = %d outside 1 .. %d", channels,
               GOALNET_WAVE_MAX_CHANNELS);
    GN_REQUIRE(n_in >= 1, GOALNET_E_SHAPE, "wave_resample: n_in = %lld < 1", (long long)n_in);
    int h = 0, l = 0;
    int64_t n = 0;
    const int rc = wave_sizes("wave_resample", up, down, n_in, &h, &l, &n);
    if (rc) return rc;
    GN_REQUIRE(gcd_int(up, down) == 1, GOALNET_E_VALUE, "wave_resample: up = %d and down = %d are not coprime", up, down);
    GN_REQUIRE(taps || (up == 1 && down == 1), GOALNET_E_NULL, "wave_resample: null taps");
    GN_REQUIRE(half_len == h && taps_per_phase == l, GOALNET_E_VALUE, "wave_resample: half_len = %d, taps_per_phase = %d, the plan gives %d, %d",
               half_len, taps_per_phase, h, l);
    GN_REQUIRE(n_out == n, GOALNET_E_SHAPE, "wave_resample: n_out = %lld, the plan gives %lld", (long long)n_out, (long long)n);
    GN_REQUIRE(ceil_div64(n_out, WAVE_BLOCK) <= WAVE_MAX_GRID, GOALNET_E_SHAPE, "wave_resample: n_out = %lld needs more than 2^31 - 1 blocks",
               (long long)n_out);
    const size_t item = fmt == GOALNET_WAVE_S16 ? sizeof(int16_t) : sizeof(float);
    GN_REQUIRE((reinterpret_cast<uintptr_t>(x) & (item - 1)) == 0 && (reinterpret_cast<uintptr_t>(y) & 3u) == 0 &&
               (reinterpret_cast<uintptr_t>(taps) & 7u) == 0, GOALNET_E_ALIGN, "wave_resample: x, taps and y must be naturally aligned");
    hipStream_t st = (hipStream_t)stream;
    if (fmt == GOALNET_WAVE_S16) launch_wave_c<int16_t>((const int16_t*)x, n_in, channels, taps, up, down, h, l, y, n_out, st);
    else launch_wave_c<float>((const float*)x, n_in, channels, taps, up, down, h, l, y, n_out, st);
    GN_LAUNCH_CHECK("wave_resample");
    return 0;
}

}  // extern "C"
