// Audio augmentation and mixup for a pass over a video resident on the device (include/goalnet_mix.h; EXTENSION, no reference code):
// the second plan table (per-frame audio draws, mixup partner and lambda), the audio gather that applies it, and the frame / row
// gathers that mix a row with its partner. Everything here is integer or non-contracted fp32, element-wise in the output: any
// launch geometry gives the bits of tests/_mix_ref.py. The kernels of epoch.hip are not touched.
#include "common.h"
#include "rng.h"
#include "../../include/goalnet_mix.h"

#include <math.h>

using namespace goalnet;

namespace {

constexpr uint64_t GAMMA = 0x9E3779B97F4A7C15ull;
constexpr uint32_t ONE_BITS = 0x3F800000u;      // 1.0f: the lambda of an unmixed row
constexpr float U24 = 5.9604644775390625e-08f;  // 2^-24, exact

__device__ __forceinline__ uint64_t stream_bits(uint64_t key, uint32_t r) { return mix64(key + (uint64_t)(r + 1u) * GAMMA); }      // rng.h: element r
__device__ __forceinline__ uint64_t u24_of(uint64_t key, uint32_t r) { return stream_bits(key, r) >> 40; }
__device__ __forceinline__ float unit_of(uint64_t key, uint32_t r) { return (float)(uint32_t)u24_of(key, r) * U24; }

// out = fmaf(a, lambda, 0) + fmaf(b, mu, 0): two rounded products, one rounded sum; fma(x, y, 0) cannot be contracted with the add
__device__ __forceinline__ uint32_t mix_words(uint32_t a, uint32_t b, float lambda) {
    const float mu = 1.0f - lambda;
    return __float_as_uint(__builtin_fmaf(__uint_as_float(a), lambda, 0.0f) + __builtin_fmaf(__uint_as_float(b), mu, 0.0f));
}

struct Plan2Keys { uint64_t k[10]; };

// one thread per position i; every draw is element r = plan[i].src of its stream
__global__ __launch_bounds__(256) void epoch_plan2_kernel(int32_t* __restrict__ plan2, const int32_t* __restrict__ plan, int n, Plan2Keys keys,
                                                          int C, int B, int max_shift, int time_mask, int coeff_mask, float g_lo, float g_span,
                                                          int gain_on, int noise_on, float l_lo, float l_span, float mix_p, int mix_on) {
    for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < n; i += gridDim.x * blockDim.x) {
        const uint32_t r = (uint32_t)plan[(int64_t)i * GOALNET_PLAN_WORDS];
        int a_shift = 0, t0 = 0, tw = 0, c0 = 0, cw = 0, partner = i;
        float gain = 1.0f, lambda = 1.0f;
        uint64_t nkey = 0;
        if (max_shift > 0) a_shift = (int)((u24_of(keys.k[0], r) * (2ull * (uint64_t)max_shift + 1ull)) >> 24) - max_shift;
        if (time_mask > 0) {
            tw = (int)((u24_of(keys.k[1], r) * (uint64_t)(time_mask + 1)) >> 24);
            t0 = (int)((u24_of(keys.k[2], r) * (uint64_t)(B - tw + 1)) >> 24);
        }
        if (coeff_mask > 0) {
            cw = (int)((u24_of(keys.k[3], r) * (uint64_t)(coeff_mask + 1)) >> 24);
            c0 = 1 + (int)((u24_of(keys.k[4], r) * (uint64_t)(C - cw)) >> 24);
        }
        if (gain_on) gain = g_lo + __builtin_fmaf(g_span, unit_of(keys.k[5], r), 0.0f);
        if (noise_on) nkey = stream_bits(keys.k[6], r);
        if (mix_on) {
            const int q = (int)((u24_of(keys.k[7], r) * (uint64_t)n) >> 24);
            const float l = l_lo + __builtin_fmaf(l_span, unit_of(keys.k[8], r), 0.0f);
            const bool apply = unit_of(keys.k[9], r) < mix_p;
            if (apply && q != i && __float_as_uint(l) != ONE_BITS) { partner = q; lambda = l; }
        }
        int4* row = reinterpret_cast<int4*>(plan2 + (int64_t)i * GOALNET_PLAN2_WORDS);
        row[0] = make_int4(a_shift, t0, tw, c0);
        row[1] = make_int4(cw, __float_as_int(gain), partner, __float_as_int(lambda));
        row[2] = make_int4((int)(uint32_t)nkey, (int)(uint32_t)(nkey >> 32), 0, 0);
    }
}

// steps 1-4 of the audio gather for plan row `prow` (in range) whose src is in range: the word at output coordinate (c, t)
template <bool GAIN, bool NOISE>
__device__ __forceinline__ uint32_t audio_word(const uint32_t* __restrict__ table, const int32_t* __restrict__ plan2, int64_t prow, int src, int C,
                                               int B, int c, int t, float n_lo, float n_span) {
    const int4 a = *reinterpret_cast<const int4*>(plan2 + prow * GOALNET_PLAN2_WORDS);             // a_shift, t0, tw, c0
    const int2 b = *reinterpret_cast<const int2*>(plan2 + prow * GOALNET_PLAN2_WORDS + 4);         // cw, gain
    // 64-bit: a plan is caller memory
    if (c >= 1 && ((t >= a.y && (int64_t)t < (int64_t)a.y + a.z) || (c >= a.w && (int64_t)c < (int64_t)a.w + b.x))) return 0u;        // +0.0
    int64_t st = (int64_t)t - a.x;
    st = st < 0 ? 0 : st > B - 1 ? B - 1 : st;
    uint32_t w = table[(int64_t)src * C * B + (int64_t)c * B + st];
    if (GAIN) w = __float_as_uint(__builtin_fmaf(__uint_as_float(w), __int_as_float(b.y), 0.0f));
    if (NOISE) {
        const uint2 k = *reinterpret_cast<const uint2*>(plan2 + prow * GOALNET_PLAN2_WORDS + 8);
        const uint64_t nkey = (uint64_t)k.x | ((uint64_t)k.y << 32);
        const float nz = n_lo + __builtin_fmaf(n_span, unit_of(nkey, (uint32_t)(c * B + t)), 0.0f);
        w = __float_as_uint(__uint_as_float(w) + nz);
    }
    return w;
}

template <bool GAIN, bool NOISE, bool MIX>
__global__ __launch_bounds__(256) void audio_gather_aug_kernel(const uint32_t* __restrict__ table, int64_t table_rows, uint32_t* __restrict__ out,
                                                               const int32_t* __restrict__ plan, const int32_t* __restrict__ plan2, int plan_rows,
                                                               int C, int B, int nrows, const int64_t* __restrict__ cursor, int64_t cursor_bias,
                                                               float n_lo, float n_span) {
    const int64_t base = *cursor + cursor_bias;
    const int CB = C * B;
    const int64_t total = (int64_t)nrows * CB;
    for (int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; e < total; e += (int64_t)gridDim.x * blockDim.x) {
        const int i = (int)(e / CB);
        const int rem = (int)(e - (int64_t)i * CB);
        const int64_t prow = base + i;
        if (prow < 0 || prow >= plan_rows) continue;
        const int src = plan[prow * GOALNET_PLAN_WORDS];
        if (src < 0 || src >= table_rows) continue;
        const int c = rem / B, t = rem - c * B;
        uint32_t w = audio_word<GAIN, NOISE>(table, plan2, prow, src, C, B, c, t, n_lo, n_span);
        if (MIX) {
            const int2 pl = *reinterpret_cast<const int2*>(plan2 + prow * GOALNET_PLAN2_WORDS + 6);        // partner, lambda
            if ((uint32_t)pl.y != ONE_BITS) {
                const int64_t q = pl.x;
                if (q < 0 || q >= plan_rows) continue;
                const int qsrc = plan[q * GOALNET_PLAN_WORDS];
                if (qsrc < 0 || qsrc >= table_rows) continue;
                w = mix_words(w, audio_word<GAIN, NOISE>(table, plan2, q, qsrc, C, B, c, t, n_lo, n_span), __int_as_float(pl.y));
            }
        }
        out[e] = w;
    }
}

// goalnet_frames_gather_aug's value for plan row `prow` (in range) with words {src, flip, dx, dy} = p, src in range, at (c, y, x)
template <bool COLOUR>
__device__ __forceinline__ uint32_t frame_word(const uint32_t* __restrict__ table, const int32_t* __restrict__ plan, int64_t prow, int4 p, int CHW,
                                               int HW, int H, int W, int c, int y, int x) {
    // 64-bit: |dx|, |dy| <= 32767 by the plan's contract, but a plan is caller memory
    int64_t sy = (int64_t)y - p.w, sx = (int64_t)(p.y ? W - 1 - x : x) - p.z;
    sy = sy < 0 ? 0 : sy > H - 1 ? H - 1 : sy;
    sx = sx < 0 ? 0 : sx > W - 1 ? W - 1 : sx;
    const uint32_t v = table[(int64_t)p.x * CHW + (int64_t)c * HW + sy * W + sx];
    if (COLOUR) {
        const int2 gb = *reinterpret_cast<const int2*>(plan + prow * GOALNET_PLAN_WORDS + 4);
        const float t = __builtin_fmaf(__uint_as_float(v), __int_as_float(gb.x), 0.0f) + __int_as_float(gb.y);
        return __float_as_uint(fminf(fmaxf(t, 0.0f), 1.0f));
    }
    return v;
}

template <bool COLOUR>
__global__ __launch_bounds__(256) void frames_gather_mix_kernel(const uint32_t* __restrict__ table, int64_t table_rows, uint32_t* __restrict__ out,
                                                                const int32_t* __restrict__ plan, const int32_t* __restrict__ plan2, int plan_rows,
                                                                int C, int H, int W, int nrows, const int64_t* __restrict__ cursor,
                                                                int64_t cursor_bias) {
    const int64_t base = *cursor + cursor_bias;
    const int HW = H * W, CHW = C * HW;
    const int64_t total = (int64_t)nrows * CHW;
    for (int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; e < total; e += (int64_t)gridDim.x * blockDim.x) {
        const int i = (int)(e / CHW);
        const int rem = (int)(e - (int64_t)i * CHW);
        const int64_t prow = base + i;
        if (prow < 0 || prow >= plan_rows) continue;
        const int4 p = *reinterpret_cast<const int4*>(plan + prow * GOALNET_PLAN_WORDS);       // src, flip, dx, dy
        if (p.x < 0 || p.x >= table_rows) continue;
        const int c = rem / HW, yx = rem - c * HW, y = yx / W, x = yx - y * W;
        uint32_t w = frame_word<COLOUR>(table, plan, prow, p, CHW, HW, H, W, c, y, x);
        const int2 pl = *reinterpret_cast<const int2*>(plan2 + prow * GOALNET_PLAN2_WORDS + 6);            // partner, lambda
        if ((uint32_t)pl.y != ONE_BITS) {
            const int64_t q = pl.x;
            if (q < 0 || q >= plan_rows) continue;
            const int4 pq = *reinterpret_cast<const int4*>(plan + q * GOALNET_PLAN_WORDS);
            if (pq.x < 0 || pq.x >= table_rows) continue;
            w = mix_words(w, frame_word<COLOUR>(table, plan, q, pq, CHW, HW, H, W, c, y, x), __int_as_float(pl.y));
        }
        out[e] = w;
    }
}

struct RowMixes { goalnet_rowmix seg[GOALNET_ROWCOPY_MAX]; };

// blockIdx.y selects the segment
__global__ __launch_bounds__(256) void rows_mix_indexed_kernel(RowMixes rm, const int32_t* __restrict__ plan, const int32_t* __restrict__ plan2,
                                                               int plan_rows) {
    const goalnet_rowmix sg = rm.seg[blockIdx.y];
    const int64_t words = sg.row_elems * sg.nrows, base = *sg.cursor + sg.cursor_bias;
    const uint32_t* s = (const uint32_t*)sg.table;
    uint32_t* d = (uint32_t*)sg.dst;
    for (int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; e < words; e += (int64_t)gridDim.x * blockDim.x) {
        const int64_t i = e / sg.row_elems, k = e - i * sg.row_elems;
        const int64_t prow = base + i;
        if (prow < 0 || prow >= plan_rows) continue;
        const int64_t src = plan[prow * GOALNET_PLAN_WORDS];
        if (src < 0 || src >= sg.table_rows) continue;
        uint32_t w = s[src * sg.row_elems + k];
        const int2 pl = *reinterpret_cast<const int2*>(plan2 + prow * GOALNET_PLAN2_WORDS + 6);            // partner, lambda
        if ((uint32_t)pl.y != ONE_BITS) {
            const int64_t q = pl.x;
            if (q < 0 || q >= plan_rows) continue;
            const int64_t qsrc = plan[q * GOALNET_PLAN_WORDS];
            if (qsrc < 0 || qsrc >= sg.table_rows) continue;
            w = mix_words(w, s[qsrc * sg.row_elems + k], __int_as_float(pl.y));
        }
        d[e] = w;
    }
}

unsigned blocks_for(int64_t n, int cap) {
    int64_t b = (n + 255) / 256;
    if (b > cap) b = cap;
    if (b < 1) b = 1;
    return (unsigned)b;
}

template <bool GAIN, bool NOISE>
void launch_audio(bool mix, dim3 grid, hipStream_t st, const uint32_t* table, int64_t table_rows, uint32_t* out, const int32_t* plan,
                  const int32_t* plan2, int plan_rows, int C, int B, int nrows, const int64_t* cursor, int64_t cursor_bias, float n_lo, float n_span) {
    if (mix)
        hipLaunchKernelGGL((audio_gather_aug_kernel<GAIN, NOISE, true>), grid, dim3(256), 0, st, table, table_rows, out, plan, plan2, plan_rows, C, B,
                           nrows, cursor, cursor_bias, n_lo, n_span);
    else
        hipLaunchKernelGGL((audio_gather_aug_kernel<GAIN, NOISE, false>), grid, dim3(256), 0, st, table, table_rows, out, plan, plan2, plan_rows, C, B,
                           nrows, cursor, cursor_bias, n_lo, n_span);
}

}  // namespace

extern "C" {

int goalnet_epoch_plan2(int32_t* plan2, const int32_t* plan, int n, uint64_t seed, uint32_t index, int C, int B, int max_shift,
                        int time_mask, int coeff_mask, float gain, float noise, float strength, float p, void* stream) {
    GN_REQUIRE(plan2 && plan, GOALNET_E_NULL, "epoch_plan2: null pointer");
    GN_REQUIRE(aligned16(plan2) && aligned16(plan), GOALNET_E_ALIGN, "epoch_plan2: both plans must be 16-byte aligned");
    GN_REQUIRE(n >= 1 && n <= GOALNET_EPOCH_MAX_N, GOALNET_E_SHAPE, "epoch_plan2: 1 <= n <= %d", GOALNET_EPOCH_MAX_N);
    GN_REQUIRE(C >= 1 && B >= 1 && (int64_t)C * B < (1ll << 31), GOALNET_E_SHAPE, "epoch_plan2: C >= 1, B >= 1, C * B < 2^31");
    GN_REQUIRE(max_shift >= 0 && max_shift <= GOALNET_MAX_SHIFT, GOALNET_E_VALUE, "epoch_plan2: 0 <= max_shift <= %d", GOALNET_MAX_SHIFT);
    GN_REQUIRE(time_mask >= 0 && time_mask <= B, GOALNET_E_VALUE, "epoch_plan2: 0 <= time_mask <= B");
    GN_REQUIRE(coeff_mask >= 0 && coeff_mask <= C - 1, GOALNET_E_VALUE, "epoch_plan2: 0 <= coeff_mask <= C - 1");
    GN_REQUIRE(gain >= 0.f && gain < 1.f, GOALNET_E_VALUE, "epoch_plan2: 0 <= gain < 1");
    GN_REQUIRE(noise >= 0.f && isfinite(noise), GOALNET_E_VALUE, "epoch_plan2: 0 <= noise, finite");
    GN_REQUIRE(strength >= 0.f && strength <= 1.f, GOALNET_E_VALUE, "epoch_plan2: 0 <= strength <= 1");
    GN_REQUIRE(p >= 0.f && p <= 1.f, GOALNET_E_VALUE, "epoch_plan2: 0 <= p <= 1");
    GN_REQUIRE(index < (uint32_t)GOALNET_PLAN2_MAX_INDEX, GOALNET_E_VALUE, "epoch_plan2: index < 2^26");
    Plan2Keys keys;
    for (uint32_t k = 0; k < 10; ++k) keys.k[k] = stream_key(seed, (uint32_t)GOALNET_TID_PLAN2 + 16u * index + k);
    const float g_lo = 1.0f - gain, g_hi = 1.0f + gain, l_lo = 1.0f - strength;
    hipLaunchKernelGGL(epoch_plan2_kernel, dim3(blocks_for(n, 256)), dim3(256), 0, (hipStream_t)stream, plan2, plan, n, keys, C, B, max_shift,
                       time_mask, coeff_mask, g_lo, g_hi - g_lo, gain > 0.f ? 1 : 0, noise > 0.f ? 1 : 0, l_lo, 1.0f - l_lo, p,
                       strength > 0.f && p > 0.f ? 1 : 0);
    GN_LAUNCH_CHECK("epoch_plan2");
    return 0;
}

int goalnet_audio_gather_aug(const float* table, int64_t table_rows, float* out, const int32_t* plan, const int32_t* plan2,
                             int plan_rows, int C, int B, int nrows, const int64_t* cursor, int64_t cursor_bias, int flags,
                             float noise, void* stream) {
    GN_REQUIRE(table && out && plan && plan2 && cursor, GOALNET_E_NULL, "audio_gather_aug: null pointer");
    GN_REQUIRE(aligned16(plan) && aligned16(plan2), GOALNET_E_ALIGN, "audio_gather_aug: both plans must be 16-byte aligned");
    GN_REQUIRE(C >= 1 && B >= 1 && nrows >= 1 && table_rows >= 1 && plan_rows >= 1 && (int64_t)C * B < (1ll << 31), GOALNET_E_SHAPE,
               "audio_gather_aug: positive dims, C * B < 2^31");
    GN_REQUIRE((flags & ~(GOALNET_AUDIO_GAIN | GOALNET_AUDIO_NOISE | GOALNET_AUDIO_MIX)) == 0, GOALNET_E_VALUE, "audio_gather_aug: unknown flag");
    GN_REQUIRE(noise >= 0.f && isfinite(noise), GOALNET_E_VALUE, "audio_gather_aug: 0 <= noise, finite");
    const dim3 grid(blocks_for((int64_t)nrows * C * B, 2048));
    const float n_lo = -noise, n_span = noise - n_lo;
    const bool mix = flags & GOALNET_AUDIO_MIX;
    const uint32_t* t = (const uint32_t*)table;
    uint32_t* o = (uint32_t*)out;
    hipStream_t st = (hipStream_t)stream;
    switch (flags & (GOALNET_AUDIO_GAIN | GOALNET_AUDIO_NOISE)) {
        case 0: launch_audio<false, false>(mix, grid, st, t, table_rows, o, plan, plan2, plan_rows, C, B, nrows, cursor, cursor_bias, n_lo, n_span); break;
        case GOALNET_AUDIO_GAIN: launch_audio<true, false>(mix, grid, st, t, table_rows, o, plan, plan2, plan_rows, C, B, nrows, cursor, cursor_bias, n_lo, n_span); break;
        case GOALNET_AUDIO_NOISE: launch_audio<false, true>(mix, grid, st, t, table_rows, o, plan, plan2, plan_rows, C, B, nrows, cursor, cursor_bias, n_lo, n_span); break;
        default: launch_audio<true, true>(mix, grid, st, t, table_rows, o, plan, plan2, plan_rows, C, B, nrows, cursor, cursor_bias, n_lo, n_span); break;
    }
    GN_LAUNCH_CHECK("audio_gather_aug");
    return 0;
}

int goalnet_frames_gather_mix(const float* table, int64_t table_rows, float* out, const int32_t* plan, const int32_t* plan2,
                              int plan_rows, int C, int H, int W, int nrows, const int64_t* cursor, int64_t cursor_bias, int colour,
                              void* stream) {
    GN_REQUIRE(table && out && plan && plan2 && cursor, GOALNET_E_NULL, "frames_gather_mix: null pointer");
    GN_REQUIRE(aligned16(plan) && aligned16(plan2), GOALNET_E_ALIGN, "frames_gather_mix: both plans must be 16-byte aligned");
    GN_REQUIRE(C >= 1 && H >= 1 && W >= 1 && nrows >= 1 && table_rows >= 1 && plan_rows >= 1 && (int64_t)C * H * W < (1ll << 31),
               GOALNET_E_SHAPE, "frames_gather_mix: positive dims, C * H * W < 2^31");
    const dim3 grid(blocks_for((int64_t)nrows * C * H * W, 4096)), block(256);
    if (colour)
        hipLaunchKernelGGL(frames_gather_mix_kernel<true>, grid, block, 0, (hipStream_t)stream, (const uint32_t*)table, table_rows, (uint32_t*)out,
                           plan, plan2, plan_rows, C, H, W, nrows, cursor, cursor_bias);
    else
        hipLaunchKernelGGL(frames_gather_mix_kernel<false>, grid, block, 0, (hipStream_t)stream, (const uint32_t*)table, table_rows, (uint32_t*)out,
                           plan, plan2, plan_rows, C, H, W, nrows, cursor, cursor_bias);
    GN_LAUNCH_CHECK("frames_gather_mix");
    return 0;
}

int goalnet_rows_mix_indexed(const goalnet_rowmix* segs, int count, const int32_t* plan, const int32_t* plan2, int plan_rows,
                             void* stream) {
    GN_REQUIRE(segs && plan && plan2, GOALNET_E_NULL, "rows_mix_indexed: null pointer");
    GN_REQUIRE(aligned16(plan) && aligned16(plan2), GOALNET_E_ALIGN, "rows_mix_indexed: both plans must be 16-byte aligned");
    GN_REQUIRE(count >= 1 && count <= GOALNET_ROWCOPY_MAX, GOALNET_E_SHAPE, "rows_mix_indexed: 1..%d segments", GOALNET_ROWCOPY_MAX);
    GN_REQUIRE(plan_rows >= 1, GOALNET_E_SHAPE, "rows_mix_indexed: an empty plan");
    RowMixes rm;
    int64_t most = 0;
    for (int i = 0; i < count; ++i) {
        const goalnet_rowmix& g = segs[i];
        GN_REQUIRE(g.table && g.dst && g.cursor, GOALNET_E_NULL, "rows_mix_indexed: null pointer in segment %d", i);
        GN_REQUIRE(g.row_elems >= 1 && g.row_elems < (1ll << 31) && g.nrows >= 1 && g.table_rows >= 1, GOALNET_E_SHAPE,
                   "rows_mix_indexed: segment %d: rows of 1 .. 2^31 - 1 elements, at least one row, the table not empty", i);
        rm.seg[i] = g;
        const int64_t words = g.row_elems * g.nrows;
        if (words > most) most = words;
    }
    hipLaunchKernelGGL(rows_mix_indexed_kernel, dim3(blocks_for(most, 2048), (unsigned)count), dim3(256), 0, (hipStream_t)stream, rm, plan, plan2,
                       plan_rows);
    GN_LAUNCH_CHECK("rows_mix_indexed");
    return 0;
}

}  // extern "C"
