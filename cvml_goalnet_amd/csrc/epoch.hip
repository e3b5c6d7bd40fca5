// A shuffled, augmented pass over a video resident on the device (include/goalnet_epoch.h; EXTENSION, no reference code):
// the plan of one pass (frame order + per-frame augmentation draws), the gather that applies it to the frames, and the row copies
// that take labels / audio / weights and predictions through the same order. Everything here is integer or non-contracted fp32,
// element-wise in the source frame: any launch geometry gives the bits of tests/_augment_ref.py.
#include "common.h"
#include "rng.h"
#include "../../include/goalnet_epoch.h"

#include <math.h>

using namespace goalnet;

namespace {

constexpr int PLAN_TILE = 256;      // keys per LDS tile = threads per block

__device__ __forceinline__ uint64_t stream_bits(uint64_t key, uint32_t r) {
    return mix64(key + (uint64_t)(r + 1u) * 0x9E3779B97F4A7C15ull);      // rng.h: element r of the stream
}
__device__ __forceinline__ uint64_t sort_key(uint64_t key, uint32_t r) { return (stream_bits(key, r) & ~0xFFFFFFull) | r; }

struct PlanKeys { uint64_t k[6]; };

// one thread per source frame r: its position in the order (rank by counting over LDS tiles of keys) and its own draws
__global__ __launch_bounds__(PLAN_TILE) void epoch_plan_kernel(int32_t* __restrict__ plan, int n, PlanKeys keys, int shuffle, float flip_p,
                                                               int max_shift, float g_lo, float g_span, int contrast_on, float b_lo,
                                                               float b_span, int brightness_on) {
    __shared__ uint64_t tile[PLAN_TILE];
    for (int r0 = blockIdx.x * PLAN_TILE; r0 < n; r0 += gridDim.x * PLAN_TILE) {      // block-uniform: every thread meets the barriers
        const int r = r0 + threadIdx.x;
        const bool live = r < n;
        int pos = r;
        if (shuffle) {
            const uint64_t mine = sort_key(keys.k[0], (uint32_t)r);
            pos = 0;
            for (int s0 = 0; s0 < n; s0 += PLAN_TILE) {
                const int s = s0 + threadIdx.x;
                __syncthreads();
                tile[threadIdx.x] = s < n ? sort_key(keys.k[0], (uint32_t)s) : ~0ull;      // all ones: above every real key
                __syncthreads();
#pragma unroll 8
                for (int j = 0; j < PLAN_TILE; ++j) pos += tile[j] < mine ? 1 : 0;
            }
        }
        if (!live) continue;
        int flip = 0, dx = 0, dy = 0;
        float gain = 1.0f, bias = 0.0f;
        if (flip_p > 0.f) flip = (float)(uint32_t)(stream_bits(keys.k[1], r) >> 40) * 5.9604644775390625e-08f < flip_p ? 1 : 0;
        if (max_shift > 0) {
            const uint64_t width = 2ull * (uint64_t)max_shift + 1ull;
            dx = (int)(((stream_bits(keys.k[2], r) >> 40) * width) >> 24) - max_shift;
            dy = (int)(((stream_bits(keys.k[3], r) >> 40) * width) >> 24) - max_shift;
        }
        // fma(span, u, 0) is the rounded product and cannot be contracted with the add (fill.hip)
        if (contrast_on) gain = g_lo + __builtin_fmaf(g_span, (float)(uint32_t)(stream_bits(keys.k[4], r) >> 40) * 5.9604644775390625e-08f, 0.0f);
        if (brightness_on) bias = b_lo + __builtin_fmaf(b_span, (float)(uint32_t)(stream_bits(keys.k[5], r) >> 40) * 5.9604644775390625e-08f, 0.0f);
        int4* row = reinterpret_cast<int4*>(plan + (int64_t)pos * GOALNET_PLAN_WORDS);
        row[0] = make_int4(r, flip, dx, dy);
        row[1] = make_int4(__float_as_int(gain), __float_as_int(bias), 0, 0);
    }
}

template <bool COLOUR>
__global__ __launch_bounds__(256) void frames_gather_aug_kernel(const uint32_t* __restrict__ table, int64_t table_rows, uint32_t* __restrict__ out,
                                                                const int32_t* __restrict__ plan, int plan_rows, int C, int H, int W, int nrows,
                                                                const int64_t* __restrict__ cursor, int64_t cursor_bias) {
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
        // 64-bit: |dx|, |dy| <= 32767 by the plan's contract, but a plan is caller memory
        int64_t sy = (int64_t)y - p.w, sx = (int64_t)(p.y ? W - 1 - x : x) - p.z;
        sy = sy < 0 ? 0 : sy > H - 1 ? H - 1 : sy;
        sx = sx < 0 ? 0 : sx > W - 1 ? W - 1 : sx;
        const uint32_t v = table[(int64_t)p.x * CHW + (int64_t)c * HW + sy * W + sx];
        if (COLOUR) {
            const int2 gb = *reinterpret_cast<const int2*>(plan + prow * GOALNET_PLAN_WORDS + 4);
            const float t = __builtin_fmaf(__uint_as_float(v), __int_as_float(gb.x), 0.0f) + __int_as_float(gb.y);
            out[e] = __float_as_uint(fminf(fmaxf(t, 0.0f), 1.0f));
        } else {
            out[e] = v;
        }
    }
}

struct IndexedCopies { goalnet_rowcopy_indexed seg[GOALNET_ROWCOPY_MAX]; };

// blockIdx.y selects the segment
__global__ __launch_bounds__(256) void rows_copy_indexed_kernel(IndexedCopies rc, const int32_t* __restrict__ plan, int plan_rows) {
    const goalnet_rowcopy_indexed sg = rc.seg[blockIdx.y];
    const int64_t row_words = sg.row_bytes / 4, words = row_words * sg.nrows, base = *sg.cursor + sg.cursor_bias;
    const uint32_t* s = (const uint32_t*)sg.src;
    uint32_t* d = (uint32_t*)sg.dst;
    for (int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; e < words; e += (int64_t)gridDim.x * blockDim.x) {
        const int64_t i = e / row_words, w = e - i * row_words;
        int64_t t = base + i;                                   // the row on the table side
        if (sg.indexed) {
            if (t < 0 || t >= plan_rows) continue;
            t = plan[t * GOALNET_PLAN_WORDS];
        }
        if (t < 0 || t >= sg.table_rows) continue;
        if (sg.gather) d[e] = s[t * row_words + w];
        else d[t * row_words + w] = s[e];
    }
}

unsigned blocks_for(int64_t n, int cap) {
    int64_t b = (n + 255) / 256;
    if (b > cap) b = cap;
    if (b < 1) b = 1;
    return (unsigned)b;
}

}  // namespace

extern "C" {

int goalnet_epoch_plan(int32_t* plan, int n, uint64_t seed, uint32_t index, int shuffle, float flip_p, int max_shift,
                       float contrast, float brightness, void* stream) {
    GN_REQUIRE(plan, GOALNET_E_NULL, "epoch_plan: null pointer");
    GN_REQUIRE(aligned16(plan), GOALNET_E_ALIGN, "epoch_plan: the plan must be 16-byte aligned");
    GN_REQUIRE(n >= 1 && n <= GOALNET_EPOCH_MAX_N, GOALNET_E_SHAPE, "epoch_plan: 1 <= n <= %d", GOALNET_EPOCH_MAX_N);
    GN_REQUIRE(max_shift >= 0 && max_shift <= GOALNET_MAX_SHIFT, GOALNET_E_VALUE, "epoch_plan: 0 <= max_shift <= %d", GOALNET_MAX_SHIFT);
    GN_REQUIRE(flip_p >= 0.f && flip_p <= 1.f, GOALNET_E_VALUE, "epoch_plan: 0 <= flip_p <= 1");
    GN_REQUIRE(contrast >= 0.f && contrast < 1.f, GOALNET_E_VALUE, "epoch_plan: 0 <= contrast < 1");
    GN_REQUIRE(brightness >= 0.f && isfinite(brightness), GOALNET_E_VALUE, "epoch_plan: 0 <= brightness, finite");
    GN_REQUIRE(index < (1u << 28), GOALNET_E_VALUE, "epoch_plan: index < 2^28");
    PlanKeys keys;
    for (uint32_t k = 0; k < 6; ++k) keys.k[k] = stream_key(seed, (uint32_t)GOALNET_TID_PLAN + 8u * index + k);
    const float g_lo = 1.0f - contrast, g_hi = 1.0f + contrast, b_lo = -brightness;
    hipLaunchKernelGGL(epoch_plan_kernel, dim3((unsigned)((n + PLAN_TILE - 1) / PLAN_TILE)), dim3(PLAN_TILE), 0, (hipStream_t)stream, plan, n,
                       keys, shuffle ? 1 : 0, flip_p, max_shift, g_lo, g_hi - g_lo, contrast > 0.f ? 1 : 0, b_lo, brightness - b_lo,
                       brightness > 0.f ? 1 : 0);
    GN_LAUNCH_CHECK("epoch_plan");
    return 0;
}

int goalnet_frames_gather_aug(const float* table, int64_t table_rows, float* out, const int32_t* plan, int plan_rows,
                              int C, int H, int W, int nrows, const int64_t* cursor, int64_t cursor_bias, int colour, void* stream) {
    GN_REQUIRE(table && out && plan && cursor, GOALNET_E_NULL, "frames_gather_aug: null pointer");
    GN_REQUIRE(aligned16(plan), GOALNET_E_ALIGN, "frames_gather_aug: the plan must be 16-byte aligned");
    GN_REQUIRE(C >= 1 && H >= 1 && W >= 1 && nrows >= 1 && table_rows >= 1 && plan_rows >= 1 && (int64_t)C * H * W < (1ll << 31),
               GOALNET_E_SHAPE, "frames_gather_aug: positive dims, C * H * W < 2^31");
    const int64_t total = (int64_t)nrows * C * H * W;
    const dim3 grid(blocks_for(total, 4096)), block(256);
    if (colour)
        hipLaunchKernelGGL(frames_gather_aug_kernel<true>, grid, block, 0, (hipStream_t)stream, (const uint32_t*)table, table_rows,
                           (uint32_t*)out, plan, plan_rows, C, H, W, nrows, cursor, cursor_bias);
    else
        hipLaunchKernelGGL(frames_gather_aug_kernel<false>, grid, block, 0, (hipStream_t)stream, (const uint32_t*)table, table_rows,
                           (uint32_t*)out, plan, plan_rows, C, H, W, nrows, cursor, cursor_bias);
    GN_LAUNCH_CHECK("frames_gather_aug");
    return 0;
}

int goalnet_rows_copy_indexed(const goalnet_rowcopy_indexed* segs, int count, const int32_t* plan, int plan_rows, void* stream) {
    GN_REQUIRE(segs && plan, GOALNET_E_NULL, "rows_copy_indexed: null pointer");
    GN_REQUIRE(count >= 1 && count <= GOALNET_ROWCOPY_MAX, GOALNET_E_SHAPE, "rows_copy_indexed: 1..%d segments", GOALNET_ROWCOPY_MAX);
    GN_REQUIRE(plan_rows >= 1, GOALNET_E_SHAPE, "rows_copy_indexed: an empty plan");
    IndexedCopies rc;
    int64_t most = 0;
    for (int i = 0; i < count; ++i) {
        const goalnet_rowcopy_indexed& g = segs[i];
        GN_REQUIRE(g.src && g.dst && g.cursor, GOALNET_E_NULL, "rows_copy_indexed: null pointer in segment %d", i);
        GN_REQUIRE(g.row_bytes > 0 && (g.row_bytes & 3) == 0 && g.nrows > 0 && g.table_rows >= 1, GOALNET_E_SHAPE,
                   "rows_copy_indexed: segment %d: rows must be a positive multiple of 4 bytes, the table not empty", i);
        rc.seg[i] = g;
        const int64_t words = g.row_bytes / 4 * g.nrows;
        if (words > most) most = words;
    }
    hipLaunchKernelGGL(rows_copy_indexed_kernel, dim3(blocks_for(most, 2048), (unsigned)count), dim3(256), 0, (hipStream_t)stream, rc, plan,
                       plan_rows);
    GN_LAUNCH_CHECK("rows_copy_indexed");
    return 0;
}

}  // extern "C"
