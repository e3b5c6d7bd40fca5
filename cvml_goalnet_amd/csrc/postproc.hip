// What the reference runs after the hot path for every video in every epoch, on the device:
//   importance rounding + expansion + per-clip sums   /root/reference/utils.py:608-613, 396-410, 445-463
//   0/1 knapsack over the clips                       /root/reference/utils.py:465-510, 633-635
//   summary mask                                      /root/reference/utils.py:637-641
//   F-score against the annotators                    /root/reference/utils.py:552-580
// Integer work, bit-exact with the reference's Python: int64 sums, the same DP recurrence and back-tracking rule, and
// the same sequence of IEEE double operations for precision / recall / F (one division, 2*p*r/(p+r), a running sum).
// Quirks kept: clip sums and weights use the end-exclusive slice [a:b), the mask the
// end-inclusive range [a, b]. The reference does this in pure Python (a 200 x 15 000 DP table of list-of-lists).
#include "common.h"

#include <cstdlib>

using namespace goalnet;

namespace {

// importance of raw frame f: torch.round (half to even) -> int8, then expand_array (repeat, truncate, pad with the last)
__device__ __forceinline__ int importance_at(const float* __restrict__ pred, int n_sampled, int skip, int full_n, int f) {
    int i = n_sampled == full_n ? f : f / skip;
    if (i >= n_sampled) i = n_sampled - 1;
    return (int)(signed char)(int)rintf(pred[i]);
}

// one block per clip: value = sum of importances over [a:b) clamped like a Python slice, length = len of that slice
__device__ __forceinline__ void clip_info_block(const float* __restrict__ pred, int n_sampled, int skip, int full_n,
                                                const int32_t* __restrict__ cps, int c, int64_t* __restrict__ values,
                                                int32_t* __restrict__ lengths) {
    __shared__ int64_t red[4];
    int a = cps[2 * c], b = cps[2 * c + 1];
    if (a < 0) a = a + full_n < 0 ? 0 : a + full_n;            // Python slice semantics: negative bounds count from the end
    if (b < 0) b = b + full_n < 0 ? 0 : b + full_n;
    a = a > full_n ? full_n : a;
    b = b > full_n ? full_n : b;
    const int len = b > a ? b - a : 0;
    int64_t s = 0;
    for (int f = a + threadIdx.x; f < a + len; f += 256) s += importance_at(pred, n_sampled, skip, full_n, f);
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) s += __shfl_xor(s, o, 64);
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = s;
    __syncthreads();
    if (threadIdx.x == 0) {
        values[c] = red[0] + red[1] + red[2] + red[3];
        lengths[c] = len;
    }
}

__global__ __launch_bounds__(256) void clip_info_kernel(const float* __restrict__ pred, int n_sampled, int skip, int full_n,
                                                       const int32_t* __restrict__ cps, int n_clips,
                                                       int64_t* __restrict__ values, int32_t* __restrict__ lengths) {
    clip_info_block(pred, n_sampled, skip, full_n, cps, blockIdx.x, values, lengths);
}

// the same for `batch` importance vectors of one video: grid (n_clips, batch), item b = row b of pred / values / lengths
__global__ __launch_bounds__(256) void clip_info_batch_kernel(const float* __restrict__ pred, int n_sampled, int skip, int full_n,
                                                             const int32_t* __restrict__ cps, int n_clips,
                                                             int64_t* __restrict__ values, int32_t* __restrict__ lengths) {
    const size_t b = blockIdx.y;
    clip_info_block(pred + b * n_sampled, n_sampled, skip, full_n, cps, blockIdx.x, values + b * n_clips, lengths + b * n_clips);
}

// K[i][w] of utils.py:480-491, one row per iteration, the row's columns spread over the block; then the back-tracking of
// utils.py:493-508 by thread 0. K: (n + 1) x (cap + 1) int64 in global memory (L2-resident: <= 24 MB).
__global__ __launch_bounds__(1024) void knapsack_kernel(const int64_t* __restrict__ values, const int32_t* __restrict__ lengths,
                                                       int weight_scale, const int32_t* __restrict__ weights_in, int n, int cap,
                                                       int64_t* __restrict__ K, int32_t* __restrict__ selected) {
    const int W = cap + 1;
    for (int w = threadIdx.x; w < W; w += 1024) K[w] = 0;
    for (int i = threadIdx.x; i < n; i += 1024) selected[i] = 0;
    __syncthreads();
    for (int i = 1; i <= n; ++i) {
        const int64_t v = values[i - 1];
        const int wt = weights_in ? weights_in[i - 1] : lengths[i - 1] * weight_scale;
        const int64_t* prev = K + (int64_t)(i - 1) * W;
        int64_t* cur = K + (int64_t)i * W;
        for (int w = threadIdx.x; w < W; w += 1024) {
            int64_t r = prev[w];
            if (w == 0) r = 0;
            else if (wt <= w) { const int64_t t = v + prev[w - wt]; r = t > r ? t : r; }
            cur[w] = r;
        }
        __syncthreads();
    }
    if (threadIdx.x == 0) {
        int64_t res = K[(int64_t)n * W + cap];
        int w = cap;
        for (int i = n; i > 0; --i) {
            if (res <= 0) break;
            if (res == K[(int64_t)(i - 1) * W + w]) continue;
            selected[i - 1] = 1;
            res -= values[i - 1];
            w -= weights_in ? weights_in[i - 1] : lengths[i - 1] * weight_scale;
        }
    }
}

// mask[a .. b] = 1 for the selected clips (end inclusive); a frame outside the video sets status (numpy: IndexError)
__device__ __forceinline__ void summary_mask_block(const int32_t* __restrict__ cps, const int32_t* __restrict__ selected, int c,
                                                   int full_n, uint8_t* __restrict__ mask, int32_t* __restrict__ status) {
    if (!selected[c]) return;
    const int a = cps[2 * c], b = cps[2 * c + 1];
    if (threadIdx.x == 0 && b >= a && (a < -full_n || b >= full_n)) atomicOr(status, 1);
    for (int f = a + threadIdx.x; f <= b; f += 256) {
        const int g = f < 0 ? f + full_n : f;                      // numpy wraps negative indices
        if (g >= 0 && g < full_n) mask[g] = 1;
    }
}

__global__ __launch_bounds__(256) void summary_mask_kernel(const int32_t* __restrict__ cps, const int32_t* __restrict__ selected,
                                                          int n_clips, int full_n, uint8_t* __restrict__ mask, int32_t* __restrict__ status) {
    summary_mask_block(cps, selected, blockIdx.x, full_n, mask, status);
}

// grid (n_clips, batch): item b writes row b of mask [batch][full_n] and status[b]
__global__ __launch_bounds__(256) void summary_mask_batch_kernel(const int32_t* __restrict__ cps, const int32_t* __restrict__ selected,
                                                                int n_clips, int full_n, uint8_t* __restrict__ mask,
                                                                int32_t* __restrict__ status) {
    const size_t b = blockIdx.y;
    summary_mask_block(cps, selected + b * n_clips, blockIdx.x, full_n, mask + b * full_n, status + b);
}

// counts[u] = {sum(S and G_u), sum(G_u)}; counts[n_users] = {sum(S), 0}
__device__ __forceinline__ void fscore_counts_block(const uint8_t* __restrict__ gd, const uint8_t* __restrict__ mask, int n_users,
                                                    int u, int full_n, int64_t* __restrict__ counts) {
    __shared__ int64_t red[4][2];
    int64_t ov = 0, sg = 0;
    if (u < n_users) {
        const uint8_t* g = gd + (int64_t)u * full_n;
        for (int f = threadIdx.x; f < full_n; f += 256) { const int gv = g[f]; ov += (gv != 0 && mask[f] != 0) ? 1 : 0; sg += gv; }
    } else {
        for (int f = threadIdx.x; f < full_n; f += 256) ov += mask[f];
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) { ov += __shfl_xor(ov, o, 64); sg += __shfl_xor(sg, o, 64); }
    if ((threadIdx.x & 63) == 0) { red[threadIdx.x >> 6][0] = ov; red[threadIdx.x >> 6][1] = sg; }
    __syncthreads();
    if (threadIdx.x == 0) {
        counts[2 * u] = red[0][0] + red[1][0] + red[2][0] + red[3][0];
        counts[2 * u + 1] = red[0][1] + red[1][1] + red[2][1] + red[3][1];
    }
}

__global__ __launch_bounds__(256) void fscore_counts_kernel(const uint8_t* __restrict__ gd, const uint8_t* __restrict__ mask, int n_users,
                                                           int full_n, int64_t* __restrict__ counts) {
    fscore_counts_block(gd, mask, n_users, blockIdx.x, full_n, counts);
}

// grid (n_users + 1, batch): the annotators of the one video against row b of mask; counts: [batch] blocks of `counts_stride` int64
__global__ __launch_bounds__(256) void fscore_counts_batch_kernel(const uint8_t* __restrict__ gd, const uint8_t* __restrict__ mask,
                                                                 int n_users, int full_n, int64_t* __restrict__ counts,
                                                                 size_t counts_stride) {
    const size_t b = blockIdx.y;
    fscore_counts_block(gd, mask + b * full_n, n_users, blockIdx.x, full_n, counts + b * counts_stride);
}

// utils.py:566-580 in the reference's order of double operations
__device__ __forceinline__ void fscore_final_item(const int64_t* __restrict__ counts, int n_users, double* __restrict__ out) {
    const int64_t s_sum = counts[2 * n_users];
    double total = 0.0, best = 0.0;
    for (int u = 0; u < n_users; ++u) {
        const int64_t ov = counts[2 * u], g_sum = counts[2 * u + 1];
        const double precision = s_sum != 0 ? (double)ov / (double)s_sum : 0.0;
        const double recall = g_sum != 0 ? (double)ov / (double)g_sum : 0.0;
        const double pr = precision + recall;
        const double f = pr != 0.0 ? 2.0 * precision * recall / pr : 0.0;
        total += f;
        best = (u == 0 || f > best) ? f : best;
    }
    out[0] = total / (double)n_users;
    out[1] = best;
}

__global__ void fscore_final_kernel(const int64_t* __restrict__ counts, int n_users, double* __restrict__ out) {
    fscore_final_item(counts, n_users, out);
}

// one thread per item: fscore [batch][2]
__global__ __launch_bounds__(64) void fscore_final_batch_kernel(const int64_t* __restrict__ counts, size_t counts_stride, int n_users,
                                                               int batch, double* __restrict__ out) {
    const int b = blockIdx.x * 64 + threadIdx.x;
    if (b < batch) fscore_final_item(counts + (size_t)b * counts_stride, n_users, out + 2 * (size_t)b);
}

// ---- the batched knapsack: `batch` independent instances of utils.py:465-510, one 1024-thread block (one CU) each ----
// knapsack_kernel above keeps the whole (n + 1) x (cap + 1) int64 table K in global memory (24 MB at 200 clips x 15 001
// columns). Twenty of them would be 480 MB, past the L2. Here only the CURRENT row lives on chip and global memory holds
// one decision bit per cell,
//     bit(i, w) = (K[i][w] != K[i-1][w]),        i = 1 .. n, w = 0 .. cap,        n * ceil((cap + 1) / 64) words,
// which is all the back-tracking of utils.py:495-508 reads. Why that loop can be replayed from the bits alone:
//   * At the top of its iteration i the loop holds res == K[i][w]. True at the start (res = K[n][cap], w = cap). If
//     res == K[i-1][w] it `continue`s and the statement holds for i - 1. Otherwise K[i][w] != K[i-1][w], so the table took the
//     branch K[i][w] = values[i-1] + K[i-1][w - weights[i-1]] (utils.py:490), and after res -= value, w -= weight again
//     res == K[i-1][w]. Hence `res == K[i-1][w]` is exactly bit(i, w) == 0, and an item is selected exactly where the bit is set.
//   * K is non-negative (row 0 is zero and K[i][w] >= K[i-1][w]) and non-decreasing in i and in w. So `res <= 0` means
//     K[i][w] == 0, hence K[j][w'] == 0 for every j <= i, w' <= w: every bit the loop could still visit is 0 and it would select
//     nothing more. Leaving at the `break` and walking on to i = 0 give the same list.
// The walk is therefore: for i = n .. 1: if bit(i, w) { select i-1; w -= weight[i-1] }. One wavefront runs it, 64 rows per
// step: lane l tests bit(i - l, w), the first set lane is the next selected item, everything before it was a `continue`.
//
// Variant "lds" (cap + 1 <= KB_LDS_MAX_COLS): column w = c * 1024 + tid of the row sits in register r[c] of thread tid and the
// row is mirrored in LDS for the shifted read prev[w - wt]. Per item: read the old row from LDS, update the registers,
// ballot the decision bits (64 consecutive columns per wavefront = one word), barrier, write the changed columns back,
// barrier. (cap + 1) * 8 bytes of dynamic LDS: 120 KB at 15 001 columns, 160 000 B at the limit of 20 000 (160 KiB per CU).
// Variant "rolling" (wider rows): two rows per item in the workspace, same bits, one barrier per item row.
constexpr int KB_THREADS = 1024;
constexpr int KB_LDS_MAX_COLS = 20000;

__device__ __forceinline__ void knapsack_backtrack_bits(const uint64_t* __restrict__ bits, int words_per_row,
                                                        const int32_t* __restrict__ lengths, int weight_scale, int n, int cap,
                                                        int32_t* __restrict__ selected) {
    const int lane = threadIdx.x;                                  // called by the first wavefront only
    int w = cap, i = n;
    while (i > 0) {
        const int row = i - 1 - lane;
        const bool set = row >= 0 && ((bits[(size_t)row * words_per_row + (w >> 6)] >> (w & 63)) & 1ull);
        const unsigned long long m = __ballot(set);
        if (m == 0) { i -= 64; continue; }
        const int item = i - 1 - (__ffsll(m) - 1);
        if (lane == 0) selected[item] = 1;
        w -= lengths[item] * weight_scale;
        i = item;
    }
}

template <int MAXC>
__global__ __launch_bounds__(KB_THREADS) void knapsack_batch_lds_kernel(const int64_t* __restrict__ values_all,
                                                                       const int32_t* __restrict__ lengths_all, int weight_scale,
                                                                       int n, int cap, uint64_t* __restrict__ bits_all,
                                                                       size_t bits_stride, int32_t* __restrict__ selected_all) {
    extern __shared__ int64_t kb_row[];
    const size_t b = blockIdx.x;
    const int64_t* values = values_all + b * n;
    const int32_t* lengths = lengths_all + b * n;
    int32_t* selected = selected_all + b * n;
    uint64_t* bits = bits_all + b * bits_stride;
    const int W = cap + 1, WW = (W + 63) >> 6, C = (W + KB_THREADS - 1) / KB_THREADS;
    const int tid = threadIdx.x;
    int64_t r[MAXC];
#pragma unroll
    for (int c = 0; c < MAXC; ++c) {
        r[c] = 0;
        const int w = c * KB_THREADS + tid;
        if (w < W) kb_row[w] = 0;
    }
    for (int i = tid; i < n; i += KB_THREADS) selected[i] = 0;
    int64_t v = values[0];
    int wt = lengths[0] * weight_scale;
    __syncthreads();
    for (int i = 0; i < n; ++i) {
        const int64_t v_next = i + 1 < n ? values[i + 1] : 0;      // fetched a row ahead: off the barrier-to-barrier path
        const int wt_next = i + 1 < n ? lengths[i + 1] * weight_scale : 0;
        uint64_t* brow = bits + (size_t)i * WW;
        unsigned changed = 0;
#pragma unroll
        for (int c = 0; c < MAXC; ++c) {
            if (c < C) {                                           // uniform over the block
                const int w = c * KB_THREADS + tid;
                bool take = false;
                if (w < W && w > 0 && wt <= w) {                    // utils.py:487-490 (w == 0 stays 0)
                    const int64_t t = v + kb_row[w - wt];
                    if (t > r[c]) { r[c] = t; take = true; }
                }
                const unsigned long long m = __ballot(take);
                const int word = (c * KB_THREADS + (tid & ~63)) >> 6;
                if ((tid & 63) == 0 && word < WW) brow[word] = m;
                changed |= take ? 1u << c : 0u;
            }
        }
        __syncthreads();                                           // every read of row i-1 is done
#pragma unroll
        for (int c = 0; c < MAXC; ++c)
            if (changed & (1u << c)) kb_row[c * KB_THREADS + tid] = r[c];
        __syncthreads();
        v = v_next;
        wt = wt_next;
    }
    if (tid < 64) knapsack_backtrack_bits(bits, WW, lengths, weight_scale, n, cap, selected);
}

// rows: [batch][2][cap + 1] int64 in the workspace
__global__ __launch_bounds__(KB_THREADS) void knapsack_batch_rolling_kernel(const int64_t* __restrict__ values_all,
                                                                           const int32_t* __restrict__ lengths_all, int weight_scale,
                                                                           int n, int cap, uint64_t* __restrict__ bits_all,
                                                                           size_t bits_stride, int64_t* __restrict__ rows_all,
                                                                           int32_t* __restrict__ selected_all) {
    const size_t b = blockIdx.x;
    const int64_t* values = values_all + b * n;
    const int32_t* lengths = lengths_all + b * n;
    int32_t* selected = selected_all + b * n;
    uint64_t* bits = bits_all + b * bits_stride;
    const int W = cap + 1, WW = (W + 63) >> 6;
    int64_t* rows = rows_all + b * 2 * (size_t)W;
    const int tid = threadIdx.x;
    for (int w = tid; w < W; w += KB_THREADS) rows[w] = 0;
    for (int i = tid; i < n; i += KB_THREADS) selected[i] = 0;
    __syncthreads();
    for (int i = 0; i < n; ++i) {
        const int64_t v = values[i];
        const int wt = lengths[i] * weight_scale;
        const int64_t* prev = rows + (size_t)(i & 1) * W;
        int64_t* cur = rows + (size_t)((i + 1) & 1) * W;
        uint64_t* brow = bits + (size_t)i * WW;
        for (int w = tid; w < WW * 64; w += KB_THREADS) {          // whole wavefronts enter or leave together (ballot)
            bool take = false;
            if (w < W) {
                int64_t x = prev[w];
                if (w > 0 && wt <= w) {
                    const int64_t t = v + prev[w - wt];
                    if (t > x) { x = t; take = true; }
                }
                cur[w] = x;
            }
            const unsigned long long m = __ballot(take);
            if ((tid & 63) == 0) brow[w >> 6] = m;
        }
        __syncthreads();
    }
    if (tid < 64) knapsack_backtrack_bits(bits, WW, lengths, weight_scale, n, cap, selected);
}

bool kb_rolling(int capacity_scaled) {
    return capacity_scaled + 1 > KB_LDS_MAX_COLS || getenv("GOALNET_KNAPSACK_BATCH_ROLLING") != nullptr;   // the switch: A/B runs, tests
}

int kb_maxc(int capacity_scaled) {
    const int c = (capacity_scaled + 1 + KB_THREADS - 1) / KB_THREADS;
    return c <= 4 ? 4 : c <= 8 ? 8 : c <= 16 ? 16 : 20;
}

template <int MAXC>
hipError_t launch_knapsack_batch_lds(hipStream_t st, int batch, const int64_t* values, const int32_t* lengths, int weight_scale, int n,
                                     int cap, uint64_t* bits, size_t bits_stride, int32_t* selected) {
    const size_t lds = (size_t)(cap + 1) * sizeof(int64_t);
    if (lds > 64 * 1024) {                                          // past the default limit of dynamic LDS
        hipError_t e = hipFuncSetAttribute((const void*)knapsack_batch_lds_kernel<MAXC>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
        if (e != hipSuccess) return e;
    }
    hipLaunchKernelGGL(knapsack_batch_lds_kernel<MAXC>, dim3(batch), dim3(KB_THREADS), lds, st, values, lengths, weight_scale, n, cap, bits,
                       bits_stride, selected);
    return hipGetLastError();
}

// get_annotations, utils.py:382-394: labels_full[f] = np.round(np.mean(scores[:, f])) in float32, one thread per frame.
// np.mean of a 1-D float32 array = numpy's pairwise sum (then one division by the count, correctly rounded):
//   n < 8:   ((a0 + a1) + a2) + ...            8 <= n <= 128: eight running sums r[j] += a[8k + j] over the whole groups of 8,
//   ((r0 + r1) + (r2 + r3)) + ((r4 + r5) + (r6 + r7)), then the n % 8 trailing elements added one by one.
// (Past 128 elements numpy splits recursively; the entry point takes up to 128 annotators.)
__global__ __launch_bounds__(256) void mean_annotations_kernel(const float* __restrict__ scores, int n_annot, int full_n, int skip,
                                                              float* __restrict__ trimmed, float* __restrict__ full) {
    const int f = blockIdx.x * 256 + threadIdx.x;
    if (f >= full_n) return;
    const float* a = scores + f;
    const size_t s = (size_t)full_n;
    float res;
    if (n_annot < 8) {
        res = 0.0f;
        for (int i = 0; i < n_annot; ++i) res += a[i * s];
    } else {
        float r[8];
#pragma unroll
        for (int j = 0; j < 8; ++j) r[j] = a[j * s];
        int i = 8;
        for (; i < n_annot - (n_annot % 8); i += 8) {
#pragma unroll
            for (int j = 0; j < 8; ++j) r[j] += a[(i + j) * s];
        }
        res = ((r[0] + r[1]) + (r[2] + r[3])) + ((r[4] + r[5]) + (r[6] + r[7]));
        for (; i < n_annot; ++i) res += a[i * s];
    }
    // a float32 quotient through double is the correctly rounded float32 quotient (53 >= 2 * 24 + 2 bits)
    const float mean = (float)((double)res / (double)n_annot);
    const float lab = rintf(mean);                                 // np.round: half to even
    full[f] = lab;
    if (f % skip == 0) trimmed[f / skip] = lab;
}

size_t align256(size_t b) { return (b + 255) / 256 * 256; }

}  // namespace

extern "C" {

size_t goalnet_knapsack_ws_bytes(int n_items, int capacity_scaled) {
    if (n_items < 0 || capacity_scaled < 0) return 0;
    return align256((size_t)(n_items + 1) * (size_t)(capacity_scaled + 1) * sizeof(int64_t));
}

int goalnet_knapsack(const int64_t* values, const int32_t* weights_scaled, int n_items, int capacity_scaled,
                     int32_t* selected, void* ws, size_t ws_bytes, void* stream) {
    GN_REQUIRE(values && weights_scaled && selected && ws, GOALNET_E_NULL, "knapsack: null pointer");
    GN_REQUIRE(n_items >= 1 && capacity_scaled >= 0, GOALNET_E_SHAPE, "knapsack: need n_items >= 1, capacity >= 0");
    GN_REQUIRE(ws_bytes >= goalnet_knapsack_ws_bytes(n_items, capacity_scaled), GOALNET_E_WORKSPACE, "knapsack: workspace too small");
    hipLaunchKernelGGL(knapsack_kernel, dim3(1), dim3(1024), 0, (hipStream_t)stream, values, (const int32_t*)nullptr, 0, weights_scaled,
                       n_items, capacity_scaled, (int64_t*)ws, selected);
    GN_LAUNCH_CHECK("knapsack");
    return 0;
}

int goalnet_fscore(const uint8_t* gd, const uint8_t* mask, int n_users, int full_n_frames, double* fscore, int64_t* counts,
                   void* stream) {
    GN_REQUIRE(gd && mask && fscore && counts, GOALNET_E_NULL, "fscore: null pointer");
    GN_REQUIRE(n_users >= 1 && full_n_frames >= 1, GOALNET_E_SHAPE, "fscore: need n_users >= 1 and frames >= 1");
    hipStream_t st = (hipStream_t)stream;
    hipLaunchKernelGGL(fscore_counts_kernel, dim3(n_users + 1), dim3(256), 0, st, gd, mask, n_users, full_n_frames, counts);
    GN_LAUNCH_CHECK("fscore.counts");
    hipLaunchKernelGGL(fscore_final_kernel, dim3(1), dim3(1), 0, st, counts, n_users, fscore);
    GN_LAUNCH_CHECK("fscore.final");
    return 0;
}

size_t goalnet_postprocess_ws_bytes(int n_clips, int capacity_scaled, int n_users) {
    if (n_clips < 0 || capacity_scaled < 0 || n_users < 0) return 0;
    return goalnet_knapsack_ws_bytes(n_clips, capacity_scaled) + align256((size_t)(n_users + 1) * 2 * sizeof(int64_t));
}

int goalnet_postprocess(const float* pred, int n_sampled, int skip_frames, int full_n_frames, const int32_t* change_points,
                        int n_clips, int weight_scale, int capacity_scaled, const uint8_t* gd, int n_users, uint8_t* mask,
                        int32_t* selected, int64_t* clip_values, int32_t* clip_lengths, double* fscore, int32_t* status,
                        void* ws, size_t ws_bytes, void* stream) {
    GN_REQUIRE(pred && change_points && mask && selected && clip_values && clip_lengths && status && ws, GOALNET_E_NULL,
               "postprocess: null pointer");
    GN_REQUIRE((gd == nullptr) == (fscore == nullptr), GOALNET_E_NULL, "postprocess: gd and fscore must both be set or both NULL");
    GN_REQUIRE(n_sampled >= 1 && skip_frames >= 1 && full_n_frames >= 1 && n_clips >= 1 && weight_scale >= 0 && capacity_scaled >= 0 &&
               (gd == nullptr || n_users >= 1), GOALNET_E_SHAPE, "postprocess: bad dims");
    GN_REQUIRE(ws_bytes >= goalnet_postprocess_ws_bytes(n_clips, capacity_scaled, gd ? n_users : 0), GOALNET_E_WORKSPACE,
               "postprocess: workspace too small");
    hipStream_t st = (hipStream_t)stream;
    hipError_t e = hipMemsetAsync(mask, 0, (size_t)full_n_frames, st);
    if (e == hipSuccess) e = hipMemsetAsync(status, 0, sizeof(int32_t), st);
    if (e != hipSuccess) { set_error("postprocess: memset failed: %s", hipGetErrorString(e)); return (int)e; }
    hipLaunchKernelGGL(clip_info_kernel, dim3(n_clips), dim3(256), 0, st, pred, n_sampled, skip_frames, full_n_frames, change_points,
                       n_clips, clip_values, clip_lengths);
    GN_LAUNCH_CHECK("postprocess.clip_info");
    hipLaunchKernelGGL(knapsack_kernel, dim3(1), dim3(1024), 0, st, (const int64_t*)clip_values, (const int32_t*)clip_lengths, weight_scale,
                       (const int32_t*)nullptr, n_clips, capacity_scaled, (int64_t*)ws, selected);
    GN_LAUNCH_CHECK("postprocess.knapsack");
    hipLaunchKernelGGL(summary_mask_kernel, dim3(n_clips), dim3(256), 0, st, change_points, (const int32_t*)selected, n_clips, full_n_frames,
                       mask, status);
    GN_LAUNCH_CHECK("postprocess.mask");
    if (gd) {
        int64_t* counts = (int64_t*)((char*)ws + goalnet_knapsack_ws_bytes(n_clips, capacity_scaled));
        return goalnet_fscore(gd, mask, n_users, full_n_frames, fscore, counts, stream);
    }
    return 0;
}

// per item: [decision bits | two rows (rolling variant only) | F-score counts], each part 256-byte aligned
static size_t pb_bits_bytes(int n_clips, int cap) { return align256((size_t)n_clips * (size_t)((cap + 1 + 63) / 64) * sizeof(uint64_t)); }
static size_t pb_rows_bytes(int cap) { return kb_rolling(cap) ? align256(2 * (size_t)(cap + 1) * sizeof(int64_t)) : 0; }
static size_t pb_counts_bytes(int n_users) { return n_users > 0 ? align256((size_t)(n_users + 1) * 2 * sizeof(int64_t)) : 0; }

size_t goalnet_postprocess_batch_ws_bytes(int n_clips, int capacity_scaled, int n_users, int batch) {
    if (n_clips < 0 || capacity_scaled < 0 || n_users < 0 || batch < 0) return 0;
    return (size_t)batch * (pb_bits_bytes(n_clips, capacity_scaled) + pb_rows_bytes(capacity_scaled) + pb_counts_bytes(n_users));
}

const char* goalnet_postprocess_batch_kernel_name(int n_clips, int capacity_scaled) {
    (void)n_clips;
    if (capacity_scaled < 0) return "";
    if (kb_rolling(capacity_scaled)) return "knapsack_batch_rolling_kernel";
    switch (kb_maxc(capacity_scaled)) {
        case 4: return "knapsack_batch_lds_kernel<4>";
        case 8: return "knapsack_batch_lds_kernel<8>";
        case 16: return "knapsack_batch_lds_kernel<16>";
        default: return "knapsack_batch_lds_kernel<20>";
    }
}

int goalnet_postprocess_batch(const float* pred, int batch, int n_sampled, int skip_frames, int full_n_frames,
                              const int32_t* change_points, int n_clips, int weight_scale, int capacity_scaled, const uint8_t* gd,
                              int n_users, uint8_t* mask, int32_t* selected, int64_t* clip_values, int32_t* clip_lengths, double* fscore,
                              int32_t* status, void* ws, size_t ws_bytes, void* stream) {
    GN_REQUIRE(pred && change_points && mask && selected && clip_values && clip_lengths && status && ws, GOALNET_E_NULL,
               "postprocess_batch: null pointer");
    GN_REQUIRE((gd == nullptr) == (fscore == nullptr), GOALNET_E_NULL, "postprocess_batch: gd and fscore must both be set or both NULL");
    GN_REQUIRE(batch >= 1 && batch <= 65535 && n_sampled >= 1 && skip_frames >= 1 && full_n_frames >= 1 && n_clips >= 1 && weight_scale >= 0 &&
               capacity_scaled >= 0 && (gd == nullptr || n_users >= 1), GOALNET_E_SHAPE,
               "postprocess_batch: bad dims (need 1 <= batch <= 65535 and positive sizes)");
    const int users = gd ? n_users : 0;
    GN_REQUIRE(ws_bytes >= goalnet_postprocess_batch_ws_bytes(n_clips, capacity_scaled, users, batch), GOALNET_E_WORKSPACE,
               "postprocess_batch: workspace too small");
    hipStream_t st = (hipStream_t)stream;
    const size_t bits_bytes = pb_bits_bytes(n_clips, capacity_scaled), rows_bytes = pb_rows_bytes(capacity_scaled);
    uint64_t* bits = (uint64_t*)ws;
    int64_t* rows = (int64_t*)((char*)ws + (size_t)batch * bits_bytes);
    int64_t* counts = (int64_t*)((char*)rows + (size_t)batch * rows_bytes);
    hipError_t e = hipMemsetAsync(mask, 0, (size_t)batch * (size_t)full_n_frames, st);
    if (e == hipSuccess) e = hipMemsetAsync(status, 0, (size_t)batch * sizeof(int32_t), st);
    if (e != hipSuccess) { set_error("postprocess_batch: memset failed: %s", hipGetErrorString(e)); return (int)e; }
    hipLaunchKernelGGL(clip_info_batch_kernel, dim3(n_clips, batch), dim3(256), 0, st, pred, n_sampled, skip_frames, full_n_frames,
                       change_points, n_clips, clip_values, clip_lengths);
    GN_LAUNCH_CHECK("postprocess_batch.clip_info");
    const int64_t* cv = clip_values;
    const int32_t* cl = clip_lengths;
    if (kb_rolling(capacity_scaled)) {
        hipLaunchKernelGGL(knapsack_batch_rolling_kernel, dim3(batch), dim3(KB_THREADS), 0, st, cv, cl, weight_scale, n_clips, capacity_scaled,
                           bits, bits_bytes / sizeof(uint64_t), rows, selected);
        e = hipGetLastError();
    } else {
        const size_t stride = bits_bytes / sizeof(uint64_t);
        switch (kb_maxc(capacity_scaled)) {
            case 4: e = launch_knapsack_batch_lds<4>(st, batch, cv, cl, weight_scale, n_clips, capacity_scaled, bits, stride, selected); break;
            case 8: e = launch_knapsack_batch_lds<8>(st, batch, cv, cl, weight_scale, n_clips, capacity_scaled, bits, stride, selected); break;
            case 16: e = launch_knapsack_batch_lds<16>(st, batch, cv, cl, weight_scale, n_clips, capacity_scaled, bits, stride, selected); break;
            default: e = launch_knapsack_batch_lds<20>(st, batch, cv, cl, weight_scale, n_clips, capacity_scaled, bits, stride, selected); break;
        }
    }
    if (e != hipSuccess) { set_error("postprocess_batch.knapsack: launch failed: %s", hipGetErrorString(e)); return (int)e; }
    hipLaunchKernelGGL(summary_mask_batch_kernel, dim3(n_clips, batch), dim3(256), 0, st, change_points, (const int32_t*)selected, n_clips,
                       full_n_frames, mask, status);
    GN_LAUNCH_CHECK("postprocess_batch.mask");
    if (gd) {
        const size_t cstride = pb_counts_bytes(n_users) / sizeof(int64_t);
        hipLaunchKernelGGL(fscore_counts_batch_kernel, dim3(n_users + 1, batch), dim3(256), 0, st, gd, (const uint8_t*)mask, n_users,
                           full_n_frames, counts, cstride);
        GN_LAUNCH_CHECK("postprocess_batch.fscore_counts");
        hipLaunchKernelGGL(fscore_final_batch_kernel, dim3((batch + 63) / 64), dim3(64), 0, st, (const int64_t*)counts, cstride, n_users, batch,
                           fscore);
        GN_LAUNCH_CHECK("postprocess_batch.fscore_final");
    }
    return 0;
}

int goalnet_mean_annotations(const float* scores, int n_annotators, int full_n_frames, int skip_frames, float* labels_trimmed,
                             float* labels_full, void* stream) {
    GN_REQUIRE(scores && labels_trimmed && labels_full, GOALNET_E_NULL, "mean_annotations: null pointer");
    GN_REQUIRE(n_annotators >= 1 && n_annotators <= 128 && full_n_frames >= 1 && skip_frames >= 1, GOALNET_E_SHAPE,
               "mean_annotations: need 1 <= annotators <= 128, frames >= 1, skip_frames >= 1");
    hipLaunchKernelGGL(mean_annotations_kernel, dim3((full_n_frames + 255) / 256), dim3(256), 0, (hipStream_t)stream, scores, n_annotators,
                       full_n_frames, skip_frames, labels_trimmed, labels_full);
    GN_LAUNCH_CHECK("mean_annotations");
    return 0;
}

}  // extern "C"
