// The reference's inference mode (/root/reference/main.py:300-348) around the model, for a decoded video that is resident in HBM:
//   sampling + pre-processing of every skip_frames-th frame   /root/reference/utils.py:274-292 (extract_condensed_frame_tensor)
//   the summarised video itself                               /root/reference/utils.py:634
//       np.concatenate([full_frames[a:b] for the selected clips])
// Both are HBM-traffic work on uint8 frames. Quirk kept: utils.py:634 slices end-EXCLUSIVE [a:b), the
// summary mask of utils.py:639-641 (postproc.hip) is end-INCLUSIVE [a, b]: the mask has one frame more per selected clip.
#include "common.h"
#include "frame_resize.h"
#include "clip_scan.h"

using namespace goalnet;

namespace {

// ---- strided pre-processing -------------------------------------------------------------------------------------------------
__global__ void minmax_init_kernel(int32_t* __restrict__ minmax, int n) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) { minmax[2 * i] = 255; minmax[2 * i + 1] = 0; }
}

__device__ __forceinline__ void minmax_word(uint32_t w, int& mn, int& mx) {
#pragma unroll
    for (int k = 0; k < 4; ++k) { const int v = (w >> (8 * k)) & 255; mn = v < mn ? v : mn; mx = v > mx ? v : mx; }
}

// min / max of the uint8 pixels of frame (blockIdx.x / bpf) * frame_stride, `bpf` blocks per frame: the bytes in front of the first
// 16-byte boundary and behind the last one are read one by one (block 0 of the frame), the vectors between them are dealt out to the
// frame's blocks in equal contiguous shares. Combined with integer atomicMin / atomicMax into minmax (initialised to {255, 0}):
// order-independent, so the result is deterministic.
__global__ __launch_bounds__(256) void frame_minmax_strided_kernel(const uint8_t* __restrict__ frames, int64_t frame_bytes, int64_t frame_pitch,
                                                                  int bpf, int32_t* __restrict__ minmax) {
    __shared__ int smn[4], smx[4];
    const int frame = blockIdx.x / bpf, part = blockIdx.x % bpf;
    const uint8_t* f = frames + (int64_t)frame * frame_pitch;
    int64_t head = (int64_t)((16 - (reinterpret_cast<uintptr_t>(f) & 15u)) & 15u);
    head = head < frame_bytes ? head : frame_bytes;
    const int64_t nvec = (frame_bytes - head) / 16, tail0 = head + nvec * 16;
    const int64_t share = (nvec + bpf - 1) / bpf;
    const int64_t v0 = (int64_t)part * share, v1 = v0 + share < nvec ? v0 + share : nvec;
    const uint4* vec = reinterpret_cast<const uint4*>(f + head);
    int mn = 255, mx = 0;
    int64_t i = v0 + threadIdx.x;
    for (; i + 256 < v1; i += 512) {                      // two independent 16-byte loads in flight per lane
        const uint4 a = vec[i], b = vec[i + 256];
        minmax_word(a.x, mn, mx); minmax_word(a.y, mn, mx); minmax_word(a.z, mn, mx); minmax_word(a.w, mn, mx);
        minmax_word(b.x, mn, mx); minmax_word(b.y, mn, mx); minmax_word(b.z, mn, mx); minmax_word(b.w, mn, mx);
    }
    if (i < v1) {
        const uint4 a = vec[i];
        minmax_word(a.x, mn, mx); minmax_word(a.y, mn, mx); minmax_word(a.z, mn, mx); minmax_word(a.w, mn, mx);
    }
    if (part == 0) {                                      // at most 15 + 15 bytes
        if ((int64_t)threadIdx.x < head) { const int v = f[threadIdx.x]; mn = v < mn ? v : mn; mx = v > mx ? v : mx; }
        if (tail0 + threadIdx.x < frame_bytes) { const int v = f[tail0 + threadIdx.x]; mn = v < mn ? v : mn; mx = v > mx ? v : mx; }
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) { const int a = __shfl_xor(mn, o, 64), b = __shfl_xor(mx, o, 64); mn = a < mn ? a : mn; mx = b > mx ? b : mx; }
    if ((threadIdx.x & 63) == 0) { smn[threadIdx.x >> 6] = mn; smx[threadIdx.x >> 6] = mx; }
    __syncthreads();
    if (threadIdx.x == 0) {
        for (int w = 1; w < 4; ++w) { mn = smn[w] < mn ? smn[w] : mn; mx = smx[w] > mx ? smx[w] : mx; }
        atomicMin(&minmax[2 * frame], mn);
        atomicMax(&minmax[2 * frame + 1], mx);
    }
}

__global__ __launch_bounds__(256) void frame_resize_strided_kernel(const uint8_t* __restrict__ frames, int64_t frame_pitch,
                                                                  const int32_t* __restrict__ minmax, float* __restrict__ out, int N, int H0,
                                                                  int W0, int H, int W, double scale_x, double scale_y) {
    frame_resize_all(frames, frame_pitch, minmax, out, N, H0, W0, H, W, scale_x, scale_y);
}

// ---- clip gather ----------------------------------------------------------------------------------------------------------
// Summary frame k = source frame starts[c] + (k - offsets[c]) of the clip c with offsets[c] <= k < offsets[c + 1]. A block copies one
// tile (256 lanes x 4 x sizeof(V) bytes of one frame) per iteration and strides over the tiles of the first min(total, capacity)
// frames; the total is read from the scan's output, so the grid is sized from the capacity without a host round trip.
template <typename V>
__global__ __launch_bounds__(256) void gather_clips_kernel(const uint8_t* __restrict__ frames, int64_t frame_bytes, const int64_t* __restrict__ offsets,
                                                          const int32_t* __restrict__ starts, int n_clips, int64_t capacity, int tiles_per_frame,
                                                          uint8_t* __restrict__ out, int32_t* __restrict__ src_index) {
    constexpr int64_t TILE = 256 * 4;                                    // elements of V per tile
    const int64_t total = offsets[n_clips];
    const int64_t n = total < capacity ? total : capacity;
    const int64_t elems = frame_bytes / (int64_t)sizeof(V);
    for (int64_t tile = blockIdx.x; tile < n * tiles_per_frame; tile += gridDim.x) {
        const int64_t k = tile / tiles_per_frame;
        const int part = (int)(tile % tiles_per_frame);
        int lo = 0, hi = n_clips;                                        // offsets[lo] <= k < offsets[hi]
        while (hi - lo > 1) {
            const int mid = (lo + hi) >> 1;
            if (offsets[mid] <= k) lo = mid; else hi = mid;
        }
        const int64_t src = (int64_t)starts[lo] + (k - offsets[lo]);
        if (part == 0 && threadIdx.x == 0) src_index[k] = (int32_t)src;
        const V* __restrict__ s = reinterpret_cast<const V*>(frames + src * frame_bytes);
        V* __restrict__ d = reinterpret_cast<V*>(out + k * frame_bytes);
        const int64_t e0 = (int64_t)part * TILE + threadIdx.x;
        if (e0 + 768 < elems) {                                          // whole tile: four loads in flight, then four stores
            const V v0 = s[e0], v1 = s[e0 + 256], v2 = s[e0 + 512], v3 = s[e0 + 768];
            d[e0] = v0; d[e0 + 256] = v1; d[e0 + 512] = v2; d[e0 + 768] = v3;
        } else {                                                         // the frame's last tile
            for (int64_t e = e0; e < elems; e += 256) d[e] = s[e];
        }
    }
}

template <typename V>
int launch_gather(const uint8_t* frames, int64_t frame_bytes, const int64_t* offsets, const int32_t* starts, int n_clips, int64_t capacity,
                  uint8_t* out, int32_t* src_index, hipStream_t st) {
    const int64_t tile_bytes = 256 * 4 * (int64_t)sizeof(V);
    const int64_t tpf = (frame_bytes + tile_bytes - 1) / tile_bytes;
    GN_REQUIRE(tpf <= INT32_MAX, GOALNET_E_SHAPE, "gather_clips: frame_bytes too large");
    const int64_t tiles = capacity * tpf;
    const unsigned blocks = (unsigned)(tiles < 2048 ? tiles : 2048);     // memory-bound: ~8 blocks per CU, stride over the rest
    hipLaunchKernelGGL(gather_clips_kernel<V>, dim3(blocks), dim3(256), 0, st, frames, frame_bytes, offsets, starts, n_clips, capacity, (int)tpf,
                       out, src_index);
    GN_LAUNCH_CHECK("gather_clips.copy");
    return 0;
}

}  // namespace

extern "C" {

int goalnet_frames_preprocess_strided(const uint8_t* frames_hwc, int n_total, int frame_stride, int H0, int W0, float* out_nchw, int H, int W,
                                      int32_t* minmax, void* stream) {
    GN_REQUIRE(frames_hwc && out_nchw && minmax, GOALNET_E_NULL, "frames_preprocess_strided: null pointer");
    GN_REQUIRE(n_total >= 1, GOALNET_E_SHAPE, "frames_preprocess_strided: n_total must be >= 1");
    GN_REQUIRE(frame_stride >= 1, GOALNET_E_SHAPE, "frames_preprocess_strided: frame_stride must be >= 1");
    GN_REQUIRE(H0 > 0 && W0 > 0 && H > 0 && W > 0, GOALNET_E_SHAPE, "frames_preprocess_strided: non-positive dim");
    hipStream_t st = (hipStream_t)stream;
    const int n = (int)(((int64_t)n_total + frame_stride - 1) / frame_stride);      // frames 0, stride, 2 stride, ... < n_total
    const int64_t frame_bytes = (int64_t)H0 * W0 * 3, pitch = frame_bytes * frame_stride;
    hipLaunchKernelGGL(minmax_init_kernel, dim3((n + 255) / 256), dim3(256), 0, st, minmax, n);
    GN_LAUNCH_CHECK("frames_preprocess_strided.init");
    // ~2048 blocks in all, and at least 1024 vectors (16 KB) per block
    int64_t bpf = (2048 + n - 1) / n;
    const int64_t by_size = (frame_bytes / 16 + 1023) / 1024;
    bpf = bpf < by_size ? bpf : by_size;
    bpf = bpf < 1 ? 1 : bpf;
    hipLaunchKernelGGL(frame_minmax_strided_kernel, dim3((unsigned)(n * bpf)), dim3(256), 0, st, frames_hwc, frame_bytes, pitch, (int)bpf, minmax);
    GN_LAUNCH_CHECK("frames_preprocess_strided.minmax");
    hipLaunchKernelGGL(frame_resize_strided_kernel, dim3(resize_blocks((int64_t)n * 3 * H * W)), dim3(256), 0, st, frames_hwc, pitch,
                       (const int32_t*)minmax, out_nchw, n, H0, W0, H, W, resize_scale(W, W0), resize_scale(H, H0));
    GN_LAUNCH_CHECK("frames_preprocess_strided.resize");
    return 0;
}

size_t goalnet_gather_clips_ws_bytes(int n_clips) {
    if (n_clips < 0) return 0;
    return offsets_bytes(n_clips) + align256((size_t)n_clips * sizeof(int32_t));
}

int goalnet_gather_clips(const uint8_t* frames, int full_n, int64_t frame_bytes, const int32_t* change_points, const int32_t* selected,
                         int n_clips, uint8_t* out, int64_t out_capacity_frames, int32_t* src_index, int64_t* count, int32_t* status,
                         void* ws, size_t ws_bytes, void* stream) {
    GN_REQUIRE(frames && change_points && selected && out && src_index && count && status && ws, GOALNET_E_NULL, "gather_clips: null pointer");
    GN_REQUIRE(full_n >= 1, GOALNET_E_SHAPE, "gather_clips: full_n must be >= 1");
    GN_REQUIRE(frame_bytes >= 1, GOALNET_E_SHAPE, "gather_clips: frame_bytes must be >= 1");
    GN_REQUIRE(n_clips >= 1 && out_capacity_frames >= 0, GOALNET_E_SHAPE, "gather_clips: need n_clips >= 1 and out_capacity_frames >= 0");
    GN_REQUIRE(ws_bytes >= goalnet_gather_clips_ws_bytes(n_clips), GOALNET_E_WORKSPACE, "gather_clips: workspace too small");
    hipStream_t st = (hipStream_t)stream;
    int64_t* offsets = (int64_t*)ws;
    int32_t* starts = (int32_t*)((char*)ws + offsets_bytes(n_clips));
    hipLaunchKernelGGL(clip_offsets_kernel, dim3(1), dim3(256), 0, st, change_points, selected, n_clips, full_n, out_capacity_frames, offsets,
                       starts, count, status);
    GN_LAUNCH_CHECK("gather_clips.offsets");
    if (out_capacity_frames == 0) return 0;
    const bool a16 = frame_bytes % 16 == 0 && aligned16(frames) && aligned16(out);
    const bool a4 = frame_bytes % 4 == 0 && (reinterpret_cast<uintptr_t>(frames) & 3u) == 0 && (reinterpret_cast<uintptr_t>(out) & 3u) == 0;
    if (a16) return launch_gather<uint4>(frames, frame_bytes, offsets, starts, n_clips, out_capacity_frames, out, src_index, st);
    if (a4) return launch_gather<uint32_t>(frames, frame_bytes, offsets, starts, n_clips, out_capacity_frames, out, src_index, st);
    return launch_gather<uint8_t>(frames, frame_bytes, offsets, starts, n_clips, out_capacity_frames, out, src_index, st);
}

}  // extern "C"
