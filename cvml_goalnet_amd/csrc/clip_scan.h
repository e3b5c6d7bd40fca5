// The scan in front of a clip gather (goalnet_gather_clips in summary.hip, goalnet_nv12_gather_clips_bgr in nv12.hip): both entry
// points compile this one kernel, so `count`, `status` and the frame order of the two are the same by construction.
#pragma once
#include "common.h"

namespace goalnet {

static inline size_t align256(size_t b) { return (b + 255) / 256 * 256; }
static inline size_t offsets_bytes(int n_clips) { return align256((size_t)(n_clips + 1) * sizeof(int64_t)); }

// The frames [a, b) of clip c, clamped like a Python slice (as clip_info_kernel); b <= a: none. The one slice rule of the clip gathers
// and of the keyframe choice (storyboard.hip).
__device__ __forceinline__ void clip_slice(const int32_t* __restrict__ cps, int c, int full_n, int& a, int& b) {
    a = cps[2 * c];
    b = cps[2 * c + 1];
    if (a < 0) a = a + full_n < 0 ? 0 : a + full_n;
    if (b < 0) b = b + full_n < 0 ? 0 : b + full_n;
    a = a > full_n ? full_n : a;
    b = b > full_n ? full_n : b;
}

// One block. offsets[c] = number of summary frames in front of clip c (exclusive scan of the selected clips' slice lengths),
// offsets[n_clips] = their total; starts[c] = first source frame of clip c. [a:b) clamped like a Python slice (as clip_info_kernel).
static __global__ __launch_bounds__(256) void clip_offsets_kernel(const int32_t* __restrict__ cps, const int32_t* __restrict__ selected, int n_clips,
                                                          int full_n, int64_t capacity, int64_t* __restrict__ offsets,
                                                          int32_t* __restrict__ starts, int64_t* __restrict__ count, int32_t* __restrict__ status) {
    __shared__ int64_t s[256];
    const int t = threadIdx.x;
    const int per = (n_clips + 255) / 256;
    const int lo = t * per < n_clips ? t * per : n_clips, hi = lo + per < n_clips ? lo + per : n_clips;
    auto slice = [&](int c, int& a) -> int {
        int b;
        clip_slice(cps, c, full_n, a, b);
        return (selected[c] != 0 && b > a) ? b - a : 0;
    };
    int64_t local = 0;
    for (int c = lo; c < hi; ++c) { int a; local += slice(c, a); }
    s[t] = local;
    __syncthreads();
    for (int o = 1; o < 256; o <<= 1) {
        const int64_t v = t >= o ? s[t - o] : 0;
        __syncthreads();
        s[t] += v;
        __syncthreads();
    }
    int64_t run = s[t] - local;
    for (int c = lo; c < hi; ++c) {
        int a;
        const int len = slice(c, a);
        offsets[c] = run;
        starts[c] = a;
        run += len;
    }
    if (t == 255) {
        offsets[n_clips] = s[255];
        *count = s[255];
        *status = s[255] > capacity ? 1 : 0;
    }
}

}  // namespace goalnet
