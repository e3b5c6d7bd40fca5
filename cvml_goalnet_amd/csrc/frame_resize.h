// One output pixel of the loader's frame pre-processing (/root/reference/utils.py:284-285): min-max normalisation in float64,
// float32, then OpenCV's INTER_LINEAR resize for float32 images (imgproc/resize.cpp: half-pixel centres, floor, border clamp,
// horizontal pass then vertical pass). Shared by goalnet_frames_preprocess (preproc.hip) and goalnet_frames_preprocess_strided
// (summary.hip), and through frame_resize_pixel_of by goalnet_nv12_preprocess_strided (nv12.hip), so that all compile the same
// arithmetic: their outputs are bit-identical by construction.
#pragma once
#include "common.h"

namespace goalnet {

// rounded product / sum without fma contraction (OpenCV's scalar path multiplies and adds separately)
__device__ __forceinline__ float mul_rn(float a, float b) { return __builtin_fmaf(a, b, 0.0f); }

// fetch(yy, xx): the 0 .. 255 value of source pixel (yy, xx) in the output element's channel (packed BGR below; nv12.hip converts
// the pixel on the way); mn / mx: the frame's min and max over all three channels; (dy, dx): the output element
template <typename Fetch>
__device__ __forceinline__ float frame_resize_pixel_of(Fetch fetch, int mn, int mx, int dy, int dx, int H0, int W0, double scale_x,
                                                       double scale_y) {
    // source coordinates, resize.cpp: fx = (float)((dx + 0.5) * scale_x - 0.5); sx = floor(fx); fx -= sx; border clamp
    float fx = (float)(((double)dx + 0.5) * scale_x - 0.5);
    int sx = (int)floorf(fx);
    fx -= (float)sx;
    if (sx < 0) { sx = 0; fx = 0.f; }
    if (sx >= W0 - 1) { sx = W0 - 1; fx = 0.f; }
    float fy = (float)(((double)dy + 0.5) * scale_y - 0.5);
    int sy = (int)floorf(fy);
    fy -= (float)sy;
    if (sy < 0) { sy = 0; fy = 0.f; }
    if (sy >= H0 - 1) { sy = H0 - 1; fy = 0.f; }
    const int sx1 = sx + 1 < W0 ? sx + 1 : W0 - 1, sy1 = sy + 1 < H0 ? sy + 1 : H0 - 1;
    const double den = (double)(mx - mn) + 1e-7;                        // uint8 difference, then + 1e-7 in float64
    auto px = [&](int yy, int xx) -> float { return (float)((double)(fetch(yy, xx) - mn) / den); };
    const float a0 = 1.f - fx, a1 = fx, b0 = 1.f - fy, b1 = fy;
    const float h0 = mul_rn(px(sy, sx), a0) + mul_rn(px(sy, sx1), a1);   // horizontal pass on the two source rows
    const float h1 = mul_rn(px(sy1, sx), a0) + mul_rn(px(sy1, sx1), a1);
    return mul_rn(h0, b0) + mul_rn(h1, b1);                             // vertical pass
}

// f: the source frame [H0][W0][3] uint8; c: the output element's channel
__device__ __forceinline__ float frame_resize_pixel(const uint8_t* __restrict__ f, int mn, int mx, int c, int dy, int dx, int H0, int W0,
                                                    double scale_x, double scale_y) {
    return frame_resize_pixel_of([&](int yy, int xx) -> int { return f[((int64_t)yy * W0 + xx) * 3 + c]; }, mn, mx, dy, dx, H0, W0, scale_x,
                                 scale_y);
}

// out[N][3][H][W] from frames n * frame_pitch (bytes) of `frames`; minmax[n] = {min, max} of that frame
__device__ __forceinline__ void frame_resize_all(const uint8_t* __restrict__ frames, int64_t frame_pitch, const int32_t* __restrict__ minmax,
                                                 float* __restrict__ out, int N, int H0, int W0, int H, int W, double scale_x, double scale_y) {
    const int64_t total = (int64_t)N * 3 * H * W;
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (int64_t)gridDim.x * blockDim.x) {
        const int dx = (int)(i % W), dy = (int)((i / W) % H), c = (int)((i / ((int64_t)W * H)) % 3);
        const int64_t n = i / ((int64_t)3 * H * W);
        out[i] = frame_resize_pixel(frames + n * frame_pitch, minmax[2 * n], minmax[2 * n + 1], c, dy, dx, H0, W0, scale_x, scale_y);
    }
}

// cv2.resize: inv_scale = dsize / ssize (double), scale = 1 / inv_scale
static inline double resize_scale(int dst, int src) { return 1.0 / ((double)dst / (double)src); }
static inline unsigned resize_blocks(int64_t total) {
    const int64_t blocks = (total + 255) / 256;
    return (unsigned)(blocks > 8192 ? 8192 : blocks);
}

}  // namespace goalnet
