// Frame pre-processing of the reference's loader, /root/reference/utils.py:274-292:
//     image = ((image - image.min()) / (image.max() - image.min() + 1e-7)).astype(np.float32)     # per decoded BGR frame, uint8 HWC
//     image = cv2.resize(image, (40, 40))                                                         # INTER_LINEAR on float32
//     np.transpose(np.array(frames), (0, 3, 1, 2))                                                # -> (N, 3, H, W), channel order BGR
// on the device, for frames that are already decoded (cv2.VideoCapture stays the reference's I/O).
// PARITY UNPINNED: OpenCV is not in the image, so neither the oracle restatement (oracle/preproc_ref.py) nor this kernel can
// be checked against cv2 here. Both follow OpenCV's published bilinear resize for float32 (imgproc/resize.cpp: half-pixel
// centres fx = (dx + 0.5) * scale - 0.5, floor, clamp to the border, horizontal pass then vertical pass, no antialiasing)
// and agree with each other bit for bit.
#include "common.h"
#include "frame_resize.h"

using namespace goalnet;

namespace {

// per-frame min / max of the uint8 pixels (all three channels together, as image.min() / image.max())
__global__ __launch_bounds__(256) void frame_minmax_kernel(const uint8_t* __restrict__ frames, int64_t frame_bytes, int32_t* __restrict__ minmax) {
    __shared__ int smn[4], smx[4];
    const uint8_t* f = frames + (int64_t)blockIdx.x * frame_bytes;
    int mn = 255, mx = 0;
    for (int64_t i = threadIdx.x; i < frame_bytes; i += 256) { const int v = f[i]; mn = v < mn ? v : mn; mx = v > mx ? v : mx; }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) { const int a = __shfl_xor(mn, o, 64), b = __shfl_xor(mx, o, 64); mn = a < mn ? a : mn; mx = b > mx ? b : mx; }
    if ((threadIdx.x & 63) == 0) { smn[threadIdx.x >> 6] = mn; smx[threadIdx.x >> 6] = mx; }
    __syncthreads();
    if (threadIdx.x == 0) {
        for (int w = 1; w < 4; ++w) { mn = smn[w] < mn ? smn[w] : mn; mx = smx[w] > mx ? smx[w] : mx; }
        minmax[2 * blockIdx.x] = mn;
        minmax[2 * blockIdx.x + 1] = mx;
    }
}

// the per-pixel arithmetic lives in frame_resize.h, shared with the strided entry point (summary.hip)
__global__ __launch_bounds__(256) void frame_resize_kernel(const uint8_t* __restrict__ frames, const int32_t* __restrict__ minmax,
                                                          float* __restrict__ out, int N, int H0, int W0, int H, int W,
                                                          double scale_x, double scale_y) {
    frame_resize_all(frames, (int64_t)H0 * W0 * 3, minmax, out, N, H0, W0, H, W, scale_x, scale_y);
}

}  // namespace

extern "C" {

int goalnet_frames_preprocess(const uint8_t* frames_hwc, int N, int H0, int W0, float* out_nchw, int H, int W,
                              int32_t* minmax, void* stream) {
    GN_REQUIRE(frames_hwc && out_nchw && minmax, GOALNET_E_NULL, "frames_preprocess: null pointer");
    GN_REQUIRE(N > 0 && H0 > 0 && W0 > 0 && H > 0 && W > 0, GOALNET_E_SHAPE, "frames_preprocess: non-positive dim");
    hipStream_t st = (hipStream_t)stream;
    hipLaunchKernelGGL(frame_minmax_kernel, dim3(N), dim3(256), 0, st, frames_hwc, (int64_t)H0 * W0 * 3, minmax);
    GN_LAUNCH_CHECK("frames_preprocess.minmax");
    hipLaunchKernelGGL(frame_resize_kernel, dim3(resize_blocks((int64_t)N * 3 * H * W)), dim3(256), 0, st, frames_hwc, (const int32_t*)minmax,
                       out_nchw, N, H0, W0, H, W, resize_scale(W, W0), resize_scale(H, H0));
    GN_LAUNCH_CHECK("frames_preprocess.resize");
    return 0;
}

}  // extern "C"
