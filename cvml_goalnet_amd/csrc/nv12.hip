// NV12 frames as an input of the inference path (include/goalnet_nv12.h; EXTENSION, the integer conversion is defined there):
//   goalnet_nv12_to_bgr               n frames -> compact BGR
//   goalnet_nv12_preprocess_strided   summary.hip's strided pre-processing, converting only what it consumes
//   goalnet_nv12_gather_clips_bgr     summary.hip's clip gather, converting on the way
// All three are HBM-traffic work on bytes. The unit of work is a BLOCK of 2 rows x 16 pixels: one lane loads 16 bytes of each Y row
// and the 16 bytes (8 U, V pairs) of the chroma row they share, converts 32 pixels in registers and holds 2 x 48 output bytes. With
// every row start on a 16-byte boundary the loads are 16-byte vectors and consecutive lanes read consecutive vectors of a row; a
// row's last, partial block and every block of an unaligned layout are loaded byte by byte, and only the W0 picture bytes of a row
// are ever loaded, so padding cannot reach a result and nothing behind the last chroma row's W0 bytes is touched.
#include "common.h"
#include "frame_resize.h"
#include "clip_scan.h"
#include "nv12_pixel.h"

using namespace goalnet;

namespace {

// Block (row pair yp, chunk xc) of frame f: ya / yb = 16 bytes of rows 2 yp and 2 yp + 1 from column 16 xc, uv = the 16 chroma bytes
// of those columns, little-endian in 4 words each. Returns the number of picture columns in the block (even, 2 .. 16); bytes beyond
// them are zero and not loaded. VEC: the row starts are 16-byte aligned (the host checked it).
template <bool VEC>
__device__ __forceinline__ int nv12_load_block(const uint8_t* __restrict__ f, const Nv12Geom& g, int yp, int xc, uint32_t (&ya)[4],
                                               uint32_t (&yb)[4], uint32_t (&uv)[4]) {
    const int x0 = xc << 4;
    const int cnt = g.W0 - x0 < 16 ? g.W0 - x0 : 16;
    const uint8_t* pa = f + (int64_t)(2 * yp) * g.pitch + x0;
    const uint8_t* pb = pa + g.pitch;
    const uint8_t* pc = f + g.uv_offset + (int64_t)yp * g.pitch + x0;
    if (VEC && cnt == 16) {
        const uint4 a = *reinterpret_cast<const uint4*>(pa), b = *reinterpret_cast<const uint4*>(pb), c = *reinterpret_cast<const uint4*>(pc);
        ya[0] = a.x; ya[1] = a.y; ya[2] = a.z; ya[3] = a.w;
        yb[0] = b.x; yb[1] = b.y; yb[2] = b.z; yb[3] = b.w;
        uv[0] = c.x; uv[1] = c.y; uv[2] = c.z; uv[3] = c.w;
    } else {
#pragma unroll
        for (int w = 0; w < 4; ++w) ya[w] = yb[w] = uv[w] = 0u;
#pragma unroll
        for (int b = 0; b < 16; ++b) {
            if (b < cnt) {
                ya[b >> 2] |= (uint32_t)pa[b] << (8 * (b & 3));
                yb[b >> 2] |= (uint32_t)pb[b] << (8 * (b & 3));
                uv[b >> 2] |= (uint32_t)pc[b] << (8 * (b & 3));
            }
        }
    }
    return cnt;
}

// emit(row 0 / 1, column 0 .. 15, B, G, R) for the 32 pixels of a loaded block; the chroma terms are computed once per 2 x 2 pixels
template <typename Emit>
__device__ __forceinline__ void nv12_convert_block(const Nv12Coef& k, const uint32_t (&ya)[4], const uint32_t (&yb)[4], const uint32_t (&uv)[4],
                                                   Emit emit) {
#pragma unroll
    for (int j = 0; j < 8; ++j) {
        const uint32_t pair = uv[j >> 1] >> (16 * (j & 1));
        const int u = (int)(pair & 255u) - 128, v = (int)((pair >> 8) & 255u) - 128;
        const int cb = k.cub * u + k.r0, cg = k.cug * u + k.cvg * v + k.r0, cr = k.cvr * v + k.r0;
#pragma unroll
        for (int r = 0; r < 2; ++r) {
#pragma unroll
            for (int e = 0; e < 2; ++e) {
                const int p = 2 * j + e;
                const int Y = (int)(((r ? yb[p >> 2] : ya[p >> 2]) >> (8 * (p & 3))) & 255u);
                const int d = Y - k.y_off;
                const int yy = (d < 0 ? 0 : d) * k.cy;
                emit(r, p, sat8((yy + cb) >> k.shift), sat8((yy + cg) >> k.shift), sat8((yy + cr) >> k.shift));
            }
        }
    }
}

// how a block's 48 output bytes per row go out: 16-byte vectors (W0 % 16 == 0 and `out` 16-byte aligned: every block is whole and
// starts on a boundary), 4-byte words (W0 % 4 == 0, `out` 4-byte aligned) or single bytes
enum { ST_BYTES = 0, ST_WORDS = 1, ST_VECTORS = 2 };

// item = yp * chunks + xc of source frame f -> the same block of the compact BGR frame d
template <bool VEC>
__device__ __forceinline__ void nv12_block_to_bgr(const uint8_t* __restrict__ f, uint8_t* __restrict__ d, const Nv12Geom& g, const Nv12Coef& k,
                                                  int chunks, int item, int st) {
    const int yp = item / chunks, xc = item - yp * chunks;
    uint32_t ya[4], yb[4], uv[4], o[2][12];
    const int cnt = nv12_load_block<VEC>(f, g, yp, xc, ya, yb, uv);
#pragma unroll
    for (int w = 0; w < 12; ++w) o[0][w] = o[1][w] = 0u;
    nv12_convert_block(k, ya, yb, uv, [&](int r, int p, int B, int G, int R) {
        o[r][(3 * p) >> 2] |= (uint32_t)B << (8 * ((3 * p) & 3));
        o[r][(3 * p + 1) >> 2] |= (uint32_t)G << (8 * ((3 * p + 1) & 3));
        o[r][(3 * p + 2) >> 2] |= (uint32_t)R << (8 * ((3 * p + 2) & 3));
    });
#pragma unroll
    for (int r = 0; r < 2; ++r) {
        uint8_t* dst = d + ((int64_t)(2 * yp + r) * g.W0 + (xc << 4)) * 3;
        if (st == ST_VECTORS) {                                        // cnt == 16
            uint4* dv = reinterpret_cast<uint4*>(dst);
            dv[0] = make_uint4(o[r][0], o[r][1], o[r][2], o[r][3]);
            dv[1] = make_uint4(o[r][4], o[r][5], o[r][6], o[r][7]);
            dv[2] = make_uint4(o[r][8], o[r][9], o[r][10], o[r][11]);
        } else if (st == ST_WORDS) {                                   // cnt % 4 == 0: 3 cnt / 4 whole words
            uint32_t* dw = reinterpret_cast<uint32_t*>(dst);
#pragma unroll
            for (int w = 0; w < 12; ++w)
                if (4 * w < 3 * cnt) dw[w] = o[r][w];
        } else {
#pragma unroll
            for (int b = 0; b < 48; ++b)
                if (b < 3 * cnt) dst[b] = (uint8_t)(o[r][b >> 2] >> (8 * (b & 3)));
        }
    }
}

template <bool VEC>
__global__ __launch_bounds__(256) void nv12_to_bgr_kernel(const uint8_t* __restrict__ frames, int64_t frame_pitch, Nv12Geom g, Nv12Coef k,
                                                         uint8_t* __restrict__ out, int64_t total, int chunks, int st) {
    const int per_frame = (g.H0 >> 1) * chunks;
    const int64_t out_bytes = (int64_t)g.H0 * g.W0 * 3;
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < total; i += (int64_t)gridDim.x * 256) {
        const int64_t n = i / per_frame;
        nv12_block_to_bgr<VEC>(frames + n * frame_pitch, out + n * out_bytes, g, k, chunks, (int)(i - n * per_frame), st);
    }
}

// min / max of the converted B, G, R values of frame (blockIdx.x / bpf) * (sample_pitch / frame_pitch): the frame's blocks of 2 x 16
// pixels are dealt out to its `bpf` thread blocks in equal contiguous shares; integer atomicMin / atomicMax into minmax (initialised
// to {255, 0}), order-independent as in summary.hip.
template <bool VEC>
__global__ __launch_bounds__(256) void nv12_minmax_strided_kernel(const uint8_t* __restrict__ frames, int64_t sample_pitch, Nv12Geom g, Nv12Coef k,
                                                                 int chunks, int bpf, int32_t* __restrict__ minmax) {
    __shared__ int smn[4], smx[4];
    const int frame = blockIdx.x / bpf, part = blockIdx.x % bpf;
    const uint8_t* f = frames + (int64_t)frame * sample_pitch;
    const int items = (g.H0 >> 1) * chunks;
    const int share = (items + bpf - 1) / bpf;
    const int i0 = part * share, i1 = i0 + share < items ? i0 + share : items;
    int mn = 255, mx = 0;
    for (int i = i0 + threadIdx.x; i < i1; i += 256) {
        const int yp = i / chunks, xc = i - yp * chunks;
        uint32_t ya[4], yb[4], uv[4];
        const int cnt = nv12_load_block<VEC>(f, g, yp, xc, ya, yb, uv);
        nv12_convert_block(k, ya, yb, uv, [&](int, int p, int B, int G, int R) {
            if (p < cnt) {
                const int lo = B < G ? (B < R ? B : R) : (G < R ? G : R), hi = B > G ? (B > R ? B : R) : (G > R ? G : R);
                mn = lo < mn ? lo : mn;
                mx = hi > mx ? hi : mx;
            }
        });
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

__global__ void nv12_minmax_init_kernel(int32_t* __restrict__ minmax, int n) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) { minmax[2 * i] = 255; minmax[2 * i + 1] = 0; }
}

// frame_resize.h's arithmetic with the pixel fetch converting on the way: at most 4 source pixels per output element, one channel each
__global__ __launch_bounds__(256) void nv12_resize_strided_kernel(const uint8_t* __restrict__ frames, int64_t sample_pitch, Nv12Geom g, Nv12Coef k,
                                                                 const int32_t* __restrict__ minmax, float* __restrict__ out, int N, int H, int W,
                                                                 double scale_x, double scale_y) {
    const int64_t total = (int64_t)N * 3 * H * W;
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (int64_t)gridDim.x * blockDim.x) {
        const int dx = (int)(i % W), dy = (int)((i / W) % H), c = (int)((i / ((int64_t)W * H)) % 3);
        const int64_t n = i / ((int64_t)3 * H * W);
        const uint8_t* f = frames + n * sample_pitch;
        out[i] = frame_resize_pixel_of([&](int yy, int xx) -> int { return nv12_channel(f, g, k, yy, xx, c); }, minmax[2 * n], minmax[2 * n + 1], dy,
                                       dx, g.H0, g.W0, scale_x, scale_y);
    }
}

// gather_clips_kernel of summary.hip with a conversion for a copy: a block handles one tile (256 blocks of 2 x 16 pixels of one
// summary frame) per iteration and strides over the tiles of the first min(total, capacity) frames
template <bool VEC>
__global__ __launch_bounds__(256) void nv12_gather_clips_kernel(const uint8_t* __restrict__ frames, int64_t frame_pitch, Nv12Geom g, Nv12Coef k,
                                                               const int64_t* __restrict__ offsets, const int32_t* __restrict__ starts, int n_clips,
                                                               int64_t capacity, int tiles_per_frame, int chunks, int st,
                                                               uint8_t* __restrict__ out, int32_t* __restrict__ src_index) {
    const int64_t total = offsets[n_clips];
    const int64_t n = total < capacity ? total : capacity;
    const int per_frame = (g.H0 >> 1) * chunks;
    const int64_t out_bytes = (int64_t)g.H0 * g.W0 * 3;
    for (int64_t tile = blockIdx.x; tile < n * tiles_per_frame; tile += gridDim.x) {
        const int64_t kf = tile / tiles_per_frame;
        const int part = (int)(tile % tiles_per_frame);
        int lo = 0, hi = n_clips;                                        // offsets[lo] <= kf < offsets[hi]
        while (hi - lo > 1) {
            const int mid = (lo + hi) >> 1;
            if (offsets[mid] <= kf) lo = mid; else hi = mid;
        }
        const int64_t src = (int64_t)starts[lo] + (kf - offsets[lo]);
        if (part == 0 && threadIdx.x == 0) src_index[kf] = (int32_t)src;
        const int item = part * 256 + (int)threadIdx.x;
        if (item < per_frame) nv12_block_to_bgr<VEC>(frames + src * frame_pitch, out + kf * out_bytes, g, k, chunks, item, st);
    }
}

int nv12_store_mode(const uint8_t* out, int W0) {
    if (W0 % 16 == 0 && aligned16(out)) return ST_VECTORS;
    if (W0 % 4 == 0 && (reinterpret_cast<uintptr_t>(out) & 3u) == 0) return ST_WORDS;
    return ST_BYTES;
}

}  // namespace

extern "C" {

int goalnet_nv12_to_bgr(const uint8_t* frames, int n, int H0, int W0, int64_t pitch, int64_t uv_offset, int64_t frame_pitch,
                        const int32_t* coeffs, uint8_t* out_hwc, void* stream) {
    GN_REQUIRE(frames && coeffs && out_hwc, GOALNET_E_NULL, "nv12_to_bgr: null pointer");
    GN_REQUIRE(n >= 1, GOALNET_E_SHAPE, "nv12_to_bgr: n must be >= 1");
    Nv12Geom g;
    Nv12Coef k;
    const int rc = nv12_args("nv12_to_bgr", H0, W0, pitch, uv_offset, frame_pitch, coeffs, &g, &k);
    if (rc) return rc;
    hipStream_t st = (hipStream_t)stream;
    const int chunks = (W0 + 15) / 16;
    const int64_t total = (int64_t)n * (H0 / 2) * chunks;
    const int64_t want = (total + 255) / 256;
    const dim3 grid((unsigned)(want < 2048 ? want : 2048));             // memory-bound: ~8 blocks per CU, stride over the rest
    const int mode = nv12_store_mode(out_hwc, W0);
    if (nv12_rows_aligned(frames, pitch, uv_offset, frame_pitch))
        hipLaunchKernelGGL(nv12_to_bgr_kernel<true>, grid, dim3(256), 0, st, frames, frame_pitch, g, k, out_hwc, total, chunks, mode);
    else
        hipLaunchKernelGGL(nv12_to_bgr_kernel<false>, grid, dim3(256), 0, st, frames, frame_pitch, g, k, out_hwc, total, chunks, mode);
    GN_LAUNCH_CHECK("nv12_to_bgr");
    return 0;
}

int goalnet_nv12_preprocess_strided(const uint8_t* frames, int n_total, int frame_stride, int H0, int W0, int64_t pitch,
                                    int64_t uv_offset, int64_t frame_pitch, const int32_t* coeffs, float* out_nchw, int H, int W,
                                    int32_t* minmax, void* stream) {
    GN_REQUIRE(frames && coeffs && out_nchw && minmax, GOALNET_E_NULL, "nv12_preprocess_strided: null pointer");
    GN_REQUIRE(n_total >= 1, GOALNET_E_SHAPE, "nv12_preprocess_strided: n_total must be >= 1");
    GN_REQUIRE(frame_stride >= 1, GOALNET_E_SHAPE, "nv12_preprocess_strided: frame_stride must be >= 1");
    GN_REQUIRE(H > 0 && W > 0, GOALNET_E_SHAPE, "nv12_preprocess_strided: non-positive dim");
    Nv12Geom g;
    Nv12Coef k;
    const int rc = nv12_args("nv12_preprocess_strided", H0, W0, pitch, uv_offset, frame_pitch, coeffs, &g, &k);
    if (rc) return rc;
    hipStream_t st = (hipStream_t)stream;
    const int n = (int)(((int64_t)n_total + frame_stride - 1) / frame_stride);      // frames 0, stride, 2 stride, ... < n_total
    const int64_t sample_pitch = frame_pitch * frame_stride;
    const int chunks = (W0 + 15) / 16;
    const int items = (H0 / 2) * chunks;
    hipLaunchKernelGGL(nv12_minmax_init_kernel, dim3((n + 255) / 256), dim3(256), 0, st, minmax, n);
    GN_LAUNCH_CHECK("nv12_preprocess_strided.init");
    // ~2048 blocks in all, and at least 512 blocks of 2 x 16 pixels (24 KB of loads) per thread block
    int64_t bpf = (2048 + n - 1) / n;
    const int64_t by_size = (items + 511) / 512;
    bpf = bpf < by_size ? bpf : by_size;
    bpf = bpf < 1 ? 1 : bpf;
    const dim3 grid((unsigned)(n * bpf));
    if (nv12_rows_aligned(frames, pitch, uv_offset, sample_pitch))
        hipLaunchKernelGGL(nv12_minmax_strided_kernel<true>, grid, dim3(256), 0, st, frames, sample_pitch, g, k, chunks, (int)bpf, minmax);
    else
        hipLaunchKernelGGL(nv12_minmax_strided_kernel<false>, grid, dim3(256), 0, st, frames, sample_pitch, g, k, chunks, (int)bpf, minmax);
    GN_LAUNCH_CHECK("nv12_preprocess_strided.minmax");
    hipLaunchKernelGGL(nv12_resize_strided_kernel, dim3(resize_blocks((int64_t)n * 3 * H * W)), dim3(256), 0, st, frames, sample_pitch, g, k,
                       (const int32_t*)minmax, out_nchw, n, H, W, resize_scale(W, W0), resize_scale(H, H0));
    GN_LAUNCH_CHECK("nv12_preprocess_strided.resize");
    return 0;
}

size_t goalnet_nv12_gather_clips_bgr_ws_bytes(int n_clips) {
    if (n_clips < 0) return 0;
    return offsets_bytes(n_clips) + align256((size_t)n_clips * sizeof(int32_t));
}

int goalnet_nv12_gather_clips_bgr(const uint8_t* frames, int full_n, int H0, int W0, int64_t pitch, int64_t uv_offset,
                                  int64_t frame_pitch, const int32_t* coeffs, const int32_t* change_points, const int32_t* selected,
                                  int n_clips, uint8_t* out, int64_t out_capacity_frames, int32_t* src_index, int64_t* count,
                                  int32_t* status, void* ws, size_t ws_bytes, void* stream) {
    GN_REQUIRE(frames && coeffs && change_points && selected && out && src_index && count && status && ws, GOALNET_E_NULL,
               "nv12_gather_clips_bgr: null pointer");
    GN_REQUIRE(full_n >= 1, GOALNET_E_SHAPE, "nv12_gather_clips_bgr: full_n must be >= 1");
    GN_REQUIRE(n_clips >= 1 && out_capacity_frames >= 0, GOALNET_E_SHAPE, "nv12_gather_clips_bgr: need n_clips >= 1 and out_capacity_frames >= 0");
    Nv12Geom g;
    Nv12Coef k;
    const int rc = nv12_args("nv12_gather_clips_bgr", H0, W0, pitch, uv_offset, frame_pitch, coeffs, &g, &k);
    if (rc) return rc;
    GN_REQUIRE(ws_bytes >= goalnet_nv12_gather_clips_bgr_ws_bytes(n_clips), GOALNET_E_WORKSPACE, "nv12_gather_clips_bgr: workspace too small");
    hipStream_t st = (hipStream_t)stream;
    int64_t* offsets = (int64_t*)ws;
    int32_t* starts = (int32_t*)((char*)ws + offsets_bytes(n_clips));
    hipLaunchKernelGGL(clip_offsets_kernel, dim3(1), dim3(256), 0, st, change_points, selected, n_clips, full_n, out_capacity_frames, offsets,
                       starts, count, status);
    GN_LAUNCH_CHECK("nv12_gather_clips_bgr.offsets");
    if (out_capacity_frames == 0) return 0;
    const int chunks = (W0 + 15) / 16;
    const int tpf = ((H0 / 2) * chunks + 255) / 256;
    const int64_t tiles = out_capacity_frames > INT64_MAX / tpf ? INT64_MAX : out_capacity_frames * tpf;
    const dim3 grid((unsigned)(tiles < 2048 ? tiles : 2048));           // memory-bound: ~8 blocks per CU, stride over the rest
    const int mode = nv12_store_mode(out, W0);
    if (nv12_rows_aligned(frames, pitch, uv_offset, frame_pitch))
        hipLaunchKernelGGL(nv12_gather_clips_kernel<true>, grid, dim3(256), 0, st, frames, frame_pitch, g, k, (const int64_t*)offsets,
                           (const int32_t*)starts, n_clips, out_capacity_frames, tpf, chunks, mode, out, src_index);
    else
        hipLaunchKernelGGL(nv12_gather_clips_kernel<false>, grid, dim3(256), 0, st, frames, frame_pitch, g, k, (const int64_t*)offsets,
                           (const int32_t*)starts, n_clips, out_capacity_frames, tpf, chunks, mode, out, src_index);
    GN_LAUNCH_CHECK("nv12_gather_clips_bgr.copy");
    return 0;
}

}  // extern "C"
