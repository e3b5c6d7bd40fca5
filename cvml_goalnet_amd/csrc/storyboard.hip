// The static summary of a video (include/goalnet_storyboard.h; EXTENSION, the keyframe choice and the box filter are defined there):
//   goalnet_storyboard_keyframes      one frame per chosen clip: the sampled frame with the highest importance
//   goalnet_storyboard_render         the named frames of a resident BGR video -> thumbnails and / or a contact sheet
//   goalnet_storyboard_render_nv12    the same from NV12 frames, converted on the way into the staging buffer
// The render is HBM-traffic work on bytes: every named frame is read once. A work item is (keyframe, output row, tile of <= 256
// output columns); the source rows that output row overlaps are staged through LDS, a piece of <= SB_CHUNK_PX columns and as many
// rows as fit at a time, as packed BGR bytes. BGR rows are copied in aligned 16-byte windows (a window that sticks out of the piece is
// copied byte by byte, so nothing outside the piece is read, whatever the alignment of base and rows); NV12 rows are loaded in
// groups of 16 pixels (16-byte loads where the row starts allow, only the W0 picture bytes of a row otherwise) and converted with
// nv12_pixel.h's pixel before they are stored. Thread t then owns output column j0 + t of the item and sums its weighted columns
// of every staged row.
// Integer widths (H0, W0, th, tw <= GOALNET_STORYBOARD_MAX_DIM = 2^14, checked by the host):
//   i H0, r th, j W0, c tw and the weights          <= 2^28                                int32
//   a row's sum  h = sum_c wx p                     <= 255 W0 < 2^22   (sum_c wx = W0)      uint32
//   wy h <= 2^14 * 2^22 and the pixel's sum         <= 255 H0 W0 + H0 W0 / 2 < 2^37         uint64
// The last division is done in 32 bits when 255 H0 W0 + H0 W0 / 2 < 2^32 (the host decides), in 64 bits otherwise.
#include "common.h"
#include "clip_scan.h"
#include "nv12_pixel.h"
#include "../../include/goalnet_storyboard.h"

using namespace goalnet;

namespace {

constexpr int SB_THREADS = 256;
constexpr int SB_CHUNK_PX = 1024;                                       // columns of a staged piece
constexpr int SB_STAGE_BYTES = 8 * (SB_CHUNK_PX + 32) * 3;              // 8 rows of a full piece (25 344 B: 6 blocks per CU)

// bytes between staged rows for a piece of cw columns: room for the piece plus 15 bytes (BGR: the source's misalignment) or plus 30
// columns (NV12: groups of 16 columns around it); a multiple of 48
__host__ __device__ __forceinline__ int sb_row_stride(int cw) { return ((cw + 31) >> 4 << 4) * 3; }

struct SbShape {
    int H0, W0, th, tw, full_n;
    int ntiles, jt;                 // tiles of output columns per row, columns per tile (<= SB_THREADS)
    int cols, gap;
    int64_t Ws;                     // the sheet's width in pixels
    int narrow;                     // 255 H0 W0 + H0 W0 / 2 < 2^32
};

// rows rb .. rb + nr - 1, columns c0 .. c0 + cw - 1 of the BGR frame f -> stage; source byte b of a row lands at row * rs + off + b
// with off = the row's address mod 16. Returns nothing: the reader recomputes off.
__device__ __forceinline__ void sb_stage_bgr(const uint8_t* __restrict__ f, int W0, int rb, int nr, int c0, int cw, int rs, uint8_t* stage) {
    const int nbytes = cw * 3;
    const int slots = (nbytes + 30) >> 4;                               // 16-byte windows that can meet off + [0, nbytes), off <= 15
    for (int idx = threadIdx.x; idx < nr * slots; idx += SB_THREADS) {
        const int rr = idx / slots, s = idx - rr * slots;
        const uint8_t* src = f + ((int64_t)(rb + rr) * W0 + c0) * 3;
        const int off = (int)(reinterpret_cast<uintptr_t>(src) & 15u);
        const int lo = 16 * s - off;                                    // the window's first byte, relative to the piece
        uint8_t* dst = stage + rr * rs + 16 * s;
        if (lo >= 0 && lo + 16 <= nbytes) {
            *reinterpret_cast<uint4*>(dst) = *reinterpret_cast<const uint4*>(src + lo);
        } else {
#pragma unroll
            for (int b = 0; b < 16; ++b)
                if (lo + b >= 0 && lo + b < nbytes) dst[b] = src[lo + b];
        }
    }
}

// the same rows of the NV12 frame f, converted: columns xg0 = c0 & ~15 onwards in groups of 16; pixel x of a row lands at
// row * rs + (x - xg0) * 3. Only picture bytes (x < W0) are loaded; what a partial group leaves behind them is never read.
template <bool VEC>
__device__ __forceinline__ void sb_stage_nv12(const uint8_t* __restrict__ f, const Nv12Geom& g, const Nv12Coef& k, int rb, int nr, int c0, int cw,
                                              int rs, uint8_t* stage) {
    const int xg0 = c0 & ~15;
    const int groups = (c0 + cw - xg0 + 15) >> 4;
    for (int idx = threadIdx.x; idx < nr * groups; idx += SB_THREADS) {
        const int rr = idx / groups, gi = idx - rr * groups;
        const int y = rb + rr, x0 = xg0 + 16 * gi;
        const int cnt = g.W0 - x0 < 16 ? g.W0 - x0 : 16;                 // even: W0 and x0 are
        const uint8_t* py = f + (int64_t)y * g.pitch + x0;
        const uint8_t* pc = f + g.uv_offset + (int64_t)(y >> 1) * g.pitch + x0;
        uint32_t yw[4], uv[4], o[12];
        if (VEC && cnt == 16) {
            const uint4 a = *reinterpret_cast<const uint4*>(py), c = *reinterpret_cast<const uint4*>(pc);
            yw[0] = a.x; yw[1] = a.y; yw[2] = a.z; yw[3] = a.w;
            uv[0] = c.x; uv[1] = c.y; uv[2] = c.z; uv[3] = c.w;
        } else {
#pragma unroll
            for (int w = 0; w < 4; ++w) yw[w] = uv[w] = 0u;
#pragma unroll
            for (int b = 0; b < 16; ++b) {
                if (b < cnt) {
                    yw[b >> 2] |= (uint32_t)py[b] << (8 * (b & 3));
                    uv[b >> 2] |= (uint32_t)pc[b] << (8 * (b & 3));
                }
            }
        }
#pragma unroll
        for (int w = 0; w < 12; ++w) o[w] = 0u;
#pragma unroll
        for (int p = 0; p < 16; ++p) {
            const int Y = (int)((yw[p >> 2] >> (8 * (p & 3))) & 255u);
            const uint32_t pair = uv[p >> 2] >> (16 * ((p >> 1) & 1));
            const int U = (int)(pair & 255u), V = (int)((pair >> 8) & 255u);
#pragma unroll
            for (int ch = 0; ch < 3; ++ch) {
                int v = nv12_channel_of(k, Y, U, V, ch);
                // Keeps the clamp and the packing apart. Without it hipcc fuses sat8(x >> s) | sat8(y >> s) << 8 of two neighbouring
                // bytes into one v_ashr_pk_u8_i32, and the words it built with that came out of the MI355X with too many bits set
                // (every thumbnail too bright; nv12.hip, whose code holds no such instruction, converts the same pixels right).
                asm("" : "+v"(v));
                o[(3 * p + ch) >> 2] |= (uint32_t)v << (8 * ((3 * p + ch) & 3));
            }
        }
        uint4* dst = reinterpret_cast<uint4*>(stage + rr * rs + gi * 48);
        dst[0] = make_uint4(o[0], o[1], o[2], o[3]);
        dst[1] = make_uint4(o[4], o[5], o[6], o[7]);
        dst[2] = make_uint4(o[8], o[9], o[10], o[11]);
    }
}

template <bool NV12, bool VEC>
__global__ __launch_bounds__(SB_THREADS) void storyboard_render_kernel(const uint8_t* __restrict__ frames, int64_t frame_pitch, Nv12Geom g, Nv12Coef k,
                                                                      const int32_t* __restrict__ frame_index, SbShape s, int64_t total,
                                                                      uint8_t* __restrict__ thumbs, uint8_t* __restrict__ sheet) {
    __shared__ uint4 stage4[SB_STAGE_BYTES / 16];
    uint8_t* stage = reinterpret_cast<uint8_t*>(stage4);
    const int t = threadIdx.x;
    const int H0 = s.H0, W0 = s.W0, th = s.th, tw = s.tw;
    for (int64_t item = blockIdx.x; item < total; item += gridDim.x) {
        const int tile = (int)(item % s.ntiles);
        const int64_t q = item / s.ntiles;
        const int i = (int)(q % th), kf = (int)(q / th);
        int src = frame_index[kf];
        src = src < 0 ? 0 : (src > s.full_n - 1 ? s.full_n - 1 : src);
        const uint8_t* f = frames + (int64_t)src * frame_pitch;
        // the source rows output row i overlaps, the source columns the tile's output columns overlap, and my own columns
        const int r0 = i * H0 / th, r1 = ((i + 1) * H0 + th - 1) / th;
        const int j0 = tile * s.jt, j1 = j0 + s.jt < tw ? j0 + s.jt : tw;
        const int cs = j0 * W0 / tw, ce = (j1 * W0 + tw - 1) / tw;
        const int j = j0 + t;
        const bool own = j < j1;
        const int jlo = j * W0, jhi = jlo + W0;                          // own: j < tw, so jhi <= tw W0 <= 2^28
        const int mc0 = own ? jlo / tw : 0, mc1 = own ? (jhi + tw - 1) / tw : 0;
        uint64_t acc0 = 0, acc1 = 0, acc2 = 0;
        for (int c0 = cs; c0 < ce; c0 += SB_CHUNK_PX) {
            const int c1 = c0 + SB_CHUNK_PX < ce ? c0 + SB_CHUNK_PX : ce;
            const int rs = sb_row_stride(c1 - c0);
            const int fit = SB_STAGE_BYTES / rs;                         // >= 8
            for (int rb = r0; rb < r1; rb += fit) {
                const int nr = r1 - rb < fit ? r1 - rb : fit;
                __syncthreads();                                         // the previous piece has been read
                if (NV12) sb_stage_nv12<VEC>(f, g, k, rb, nr, c0, c1 - c0, rs, stage);
                else sb_stage_bgr(f, W0, rb, nr, c0, c1 - c0, rs, stage);
                __syncthreads();
                const int a = mc0 > c0 ? mc0 : c0, b = mc1 < c1 ? mc1 : c1;
                if (a < b) {
                    for (int rr = 0; rr < nr; ++rr) {
                        const int r = rb + rr;
                        const int ylo = i * H0 > r * th ? i * H0 : r * th, yhi = (i + 1) * H0 < (r + 1) * th ? (i + 1) * H0 : (r + 1) * th;
                        const int wy = yhi - ylo;                        // > 0: r0 <= r < r1
                        int shift;
                        if (NV12) shift = (c0 - (c0 & ~15)) * 3;
                        else shift = (int)(reinterpret_cast<uintptr_t>(f + ((int64_t)r * W0 + c0) * 3) & 15u);
                        const uint8_t* row = stage + rr * rs + shift;
                        uint32_t h0 = 0, h1 = 0, h2 = 0;
                        for (int c = a; c < b; ++c) {
                            const int xlo = jlo > c * tw ? jlo : c * tw, xhi = jhi < (c + 1) * tw ? jhi : (c + 1) * tw;
                            const uint32_t wx = (uint32_t)(xhi - xlo);
                            const uint8_t* p = row + (c - c0) * 3;
                            h0 += wx * p[0];
                            h1 += wx * p[1];
                            h2 += wx * p[2];
                        }
                        acc0 += (uint64_t)wy * h0;
                        acc1 += (uint64_t)wy * h1;
                        acc2 += (uint64_t)wy * h2;
                    }
                }
            }
        }
        if (own) {
            const uint64_t area = (uint64_t)H0 * W0, half = area >> 1;
            uint8_t v0, v1, v2;
            if (s.narrow) {
                const uint32_t a32 = (uint32_t)area;
                v0 = (uint8_t)((uint32_t)(acc0 + half) / a32);
                v1 = (uint8_t)((uint32_t)(acc1 + half) / a32);
                v2 = (uint8_t)((uint32_t)(acc2 + half) / a32);
            } else {
                v0 = (uint8_t)((acc0 + half) / area);
                v1 = (uint8_t)((acc1 + half) / area);
                v2 = (uint8_t)((acc2 + half) / area);
            }
            if (thumbs) {
                uint8_t* d = thumbs + (((int64_t)kf * th + i) * tw + j) * 3;
                d[0] = v0; d[1] = v1; d[2] = v2;
            }
            if (sheet) {
                const int64_t y = s.gap + (int64_t)(kf / s.cols) * (th + s.gap) + i, x = s.gap + (int64_t)(kf % s.cols) * (tw + s.gap) + j;
                uint8_t* d = sheet + (y * s.Ws + x) * 3;
                d[0] = v0; d[1] = v1; d[2] = v2;
            }
        }
    }
}

__global__ __launch_bounds__(256) void storyboard_background_kernel(uint8_t* __restrict__ sheet, int64_t pixels, uint8_t b, uint8_t g, uint8_t r) {
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < pixels; i += (int64_t)gridDim.x * 256) {
        sheet[3 * i] = b;
        sheet[3 * i + 1] = g;
        sheet[3 * i + 2] = r;
    }
}

__device__ __forceinline__ float sb_key(float p) { return p != p ? -INFINITY : p; }

// One block; thread t owns the clips [t per, (t + 1) per). Pass 1: every clip's keyframe; pass 2 (only when max_keyframes cuts): an
// entry stays when fewer than max_keyframes entries beat it; pass 3: a scan of the survivors puts them out in clip order.
__global__ __launch_bounds__(256) void storyboard_keyframes_kernel(const float* __restrict__ pred, int n_sampled, int skip, int full_n,
                                                                  const int32_t* __restrict__ cps, const int32_t* __restrict__ flags, int n_clips,
                                                                  int max_keyframes, int32_t* __restrict__ frame_index, int32_t* __restrict__ clip,
                                                                  float* __restrict__ score, int capacity, int32_t* __restrict__ count) {
    __shared__ int s_frame[GOALNET_STORYBOARD_MAX_CLIPS];
    __shared__ float s_score[GOALNET_STORYBOARD_MAX_CLIPS];
    __shared__ int s_on[GOALNET_STORYBOARD_MAX_CLIPS];
    __shared__ int s_scan[256];
    const int t = threadIdx.x;
    const int per = (n_clips + 255) / 256;                               // <= 16
    const int lo = t * per < n_clips ? t * per : n_clips, hi = lo + per < n_clips ? lo + per : n_clips;
    for (int c = lo; c < hi; ++c) {
        int a, b;
        clip_slice(cps, c, full_n, a, b);
        const bool on = (flags == nullptr || flags[c] != 0) && b > a;
        int frame = 0;
        float best = 0.f;
        if (on) {
            const int64_t jl = ((int64_t)a + skip - 1) / skip;
            int64_t jh = ((int64_t)b + skip - 1) / skip;
            jh = jh < n_sampled ? jh : n_sampled;
            if (jl < jh) {
                int64_t bj = jl;
                best = sb_key(pred[jl]);
                for (int64_t j = jl + 1; j < jh; ++j) {
                    const float kj = sb_key(pred[j]);
                    if (kj > best) { best = kj; bj = j; }
                }
                frame = (int)(bj * skip);                                // < b <= full_n
            } else {
                frame = a + (b - a) / 2;
                const int qs = frame / skip;
                best = sb_key(pred[qs < n_sampled - 1 ? qs : n_sampled - 1]);
            }
        }
        s_frame[c] = frame;
        s_score[c] = best;
        s_on[c] = on ? 1 : 0;
    }
    __syncthreads();
    auto block_scan = [&](int local) -> int {                            // inclusive scan of `local` over the threads; s_scan[255] = total
        s_scan[t] = local;
        __syncthreads();
        for (int o = 1; o < 256; o <<= 1) {
            const int v = t >= o ? s_scan[t - o] : 0;
            __syncthreads();
            s_scan[t] += v;
            __syncthreads();
        }
        return s_scan[t];
    };
    int mine = 0;
    for (int c = lo; c < hi; ++c) mine += s_on[c];
    int incl = block_scan(mine);
    const int found = s_scan[255];
    if (max_keyframes > 0 && found > max_keyframes) {
        unsigned keep = 0u;
        for (int c = lo; c < hi; ++c) {
            if (!s_on[c]) continue;
            const float sc = s_score[c];
            int beat = 0;                                                // entries in front of c: a higher score, or the same from a lower clip
            for (int d = 0; d < n_clips; ++d) beat += (s_on[d] && (s_score[d] > sc || (s_score[d] == sc && d < c))) ? 1 : 0;
            if (beat < max_keyframes) keep |= 1u << (c - lo);
        }
        __syncthreads();                                                 // everyone has read s_on and s_scan[255]
        mine = 0;
        for (int c = lo; c < hi; ++c) {
            s_on[c] = (keep >> (c - lo)) & 1u;
            mine += s_on[c];
        }
        incl = block_scan(mine);
    }
    int pos = incl - mine;
    for (int c = lo; c < hi; ++c) {
        if (!s_on[c]) continue;
        if (pos < capacity) {
            frame_index[pos] = s_frame[c];
            clip[pos] = c;
            score[pos] = s_score[c];
        }
        ++pos;
    }
    if (t == 255) *count = s_scan[255];
}

int render_args(const char* who, const void* frames, const void* frame_index, const void* thumbs, const void* sheet, int full_n, int H0, int W0, int K,
                int th, int tw, int cols, int gap, int bg_b, int bg_g, int bg_r, SbShape* s, int64_t* Hs) {
    GN_REQUIRE(frames && frame_index, GOALNET_E_NULL, "%s: null pointer", who);
    GN_REQUIRE(thumbs || sheet, GOALNET_E_NULL, "%s: thumbs and sheet are both null", who);
    GN_REQUIRE(full_n >= 1 && K >= 1, GOALNET_E_SHAPE, "%s: full_n = %d and K = %d must be >= 1", who, full_n, K);
    const int M = GOALNET_STORYBOARD_MAX_DIM;
    GN_REQUIRE(H0 >= 1 && W0 >= 1 && H0 <= M && W0 <= M, GOALNET_E_SHAPE, "%s: H0 = %d, W0 = %d outside 1 .. %d", who, H0, W0, M);
    GN_REQUIRE(th >= 1 && tw >= 1 && th <= M && tw <= M, GOALNET_E_SHAPE, "%s: th = %d, tw = %d outside 1 .. %d", who, th, tw, M);
    *s = SbShape{};
    *Hs = 0;
    if (sheet) {
        GN_REQUIRE(cols >= 1 && gap >= 0, GOALNET_E_SHAPE, "%s: a sheet needs cols >= 1 and gap >= 0 (cols = %d, gap = %d)", who, cols, gap);
        const int64_t rows = ((int64_t)K + cols - 1) / cols;
        *Hs = gap + rows * ((int64_t)th + gap);
        s->Ws = gap + (int64_t)cols * ((int64_t)tw + gap);
        GN_REQUIRE(*Hs <= INT32_MAX && s->Ws <= INT32_MAX, GOALNET_E_SHAPE, "%s: a sheet of %lld x %lld pixels is too large", who, (long long)*Hs,
                   (long long)s->Ws);
        GN_REQUIRE(bg_b >= 0 && bg_b <= 255 && bg_g >= 0 && bg_g <= 255 && bg_r >= 0 && bg_r <= 255, GOALNET_E_VALUE,
                   "%s: background (%d, %d, %d) outside 0 .. 255", who, bg_b, bg_g, bg_r);
        s->cols = cols;
        s->gap = gap;
    } else {
        s->cols = 1;
    }
    s->H0 = H0; s->W0 = W0; s->th = th; s->tw = tw; s->full_n = full_n;
    s->ntiles = (tw + SB_THREADS - 1) / SB_THREADS;
    s->jt = (tw + s->ntiles - 1) / s->ntiles;
    const uint64_t area = (uint64_t)H0 * W0;
    s->narrow = 255 * area + area / 2 < ((uint64_t)1 << 32) ? 1 : 0;
    return 0;
}

template <bool NV12>
int render_launch(const char* who, const uint8_t* frames, int64_t frame_pitch, const Nv12Geom& g, const Nv12Coef& k, bool vec, const int32_t* frame_index,
                  const SbShape& s, int K, int64_t Hs, uint8_t* thumbs, uint8_t* sheet, int bg_b, int bg_g, int bg_r, hipStream_t st) {
    if (sheet) {
        const int64_t pixels = Hs * s.Ws;
        const int64_t want = (pixels + 255) / 256;
        hipLaunchKernelGGL(storyboard_background_kernel, dim3((unsigned)(want < 2048 ? (want < 1 ? 1 : want) : 2048)), dim3(256), 0, st, sheet, pixels,
                           (uint8_t)bg_b, (uint8_t)bg_g, (uint8_t)bg_r);
        GN_LAUNCH_CHECK(who);
    }
    const int64_t total = (int64_t)K * s.th * s.ntiles;
    const dim3 grid((unsigned)(total < (1 << 20) ? total : (1 << 20)));  // one item per block; a block strides over the rest
    if (vec)
        hipLaunchKernelGGL((storyboard_render_kernel<NV12, true>), grid, dim3(SB_THREADS), 0, st, frames, frame_pitch, g, k, frame_index, s, total,
                           thumbs, sheet);
    else
        hipLaunchKernelGGL((storyboard_render_kernel<NV12, false>), grid, dim3(SB_THREADS), 0, st, frames, frame_pitch, g, k, frame_index, s, total,
                           thumbs, sheet);
    GN_LAUNCH_CHECK(who);
    return 0;
}

}  // namespace

extern "C" {

int goalnet_storyboard_keyframes(const float* pred, int n_sampled, int skip, int full_n, const int32_t* change_points, const int32_t* flags,
                                 int n_clips, int max_keyframes, int32_t* frame_index, int32_t* clip, float* score, int capacity, int32_t* count,
                                 void* stream) {
    GN_REQUIRE(pred && change_points && frame_index && clip && score && count, GOALNET_E_NULL, "storyboard_keyframes: null pointer");
    GN_REQUIRE(n_sampled >= 1 && skip >= 1 && full_n >= 1, GOALNET_E_SHAPE, "storyboard_keyframes: n_sampled, skip and full_n must be >= 1");
    GN_REQUIRE(capacity >= 1, GOALNET_E_SHAPE, "storyboard_keyframes: capacity must be >= 1");
    GN_REQUIRE(n_clips >= 1 && n_clips <= GOALNET_STORYBOARD_MAX_CLIPS, GOALNET_E_SHAPE, "storyboard_keyframes: n_clips = %d outside 1 .. %d", n_clips,
               GOALNET_STORYBOARD_MAX_CLIPS);
    hipLaunchKernelGGL(storyboard_keyframes_kernel, dim3(1), dim3(256), 0, (hipStream_t)stream, pred, n_sampled, skip, full_n, change_points, flags,
                       n_clips, max_keyframes, frame_index, clip, score, capacity, count);
    GN_LAUNCH_CHECK("storyboard_keyframes");
    return 0;
}

int goalnet_storyboard_render(const uint8_t* frames, int full_n, int H0, int W0, const int32_t* frame_index, int K, int th, int tw,
                              uint8_t* thumbs, uint8_t* sheet, int cols, int gap, int bg_b, int bg_g, int bg_r, void* stream) {
    SbShape s;
    int64_t Hs;
    const int rc = render_args("storyboard_render", frames, frame_index, thumbs, sheet, full_n, H0, W0, K, th, tw, cols, gap, bg_b, bg_g, bg_r, &s, &Hs);
    if (rc) return rc;
    return render_launch<false>("storyboard_render", frames, (int64_t)H0 * W0 * 3, Nv12Geom{}, Nv12Coef{}, false, frame_index, s, K, Hs, thumbs, sheet,
                                bg_b, bg_g, bg_r, (hipStream_t)stream);
}

int goalnet_storyboard_render_nv12(const uint8_t* frames, int full_n, int H0, int W0, int64_t pitch, int64_t uv_offset, int64_t frame_pitch,
                                   const int32_t* coeffs, const int32_t* frame_index, int K, int th, int tw, uint8_t* thumbs, uint8_t* sheet,
                                   int cols, int gap, int bg_b, int bg_g, int bg_r, void* stream) {
    GN_REQUIRE(coeffs, GOALNET_E_NULL, "storyboard_render_nv12: null pointer");
    SbShape s;
    int64_t Hs;
    int rc = render_args("storyboard_render_nv12", frames, frame_index, thumbs, sheet, full_n, H0, W0, K, th, tw, cols, gap, bg_b, bg_g, bg_r, &s, &Hs);
    if (rc) return rc;
    Nv12Geom g;
    Nv12Coef k;
    rc = nv12_args("storyboard_render_nv12", H0, W0, pitch, uv_offset, frame_pitch, coeffs, &g, &k);
    if (rc) return rc;
    return render_launch<true>("storyboard_render_nv12", frames, frame_pitch, g, k, nv12_rows_aligned(frames, pitch, uv_offset, frame_pitch),
                               frame_index, s, K, Hs, thumbs, sheet, bg_b, bg_g, bg_r, (hipStream_t)stream);
}

}  // extern "C"
