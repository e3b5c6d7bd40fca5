// The NV12 pixel of include/goalnet_nv12.h, shared by the files that read NV12 frames (nv12.hip, storyboard.hip): the frame geometry,
// the colour table, the per-pixel conversion and the host check of both. One formulation, so the files agree by construction.
// File-local names (an unnamed namespace, as they were in nv12.hip): the two structs are kernel arguments, and a kernel's symbol
// carries its argument types.
#pragma once
#include "common.h"
#include "../../include/goalnet_nv12.h"

namespace {

struct Nv12Geom { int H0, W0; int64_t pitch, uv_offset; };
struct Nv12Coef { int y_off, cy, cub, cug, cvg, cvr, shift, r0; };

__device__ __forceinline__ int sat8(int x) { return x < 0 ? 0 : (x > 255 ? 255 : x); }

// channel c (0 = B, 1 = G, 2 = R) of a pixel with luma byte Y and chroma bytes U, V
__device__ __forceinline__ int nv12_channel_of(const Nv12Coef& k, int Y, int U, int V, int c) {
    const int u = U - 128, v = V - 128;
    const int d = Y - k.y_off;
    const int yy = (d < 0 ? 0 : d) * k.cy;
    const int chroma = c == 0 ? k.cub * u : (c == 1 ? k.cug * u + k.cvg * v : k.cvr * v);
    return sat8((yy + chroma + k.r0) >> k.shift);
}

// channel c (0 = B, 1 = G, 2 = R) of pixel (y, x)
__device__ __forceinline__ int nv12_channel(const uint8_t* __restrict__ f, const Nv12Geom& g, const Nv12Coef& k, int y, int x, int c) {
    const int Y = f[(int64_t)y * g.pitch + x];
    const uint8_t* uv = f + g.uv_offset + (int64_t)(y >> 1) * g.pitch + ((x >> 1) << 1);
    return nv12_channel_of(k, Y, uv[0], uv[1], c);
}

// the layout rules and the table of goalnet_nv12.h; 0 or the negative code (message set)
inline int nv12_args(const char* who, int H0, int W0, int64_t pitch, int64_t uv_offset, int64_t frame_pitch, const int32_t* c, Nv12Geom* g, Nv12Coef* k) {
    GN_REQUIRE(H0 >= 2 && W0 >= 2 && H0 % 2 == 0 && W0 % 2 == 0, GOALNET_E_SHAPE, "%s: H0 = %d and W0 = %d must be even and positive", who, H0, W0);
    GN_REQUIRE(pitch >= W0, GOALNET_E_SHAPE, "%s: pitch = %lld < W0 = %d", who, (long long)pitch, W0);
    GN_REQUIRE(pitch <= ((int64_t)1 << 31), GOALNET_E_SHAPE, "%s: pitch = %lld > 2^31", who, (long long)pitch);
    GN_REQUIRE(uv_offset >= (int64_t)H0 * pitch, GOALNET_E_SHAPE, "%s: uv_offset = %lld < H0 * pitch = %lld", who, (long long)uv_offset,
               (long long)((int64_t)H0 * pitch));
    GN_REQUIRE(uv_offset <= ((int64_t)1 << 60) && frame_pitch >= uv_offset + (int64_t)(H0 / 2 - 1) * pitch + W0, GOALNET_E_SHAPE,
               "%s: frame_pitch = %lld < uv_offset + (H0 / 2 - 1) * pitch + W0 = %lld", who, (long long)frame_pitch,
               (long long)(uv_offset + (int64_t)(H0 / 2 - 1) * pitch + W0));
    GN_REQUIRE((int64_t)(H0 / 2) * ((W0 + 15) / 16) <= INT32_MAX - 256, GOALNET_E_SHAPE, "%s: %d x %d frames are too large", who, H0, W0);
    const int shift = c[6];
    GN_REQUIRE(shift >= GOALNET_NV12_MIN_SHIFT && shift <= GOALNET_NV12_MAX_SHIFT, GOALNET_E_VALUE, "%s: shift = %d outside %d .. %d", who, shift,
               GOALNET_NV12_MIN_SHIFT, GOALNET_NV12_MAX_SHIFT);
    GN_REQUIRE(c[0] >= 0 && c[0] <= 255, GOALNET_E_VALUE, "%s: y_off = %d outside 0 .. 255", who, c[0]);
    auto mag = [](int32_t v) -> int64_t { return v < 0 ? -(int64_t)v : (int64_t)v; };
    const int64_t worst = 255 * mag(c[1]) + 128 * (mag(c[2]) + mag(c[3]) + mag(c[4]) + mag(c[5])) + ((int64_t)1 << (shift - 1));
    GN_REQUIRE(worst < ((int64_t)1 << 31), GOALNET_E_VALUE,
               "%s: 255 |cy| + 128 (|cub| + |cug| + |cvg| + |cvr|) + 2^(shift - 1) = %lld >= 2^31: an int32 intermediate could overflow", who,
               (long long)worst);
    *g = Nv12Geom{H0, W0, pitch, uv_offset};
    *k = Nv12Coef{c[0], c[1], c[2], c[3], c[4], c[5], shift, 1 << (shift - 1)};
    return 0;
}

// every row of both planes of every frame starts on a 16-byte boundary
inline bool nv12_rows_aligned(const uint8_t* frames, int64_t pitch, int64_t uv_offset, int64_t frame_pitch) {
    return goalnet::aligned16(frames) && pitch % 16 == 0 && uv_offset % 16 == 0 && frame_pitch % 16 == 0;
}

}  // namespace
