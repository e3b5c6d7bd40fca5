// Gradient accumulation over the micro-steps of a window (include/goalnet_accum.h). One streaming pass over the
// trainable ranges behind each backward: acc = g * scale on the window's first micro-step (8 bytes per element, acc is not read),
// acc = acc + g * scale on the later ones (12 bytes). The product and the sum are rounded separately (contraction is switched off
// where they meet), so the pass is the two torch operations `t = g * scale; acc = acc + t`, bit for bit. `first` and `scale` are launch
// arguments: the host knows the position in the window, and a captured graph bakes it in. Block-to-range mapping and tail are
// adam_ranges_kernel's (small.hip).
#include <math.h>

#include "../../include/goalnet_accum.h"
#include "common.h"

using namespace goalnet;

namespace {

constexpr int ACCUM_BLOCKS_MAX = 8192;                    // 256-thread blocks per range, as for Adam: beyond it a block strides

struct AccumRanges {
    int64_t begin[GOALNET_ADAM_RANGES_MAX], count[GOALNET_ADAM_RANGES_MAX];
    int first_block[GOALNET_ADAM_RANGES_MAX + 1];
};

// hipcc contracts a * b + c by default (-ffp-contract=fast-honor-pragmas), also through __fmul_rn / __fadd_rn, which are plain
// operators in its headers; under the pragma the product and the sum stay two instructions (v_pk_mul_f32, v_pk_add_f32). The pragma
// belongs at the start of a block: the kernel carries it too, for the expressions inlined into it.
__device__ __forceinline__ float accum1(float a, float g, float c) {
#pragma clang fp contract(off)
    const float t = g * c;
    return a + t;
}

template <bool FIRST>
__global__ __launch_bounds__(256) void accum_ranges_kernel(float* __restrict__ acc, const float* __restrict__ g, AccumRanges rs, int nranges,
                                                          float c) {
#pragma clang fp contract(off)
    int r = 0;
    while (r + 1 < nranges && (int)blockIdx.x >= rs.first_block[r + 1]) ++r;
    const int64_t lb = (int)blockIdx.x - rs.first_block[r], nb = rs.first_block[r + 1] - rs.first_block[r];
    const int64_t begin = rs.begin[r], n = rs.count[r], b4 = begin >> 2, n4 = n >> 2;
    for (int64_t j = lb * blockDim.x + threadIdx.x; j < n4; j += nb * blockDim.x) {
        const int64_t i = b4 + j;                         // float4 index in the arena
        const float4 gg = reinterpret_cast<const float4*>(g)[i];
        float4 a;
        if (FIRST) {
            a.x = __fmul_rn(gg.x, c);
            a.y = __fmul_rn(gg.y, c);
            a.z = __fmul_rn(gg.z, c);
            a.w = __fmul_rn(gg.w, c);
        } else {
            a = reinterpret_cast<const float4*>(acc)[i];
            a.x = accum1(a.x, gg.x, c);
            a.y = accum1(a.y, gg.y, c);
            a.z = accum1(a.z, gg.z, c);
            a.w = accum1(a.w, gg.w, c);
        }
        reinterpret_cast<float4*>(acc)[i] = a;
    }
    if (lb == 0 && threadIdx.x < (n & 3)) {
        const int64_t i = begin + (n4 << 2) + threadIdx.x;
        acc[i] = FIRST ? __fmul_rn(g[i], c) : accum1(acc[i], g[i], c);
    }
}

int blocks_for(int64_t n4) {
    int64_t b = (n4 + 255) / 256;
    if (b > ACCUM_BLOCKS_MAX) b = ACCUM_BLOCKS_MAX;
    if (b < 1) b = 1;
    return (int)b;
}

int check_ranges(const char* who, const goalnet_adam_range* ranges, int count, AccumRanges* rs) {
    GN_REQUIRE(ranges, GOALNET_E_NULL, "%s: null pointer", who);
    GN_REQUIRE(count >= 1 && count <= GOALNET_ADAM_RANGES_MAX, GOALNET_E_SHAPE, "%s: 1..%d ranges", who, GOALNET_ADAM_RANGES_MAX);
    int64_t end = 0;
    rs->first_block[0] = 0;
    for (int r = 0; r < count; ++r) {
        const goalnet_adam_range& a = ranges[r];
        GN_REQUIRE(a.begin >= 0 && a.count > 0, GOALNET_E_SHAPE, "%s: range %d is empty or starts below 0", who, r);
        GN_REQUIRE((a.begin & 3) == 0, GOALNET_E_ALIGN, "%s: range %d must begin at a multiple of 4 elements", who, r);
        GN_REQUIRE(a.begin >= end, GOALNET_E_SHAPE, "%s: range %d overlaps its predecessor or is out of order", who, r);
        end = a.begin + a.count;
        rs->begin[r] = a.begin;
        rs->count[r] = a.count;
        rs->first_block[r + 1] = rs->first_block[r] + blocks_for(a.count >> 2);
    }
    return 0;
}

}  // namespace

extern "C" {

int goalnet_grad_accum_dev_ranges(float* acc, const float* g, const goalnet_adam_range* ranges, int count, float scale, int first,
                                  void* stream) {
    GN_REQUIRE(acc && g, GOALNET_E_NULL, "grad_accum_dev_ranges: null pointer");
    AccumRanges rs;
    const int rc = check_ranges("grad_accum_dev_ranges", ranges, count, &rs);
    if (rc != 0) return rc;
    GN_REQUIRE(isfinite(scale) && scale > 0.0f, GOALNET_E_VALUE, "grad_accum_dev_ranges: scale must be finite and > 0");
    GN_REQUIRE(acc != g, GOALNET_E_VALUE, "grad_accum_dev_ranges: the accumulator and the gradients are the same arena");
    GN_REQUIRE(aligned16(acc) && aligned16(g), GOALNET_E_ALIGN, "grad_accum_dev_ranges: arenas must be 16-byte aligned");
    const dim3 grid((unsigned)rs.first_block[count]), block(256);
    if (first)
        hipLaunchKernelGGL(accum_ranges_kernel<true>, grid, block, 0, (hipStream_t)stream, acc, g, rs, count, scale);
    else
        hipLaunchKernelGGL(accum_ranges_kernel<false>, grid, block, 0, (hipStream_t)stream, acc, g, rs, count, scale);
    GN_LAUNCH_CHECK("grad_accum_dev_ranges");
    return 0;
}

}  // extern "C"
