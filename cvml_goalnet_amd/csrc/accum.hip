// Gradient accumulation over the micro-steps of a window (include/goalnet_accum.h). One streaming pass over the
// trainable ranges behind each backward: acc = g * scale on the window's first micro-step (8 bytes per element, acc is not read),
// acc = acc + g * scale on the later ones (12 bytes). The product and the sum are rounded separately (contraction is switched off
// where they meet), so the pass is the two torch operations `t = g * scale; acc = acc + t`, bit for bit. `first` and `scale` are launch
// arguments: the host knows the position in the window, and a captured graph bakes it in. Block-to-range mapping, tail and the host's
// range checks are ranges.h's.
#include <math.h>

#include "../../include/goalnet_accum.h"
#include "ranges.h"

using namespace goalnet;

namespace {

// hipcc contracts a * b + c by default (-ffp-contract=fast-honor-pragmas), also through __fmul_rn / __fadd_rn, which are plain
// operators in its headers; under the pragma the product and the sum stay two instructions (v_pk_mul_f32, v_pk_add_f32). The pragma
// belongs at the start of a block: the kernel's two functors carry it too, for the expressions inlined into them.
__device__ __forceinline__ float accum1(float a, float g, float c) {
#pragma clang fp contract(off)
    const float t = g * c;
    return a + t;
}

template <bool FIRST>
__global__ __launch_bounds__(256) void accum_ranges_kernel(float* __restrict__ acc, const float* __restrict__ g, RangeMap rs, int nranges,
                                                          float c) {
    for_share(
        block_share(rs, nranges),
        [&](int64_t i) {
#pragma clang fp contract(off)
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
        },
        [&](int64_t i) {
#pragma clang fp contract(off)
            acc[i] = FIRST ? __fmul_rn(g[i], c) : accum1(acc[i], g[i], c);
        });
}

}  // namespace

extern "C" {

int goalnet_grad_accum_dev_ranges(float* acc, const float* g, const goalnet_adam_range* ranges, int count, float scale, int first,
                                  void* stream) {
    GN_REQUIRE(acc && g, GOALNET_E_NULL, "grad_accum_dev_ranges: null pointer");
    RangeMap rs;
    const int rc = map_ranges("grad_accum_dev_ranges", ranges, count, RANGE_BLOCKS_MAX, &rs);
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
