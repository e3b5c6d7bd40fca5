// What every pass over ranges of the flat parameter arena shares: the range list as it travels in the kernel arguments,
// the host checks that fill it, and a block's walk over its share of a range. A new arena pass starts here: map_ranges on the host,
// block_share and for_share in the kernel, and the per-element work in two functors.
//
// Up to GOALNET_ADAM_RANGES_MAX ranges run in ONE launch (frozen tensors split the arena; a launch per range would cost more than a
// small step saves). The descriptors travel by value, so a captured graph bakes them. Blocks [first_block[r], first_block[r + 1])
// serve range r and stride over it alone: no block spans two ranges.
#pragma once
#include <string.h>

#include "common.h"

namespace goalnet {

struct RangeMap {
    int64_t begin[GOALNET_ADAM_RANGES_MAX], count[GOALNET_ADAM_RANGES_MAX];
    int first_block[GOALNET_ADAM_RANGES_MAX + 1];
};

constexpr int RANGE_BLOCKS_MAX = 8192;                   // 256-thread blocks per range in the streaming passes: beyond it a block strides

// ---- host -------------------------------------------------------------------------------------------------------------------------------
inline int blocks_for(int64_t n4, int cap) {
    int64_t b = (n4 + 255) / 256;
    if (b > cap) b = cap;
    if (b < 1) b = 1;
    return (int)b;
}

// Range: goalnet_adam_range, goalnet_optim_range or goalnet_group_range (the same ordering, alignment and count rules). Fills *rs for a
// launch of rs->first_block[count] blocks, at most `cap` per range. What a caller reads beyond begin and count (skipped, decay,
// group) it checks and copies itself.
template <class Range>
inline int map_ranges(const char* who, const Range* ranges, int count, int cap, RangeMap* rs) {
    GN_REQUIRE(ranges, GOALNET_E_NULL, "%s: null pointer", who);
    GN_REQUIRE(count >= 1 && count <= GOALNET_ADAM_RANGES_MAX, GOALNET_E_SHAPE, "%s: 1..%d ranges", who, GOALNET_ADAM_RANGES_MAX);
    memset(rs, 0, sizeof *rs);                           // the entries beyond `count` and the padding: a captured graph bakes every byte
    int64_t end = 0;
    for (int r = 0; r < count; ++r) {
        const Range& a = ranges[r];
        GN_REQUIRE(a.begin >= 0 && a.count > 0, GOALNET_E_SHAPE, "%s: range %d is empty or starts below 0", who, r);
        GN_REQUIRE((a.begin & 3) == 0, GOALNET_E_ALIGN, "%s: range %d must begin at a multiple of 4 elements", who, r);
        GN_REQUIRE(a.begin >= end, GOALNET_E_SHAPE, "%s: range %d overlaps its predecessor or is out of order", who, r);
        end = a.begin + a.count;
        rs->begin[r] = a.begin;
        rs->count[r] = a.count;
        rs->first_block[r + 1] = rs->first_block[r] + blocks_for(a.count >> 2, cap);
    }
    return 0;
}

// the 16-bit copy's slice [begin, begin + count) of the arena; ptr may be null (no copy). n: the arena's length where the entry point
// knows it (the whole-arena doors: the slice must lie inside), -1 where it does not (the range doors)
inline int check_shadow(const char* who, const void* ptr, int64_t begin, int64_t count, int64_t n) {
    if (!ptr) return 0;
    const bool shaped = begin >= 0 && count > 0 && (begin & 3) == 0 && (count & 3) == 0;
    if (n >= 0)
        GN_REQUIRE(shaped && begin + count <= n, GOALNET_E_SHAPE, "%s: the shadowed slice must lie inside the arena, offset and length multiples of 4", who);
    else
        GN_REQUIRE(shaped, GOALNET_E_SHAPE, "%s: the shadowed slice's offset and length must be multiples of 4", who);
    GN_REQUIRE((reinterpret_cast<uintptr_t>(ptr) & 7u) == 0, GOALNET_E_ALIGN, "%s: shadow must be 8-byte aligned", who);
    return 0;
}

// ---- device -----------------------------------------------------------------------------------------------------------------------------
// this block's share: range r = [begin, begin + n) of the arena, of whose nb blocks it is number lb
struct BlockShare {
    int r;
    int64_t begin, n, lb, nb;
};

__device__ __forceinline__ BlockShare block_share(const RangeMap& rs, int nranges) {
    int r = 0;
    while (r + 1 < nranges && (int)blockIdx.x >= rs.first_block[r + 1]) ++r;
    return {r, rs.begin[r], rs.count[r], (int)blockIdx.x - rs.first_block[r], rs.first_block[r + 1] - rs.first_block[r]};
}

// body4(i): the arena's float4 number i, once per whole float4 of the share; body1(i): element i of the n & 3 that remain, on the
// range's first block
template <class F4, class F1>
__device__ __forceinline__ void for_share(const BlockShare& b, F4 body4, F1 body1) {
    const int64_t b4 = b.begin >> 2, n4 = b.n >> 2;
    for (int64_t j = b.lb * blockDim.x + threadIdx.x; j < n4; j += b.nb * blockDim.x) body4(b4 + j);
    if (b.lb == 0 && threadIdx.x < (b.n & 3)) body1(b.begin + (n4 << 2) + threadIdx.x);
}

}  // namespace goalnet
