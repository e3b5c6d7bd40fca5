// fp32 GEMM engine on the gfx950 matrix cores (v_mfma_f32_32x32x2_f32: f32 in, f32 accumulate, bit-exact
// fmaf chain, 64 FLOP/clk/SIMD = 157 TFLOP/s chip peak) and the hot-path ops built on it:
//
//   conv 3x3 s1 p1 forward / data-gradient  (implicit GEMM, im2col on the A load, BatchNorm folded into the load)
//   conv 3x3 weight-gradient                (implicit GEMM reduced over N*H*W, deterministic split + slab sum)
//   linear forward / dX / dW                (linear5 with BatchNorm folded into the load and split-K)
//
// Replaces ATen's CPU conv2d / linear (oneDNN, MKL) under /root/reference/utils.py:156-170, 243-253 and
// their autograd counterparts (main.py:192).
//
// Geometry: 256 threads = 4 waves (one per SIMD), block tile 128 x 128 x 32, wave tile 64 x 64 =
// 2 x 2 MFMA tiles of 32 x 32 (64 accumulator VGPRs). Operands are staged global -> registers -> LDS
// (the A loader applies an affine and zero padding on the way, so LDS-DMA is not usable), double-buffered
// in LDS with the next K-tile's global loads in flight under the current tile's 64 MFMAs per wave.
// (The convolution's A operand is staged once per nine K-tiles where its strip fits: ConvAStripLoader.)
// An fp32 MFMA occupies its SIMD for 64 cycles, so the 4096 MFMA cycles per K-tile per wave cover the
// 8 global loads + 8 LDS writes + 16-32 LDS reads a thread issues per K-tile with room to spare.
//
// The K order inside a K-tile is permuted identically for A and B (lane half h of MFMA step j of group s
// holds k = 8s + 4h + j) so that a K-contiguous operand is read from LDS with one ds_read_b128 per four
// MFMA steps; rows are padded to 36 floats, which makes those reads bank-conflict free.
#include <stdlib.h>

#include "adam.h"
#include "gemm_common.h"
#include "skinny.h"

using namespace goalnet;

namespace {

constexpr int BM = 128, BN = 128, BK = 32;
constexpr int LDR = 128;              // row-contiguous operand: LDS stride between k rows
constexpr int OP_FLOATS = BM * BK;    // 4096 floats = 16 KB per operand per stage (both images)

// K-contiguous LDS image: [128 rows][32 floats], unpadded (an LDS-DMA wave-instruction writes 1 KB contiguously, so
// rows cannot be padded) with the eight 16-B chunks of a row XOR-swizzled by (row >> 1) & 7: the 16 lanes of a
// ds_read_b128 group (rows {0-3,12-15,20-27} + ...) then land on 16 distinct 4-bank slots -> conflict-free.
__device__ __forceinline__ int kc_off(int row, int chunk) { return row * BK + ((chunk ^ ((row >> 1) & 7)) << 2); }

__device__ __forceinline__ float4 f4zero() { return make_float4(0.f, 0.f, 0.f, 0.f); }
__device__ __forceinline__ float4 f4fma(float4 v, float4 s, float4 t) {
    return make_float4(fmaf(v.x, s.x, t.x), fmaf(v.y, s.y, t.y), fmaf(v.z, s.z, t.z), fmaf(v.w, s.w, t.w));
}

// ------------------------------------------------------------------------------------------------
// operand loaders: global -> registers (4 x float4 per thread per K-tile)
// ------------------------------------------------------------------------------------------------
// The fp32 MFMA runs on the SIMD's fp32 lanes: every VALU instruction a wave issues between its MFMAs costs matrix
// time one for one (measured, scripts/bench_gemm.py: conv3 forward 147 TFLOP/s with the staging instructions
// removed, 126 with the first version's ~200 VALU per K-tile of 64-bit address arithmetic, masks and selects; moving
// them to dedicated producer waves on the same SIMDs did not help). So the loaders are built to need (almost) no
// VALU in the loop:
//   * every load is a `buffer_load_dwordx4` through a per-block 128-bit buffer resource (SGPRs): the per-thread
//     byte offset is a loop-invariant VGPR, the K-tile / tap / row-group advance is a scalar offset (SALU only);
//   * rows past the end of a matrix and zero-padding taps rely on the buffer range check (out-of-range loads return
//     0) instead of selects. Validity is always encoded in the loop-invariant voffset (an OOB marker) and
//     num_records is the true extent, so the result does not depend on whether the scalar offset takes part in the
//     range check (on gfx950 it does: measured); the resource is re-based per block / K-tile to span < 4 GB;
//   * issue() only issues loads (they stay in flight under the current tile's MFMAs); finish() applies what is left
//     (the BatchNorm affine, and a select only where a zero must survive the affine) right before the LDS write.
typedef unsigned int u32x4 __attribute__((ext_vector_type(4)));
constexpr unsigned OOB = 0xFFFFFF00u;   // a voffset beyond any resource's num_records

__device__ __forceinline__ float4 f4sel(bool v, float4 a) { return v ? a : f4zero(); }

__device__ __forceinline__ __amdgpu_buffer_rsrc_t make_rsrc(const void* base, uint32_t bytes) {
    return __builtin_amdgcn_make_buffer_rsrc(const_cast<void*>(base), 0, (int)bytes, 0x00020000);
}
__device__ __forceinline__ float4 bload(__amdgpu_buffer_rsrc_t r, unsigned voff, unsigned soff) {
    const u32x4 v = __builtin_amdgcn_raw_buffer_load_b128(r, (int)voff, (int)soff, 0);
    return make_float4(__uint_as_float(v.x), __uint_as_float(v.y), __uint_as_float(v.z), __uint_as_float(v.w));
}
__device__ __forceinline__ uint32_t clamp_u32(int64_t v) {
    return v <= 0 ? 0u : (v > 0xFFFFFF00ll ? 0xFFFFFF00u : (uint32_t)v);
}

// K-contiguous matrix X[rows][K] (leading dim ld < 8M). Optional affine x*scale[k % C] + shift[k % C].
// Rows past `rows` read 0 (before the affine: with AFFINE they hold `shift`, which only reaches output rows that
// are never stored).
// convC > 0: the matrix is a 3x3 convolution's weight [rows][9][convC] read in the (channel chunk, tap) K order of ConvALoader:
// K-tile kt holds tap kt % 9 of channels [32 (kt / 9), +32).
template <bool AFFINE>
struct KCLoader {
    struct P {
        const float* x; int64_t ld; int rows;
        const float* scale; const float* shift; int bnC;
        int convC;
    };
    static constexpr bool KC = true;
    static constexpr bool STRIP = false;
    static constexpr bool ONE_STAGE = false;      // as the A operand (linear5 forward / dX): two LDS stages, see launch_gemm
    static constexpr int ONE_STAGE_BLOCKS = 3;
    __amdgpu_buffer_rsrc_t rx, rsc, rsh;
    unsigned voff[4], vaff;
    int bnC, convC;
    float4 sc, sh;
    __device__ KCLoader(const P& p, int row0, int tid) {
        const int nrows = p.rows - row0 < BM ? p.rows - row0 : BM;
        rx = make_rsrc(p.x + (int64_t)row0 * p.ld, clamp_u32((int64_t)nrows * p.ld * 4));
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const int rl = (tid >> 3) + 32 * i;
            voff[i] = rl < nrows ? (unsigned)(((int64_t)rl * p.ld + (tid & 7) * 4) * 4) : OOB;
        }
        bnC = p.bnC; convC = p.convC;
        if (AFFINE) {
            rsc = make_rsrc(p.scale, (uint32_t)p.bnC * 4);
            rsh = make_rsrc(p.shift, (uint32_t)p.bnC * 4);
            vaff = (unsigned)((tid & 7) * 16);
        }
    }
    __device__ __forceinline__ void issue(int kt, float4 (&r)[4]) {
        unsigned k4 = (unsigned)kt * (BK * 4);
        if (convC > 0) {
            const int chunk = kt / 9, tap = kt - 9 * chunk;
            k4 = (unsigned)(tap * convC + chunk * BK) * 4;
        }
        if (AFFINE) {
            const unsigned ch4 = (unsigned)((kt * BK) % bnC) * 4;
            sc = bload(rsc, vaff, ch4);
            sh = bload(rsh, vaff, ch4);
        }
#pragma unroll
        for (int i = 0; i < 4; ++i) r[i] = bload(rx, voff[i], k4);
    }
    __device__ __forceinline__ void finish(float4 (&r)[4]) const {
        if (AFFINE) {
#pragma unroll
            for (int i = 0; i < 4; ++i) r[i] = f4fma(r[i], sc, sh);
        }
    }
};

// Row-contiguous matrix X[kred][cols] (leading dim ld): for a fixed reduction index the tile's columns are
// contiguous. Optional affine per column (channel = col % C), fixed per thread. The resource is re-based every K-tile
// (32 reduction rows), so reduction rows past `kred` are out of range by construction.
template <bool AFFINE>
struct MCLoader {
    struct P {
        const float* x; int64_t ld; int cols; int kred;
        const float* scale; const float* shift; int bnC;
    };
    static constexpr bool KC = false;
    static constexpr bool STRIP = false;
    static constexpr bool ONE_STAGE = true;
#ifndef GN_MC_BLOCKS
#define GN_MC_BLOCKS 4
#endif
    static constexpr int ONE_STAGE_BLOCKS = GN_MC_BLOCKS;    // blocks per CU with one LDS stage (register budget 128; 3: budget 168)
    const float* x;
    int64_t ld;
    int kred, k0;
    unsigned voff[4];
    bool partial;
    float4 sc, sh;
    __device__ MCLoader(const P& p, int col0, int tid) {
        const int col = col0 + (tid & 31) * 4;
        const bool colok = col < p.cols;
        x = p.x; ld = p.ld; kred = p.kred; k0 = tid >> 5;
#pragma unroll
        for (int i = 0; i < 4; ++i) voff[i] = colok ? (unsigned)(((int64_t)(k0 + 8 * i) * p.ld + col) * 4) : OOB;
        partial = false;
        if (AFFINE) {
            const int ch = (colok ? col : 0) % p.bnC;
            sc = *reinterpret_cast<const float4*>(p.scale + ch);
            sh = *reinterpret_cast<const float4*>(p.shift + ch);
            if (!colok) sh = f4zero();          // columns past `cols` must stay 0 through the affine
        }
    }
    __device__ __forceinline__ void issue(int kt, float4 (&r)[4]) {
        const int kbase = kt * BK;
        const int nk = kred - kbase < BK ? kred - kbase : BK;
        partial = nk < BK;
        const __amdgpu_buffer_rsrc_t rx = make_rsrc(x + (int64_t)kbase * ld, clamp_u32((int64_t)nk * ld * 4));
#pragma unroll
        for (int i = 0; i < 4; ++i) r[i] = bload(rx, voff[i], 0);
    }
    __device__ __forceinline__ void finish(float4 (&r)[4]) const {
        if (AFFINE) {
            if (partial) {      // last K-tile only (wave-uniform): reduction rows past `kred` must be 0, not `shift`
#pragma unroll
                for (int i = 0; i < 4; ++i) r[i] = f4sel(k0 + 8 * i < (kred & (BK - 1)), f4fma(r[i], sc, sh));
            } else {
#pragma unroll
                for (int i = 0; i < 4; ++i) r[i] = f4fma(r[i], sc, sh);
            }
        }
    }
};

// bit kh * 3 + kw: tap (kh, kw) of output pixel m = (n,h,w) lies inside its frame; 0 for rows past M
__device__ __forceinline__ unsigned conv_tap_mask(int64_t m, int64_t M, int H, int W) {
    unsigned mk = 0;
    if (m < M) {
        const int w = (int)((unsigned)m % (unsigned)W);
        const int h = (int)(((unsigned)m / (unsigned)W) % (unsigned)H);
#pragma unroll
        for (int kh = 0; kh < 3; ++kh)
#pragma unroll
            for (int kw = 0; kw < 3; ++kw) {
                const bool v = (unsigned)(h + kh - 1) < (unsigned)H && (unsigned)(w + kw - 1) < (unsigned)W;
                mk |= (v ? 1u : 0u) << (kh * 3 + kw);
            }
    }
    return mk;
}

// im2col of an NHWC tensor for a 3x3 / stride 1 / pad 1 convolution: row m = (n,h,w), k = (kh,kw,ci).
// The affine (BatchNorm of the producing block) is applied to in-bounds elements only: the reference pads the
// BatchNorm OUTPUT with zeros (/root/reference/utils.py:154-156). The resource starts W+1 pixels in front of the
// tile's first pixel, so every tap shift is a non-negative scalar offset; padding taps get an out-of-range voffset.
template <bool AFFINE>
struct ConvALoader {
    struct P {
        const float* x; int H, W, C; int64_t M;
        const float* scale; const float* shift;
    };
    static constexpr bool KC = true;
    static constexpr bool STRIP = false;
    static constexpr bool ONE_STAGE = true;
    static constexpr int ONE_STAGE_BLOCKS = AFFINE ? 3 : 4;      // with the affine the loop spills at a budget of 128 registers (111 TF/s)
    __amdgpu_buffer_rsrc_t rx, rsc, rsh;
    unsigned mask[4];
    unsigned voff, vaff, vmask;
    int W, C;
    float4 sc, sh;
    __device__ ConvALoader(const P& p, int row0, int tid) {
        W = p.W; C = p.C;
        const int c4 = (tid & 7) * 4, rr = tid >> 3;
        rx = make_rsrc(p.x + ((int64_t)row0 - (p.W + 1)) * p.C, (uint32_t)((BM + 2 * (p.W + 1)) * p.C * 4));
        voff = (unsigned)((rr * p.C + c4) * 4);
        if (AFFINE) {
            rsc = make_rsrc(p.scale, (uint32_t)p.C * 4);
            rsh = make_rsrc(p.shift, (uint32_t)p.C * 4);
            vaff = (unsigned)(c4 * 4);
        }
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            mask[i] = conv_tap_mask((int64_t)row0 + rr + 32 * i, p.M, p.H, p.W);
        }
    }
    // K order = (32-channel chunk, tap): the nine taps of a chunk re-read the same 128-B lines (one pixel's chunk = one line)
    // back to back, so they hit L2 instead of streaming the whole halo of the tile nine times (profiles/r02_traffic.md)
    __device__ __forceinline__ void issue(int kt, float4 (&r)[4]) {
        const int chunk = kt / 9;
        const int tap = kt - 9 * chunk;
        const int ci = chunk * BK;
        const int kh = tap / 3, kw = tap - 3 * kh;
        const unsigned s0 = (unsigned)(((kh * W + kw) * C + ci) * 4);     // shift by the resource's W+1 pixel lead
        const unsigned rowstep = (unsigned)(32 * C * 4);
        if (AFFINE) {
            sc = bload(rsc, vaff, (unsigned)ci * 4);
            sh = bload(rsh, vaff, (unsigned)ci * 4);
        }
        vmask = 0;
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const bool v = (mask[i] >> tap) & 1u;
            vmask |= (v ? 1u : 0u) << i;
            r[i] = bload(rx, v ? voff : OOB, s0 + (unsigned)i * rowstep);
        }
    }
    __device__ __forceinline__ void finish(float4 (&r)[4]) const {
        if (AFFINE) {
#pragma unroll
            for (int i = 0; i < 4; ++i) r[i] = f4sel((vmask >> i) & 1u, f4fma(r[i], sc, sh));
        }
    }
};

// The same operand staged once per 32-channel chunk instead of once per K-tile. The nine K-tiles (taps) of a chunk hold the
// same input pixels shifted by kh * W + kw rows: all nine are windows of one strip of 128 + 2 (W + 1) consecutive pixels,
// [row0 - (W + 1), row0 + 128 + (W + 1)). The block loads that strip once (buffer loads; pixels outside the tensor read 0
// through an out-of-range voffset), applies the affine once per element and writes it to ONE K-contiguous LDS image of 128-B
// rows, swizzled by kc_off on the strip row. K-tile (chunk, tap) then reads its A fragments from strip row
// local_row + kh * W + kw. A lane whose (pixel, tap) is padding (frame border, or a row >= M) reads the row of zeros behind
// the strip instead: an ADDRESS select by the same 9-bit tap masks, no data select and no affine in the loop.
//   * bank conflicts: the 16 lanes of a ds_read_b128 group read rows whose residues mod 16 are all distinct ({0-3,12-15,
//     20-27} + ...); (row & 1, (row >> 1) & 7) is that residue, it picks the 32-bank half and the swizzled 4-bank slot, and a
//     constant row shift permutes residues. So every tap's window is conflict-free; only lanes sent to the zero row share
//     one address (a broadcast) that may collide with a single data lane.
//   * strip pixels of OTHER frames (and, with the affine, out-of-tensor rows holding `shift`) sit in the image but are only
//     ever addressed by taps that the masks send to the zero row.
//   * the loads of the next chunk's strip are issued one per tap under the current chunk's nine K-tiles, held in registers
//     (9 float4) and written after the last tap's barrier; B (the weights) is staged per K-tile as before.
// 32 strip rows per load and thread: 9 loads cover 288 rows, i.e. W <= 79; 289 rows of 128 B + 16 KB of B = 52.1 KB, three
// blocks per CU.
constexpr int STRIP_LOADS = 9;
constexpr int STRIP_ROWS = 32 * STRIP_LOADS;                 // the row behind them (index STRIP_ROWS) holds zeros
constexpr int STRIP_FLOATS = (STRIP_ROWS + 1) * BK;
constexpr int CONV_STRIP_MAX_W = (STRIP_ROWS - BM) / 2 - 1;  // 128 + 2 (W + 1) <= 288

template <bool AFFINE>
struct ConvAStripLoader {
    using P = typename ConvALoader<AFFINE>::P;
    static constexpr bool KC = true;
    static constexpr bool STRIP = true;
    static constexpr bool ONE_STAGE = true;
    static constexpr int ONE_STAGE_BLOCKS = 3;
    __amdgpu_buffer_rsrc_t rx, rsc, rsh;
    unsigned mask[2];        // tap masks of the two fragment rows this lane reads
    unsigned lrow[2];        // their local rows in the tile
    unsigned voff, vaff, bad;
    int W, C, h;
    float4 sc, sh;
    __device__ ConvAStripLoader(const P& p, int row0, int tid) {
        W = p.W; C = p.C;
        const int c4 = (tid & 7) * 4, rr = tid >> 3;
        const int64_t lead = (int64_t)row0 - (p.W + 1);
        const int nrows = BM + 2 * (p.W + 1);
        rx = make_rsrc(p.x + lead * p.C, (uint32_t)(nrows * p.C * 4));
        voff = (unsigned)((rr * p.C + c4) * 4);
        bad = 0;            // bit i: strip row rr + 32 i lies outside the tensor (or behind the strip): never touch it
#pragma unroll
        for (int i = 0; i < STRIP_LOADS; ++i) {
            const int64_t pix = lead + rr + 32 * i;
            bad |= (pix < 0 || pix >= p.M || rr + 32 * i >= nrows ? 1u : 0u) << i;
        }
        if (AFFINE) {
            rsc = make_rsrc(p.scale, (uint32_t)p.C * 4);
            rsh = make_rsrc(p.shift, (uint32_t)p.C * 4);
            vaff = (unsigned)(c4 * 4);
        }
        const int wm = tid >> 7, r = tid & 31;
        h = (tid >> 5) & 1;
#pragma unroll
        for (int q = 0; q < 2; ++q) {
            lrow[q] = (unsigned)(wm * 64 + q * 32 + r);
            mask[q] = conv_tap_mask((int64_t)row0 + lrow[q], p.M, p.H, p.W);
        }
    }
    __device__ __forceinline__ void begin(int chunk) {       // the chunk's affine coefficients (consumed by store())
        if (AFFINE) {
            sc = bload(rsc, vaff, (unsigned)(chunk * BK) * 4);
            sh = bload(rsh, vaff, (unsigned)(chunk * BK) * 4);
        }
    }
    __device__ __forceinline__ float4 load(int chunk, int i) const {
        unsigned b = bad;                   // as in frag_base: nine hoisted voffsets would spill
        asm volatile("" : "+v"(b));
        return bload(rx, (b >> i) & 1u ? OOB : voff, (unsigned)((i * 32 * C + chunk * BK) * 4));
    }
    __device__ __forceinline__ void store(float* l, const float4 (&rs)[STRIP_LOADS], int tid) const {
        const int c = tid & 7, row = tid >> 3;
#pragma unroll
        for (int i = 0; i < STRIP_LOADS; ++i)
            *reinterpret_cast<float4*>(&l[kc_off(row + 32 * i, c)]) = AFFINE ? f4fma(rs[i], sc, sh) : rs[i];
    }
    // byte offsets of this lane's two fragment rows for K-tile `tap`; group s of the K-tile is at (offset ^ (s << 5)):
    // kc_off(row, 2 s + h) * 4 = (row << 7 | (h ^ (row >> 1 & 7)) << 4) ^ (s << 5)
    __device__ __forceinline__ void frag_base(int tap, unsigned (&ab)[2]) const {
        const int kh = tap / 3, kw = tap - 3 * kh;
        const unsigned shift = (unsigned)(kh * W + kw);
#pragma unroll
        for (int q = 0; q < 2; ++q) {
            // recomputed per K-tile (7 VALU): hoisted out of the chunk loop the 72 offsets of the nine taps spill
            unsigned mk = mask[q];
            asm volatile("" : "+v"(mk));
            const unsigned row = (mk >> tap) & 1u ? lrow[q] + shift : (unsigned)STRIP_ROWS;
            ab[q] = (row << 7) | (((unsigned)h ^ ((row >> 1) & 7u)) << 4);
        }
    }
};

// B operand of the weight gradient: B(col = (tap, ci), red = m) = bnapply(x)[pixel m shifted by tap][ci].
// Tap validity comes from a per-pixel border-code byte (bit0 h==0, bit1 h==H-1, bit2 w==0, bit3 w==W-1) prepared by
// border_codes_kernel, so the loop needs no division; the resource is re-based per K-tile W+1 pixels in front of it.
// The codes act on the ADDRESS (a padding tap loads from an out-of-range offset and reads 0), never on the data: the first
// version zeroed the loaded values instead (16 selects + 4 byte loads per thread and K-tile) and the fp32 MFMA, which shares
// its issue slots with every vector instruction, ran at 112 TF/s against 136 with the selects compiled out (conv3, 128 frames).
// With the affine the zero of a padding tap becomes `shift[ci]`, i.e. the GEMM accumulates shift[ci] * dy[m][co] for every
// (pixel, tap) whose tap falls into the padding; that term is a rank-one product of shift with sums of dy over border pixels
// (wgrad_border_sums_kernel below) and the slab reduction subtracts it (EpiP::corr_*). It only involves the 2 (H + W) - 4
// border pixels of a frame, so nothing cancels: the correction is ~5 % of the accumulated magnitude.
// codes4[kt * 8 + k0] packs the codes of the four pixels kt * 32 + k0 + 8 i one thread loads of a K-tile; the word for the
// next K-tile is fetched one K-tile ahead.
// DSEL (few frames: the reference's 10-frame sub-batches, where two more launches for U cost more than the GEMM loses): the
// first version's data select instead — every tap loads, finish() zeroes the padding taps after the affine, no correction.
template <bool AFFINE, bool DSEL = false>
struct ConvWgradBLoader {
    struct P {
        const float* x; int H, W, C; int M;
        const float* scale; const float* shift;
        const uint32_t* codes4;
    };
    static constexpr bool KC = false;
    const float* x;
    __amdgpu_buffer_rsrc_t rcodes;
    int W, C, M, k0, tapshift, nextkt;
    unsigned voff[4], bad4, nextcode, badnow;
    float4 sc, sh;
    __device__ ConvWgradBLoader(const P& p, int col0, int tid) {
        const int col = col0 + (tid & 31) * 4;
        const bool colok = col < 9 * p.C;
        const int cc = colok ? col : 0;
        const int tap = cc / p.C, ci = cc - tap * p.C;
        const int kh = tap / 3, kw = tap - 3 * kh;
        x = p.x; W = p.W; C = p.C; M = p.M; k0 = tid >> 5;
        rcodes = make_rsrc(p.codes4, (uint32_t)((p.M + 31) / 32 * 32));
        bad4 = ((kh == 0 ? 1u : 0u) | (kh == 2 ? 2u : 0u) | (kw == 0 ? 4u : 0u) | (kw == 2 ? 8u : 0u)) * 0x01010101u;
        tapshift = kh * p.W + kw;
        nextkt = -1; nextcode = 0;
#pragma unroll
        for (int i = 0; i < 4; ++i) voff[i] = colok ? (unsigned)(((k0 + 8 * i + tapshift) * p.C + ci) * 4) : OOB;
        if (AFFINE) {
            sc = *reinterpret_cast<const float4*>(p.scale + ci);
            sh = *reinterpret_cast<const float4*>(p.shift + ci);
        }
    }
    __device__ __forceinline__ unsigned load_code(int kt) const {
        return (unsigned)__builtin_amdgcn_raw_buffer_load_b32(rcodes, k0 * 4, kt * 32, 0);    // past the table: 0 (never consumed)
    }
    __device__ __forceinline__ void issue(int kt, float4 (&r)[4]) {
        const int mbase = kt * BK;
        const unsigned badc = (nextkt == kt ? nextcode : load_code(kt)) & bad4;     // pixels >= M carry 0xF: every tap bad
        badnow = badc;
        const unsigned bad = DSEL ? 0u : badc;
        // pixels [mbase - (W+1), mbase + 32 + (W+1)) clipped to the tensor: taps past the end are out of range (0)
        const int64_t lead = (int64_t)mbase - (W + 1);
        const int64_t last = (int64_t)mbase + BK + (W + 1) < M ? (int64_t)mbase + BK + (W + 1) : M;
        const __amdgpu_buffer_rsrc_t rx = make_rsrc(x + lead * C, clamp_u32((last - lead) * C * 4));
        if (lead < 0) {      // first K-tiles only (wave-uniform): never touch memory in front of the tensor
#pragma unroll
            for (int i = 0; i < 4; ++i)
                r[i] = bload(rx, (mbase + k0 + 8 * i + tapshift < W + 1 || ((bad >> (8 * i)) & 0xFFu)) ? OOB : voff[i], 0);
        } else {
#pragma unroll
            for (int i = 0; i < 4; ++i) r[i] = bload(rx, ((bad >> (8 * i)) & 0xFFu) ? OOB : voff[i], 0);
        }
        nextcode = load_code(kt + 1);
        nextkt = kt + 1;
    }
    __device__ __forceinline__ void finish(float4 (&r)[4]) const {
        if (DSEL) {
#pragma unroll
            for (int i = 0; i < 4; ++i) r[i] = f4sel(((badnow >> (8 * i)) & 0xFFu) == 0, AFFINE ? f4fma(r[i], sc, sh) : r[i]);
        } else if (AFFINE) {
#pragma unroll
            for (int i = 0; i < 4; ++i) r[i] = f4fma(r[i], sc, sh);
        }
    }
};

// codes4[kt * 8 + k0] = codes of pixels kt * 32 + k0 + 8 i in byte i; code bits: 1 h==0, 2 h==H-1, 4 w==0, 8 w==W-1; pixels >= M: 0xF
__global__ __launch_bounds__(256) void border_codes_kernel(uint32_t* __restrict__ codes4, int M, int Mpad, int H, int W) {
    for (int j = blockIdx.x * blockDim.x + threadIdx.x; j < Mpad / 4; j += gridDim.x * blockDim.x) {
        const int kt = j >> 3, k0 = j & 7;
        uint32_t word = 0;
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const int m = kt * 32 + k0 + 8 * i;
            const int w = m % W, h = (m / W) % H;
            const uint32_t c = m < M ? (uint32_t)((h == 0 ? 1 : 0) | (h == H - 1 ? 2 : 0) | (w == 0 ? 4 : 0) | (w == W - 1 ? 8 : 0)) : 0xFu;
            word |= c << (8 * i);
        }
        codes4[j] = word;
    }
}

// Sums of dy over the border pixels of every frame, per output channel: [0] row h = 0, [1] row h = H-1, [2] column w = 0,
// [3] column w = W-1, [4..7] the corners (0,0) (0,W-1) (H-1,0) (H-1,W-1). One block per frame (fp64 sums, one row of
// 8 x Cout per frame), added up over the frames in a fixed order by wgrad_border_u_kernel, which also forms
// U[co][tap] = sum of dy[m][co] over the pixels m at which `tap` falls into the zero padding (inclusion - exclusion).
__global__ __launch_bounds__(256) void wgrad_border_sums_kernel(const float* __restrict__ dy, double* __restrict__ parts,
                                                               int H, int W, int Cout) {
    const int n = blockIdx.x;
    const float* f = dy + (int64_t)n * H * W * Cout;
    double* out = parts + (int64_t)n * 8 * Cout;
    for (int c = threadIdx.x; c < Cout; c += blockDim.x) {
        double r0 = 0, r1 = 0, c0 = 0, c1 = 0;
        for (int w = 0; w < W; ++w) { r0 += (double)f[(int64_t)w * Cout + c]; r1 += (double)f[((int64_t)(H - 1) * W + w) * Cout + c]; }
        for (int h = 0; h < H; ++h) { c0 += (double)f[(int64_t)h * W * Cout + c]; c1 += (double)f[((int64_t)h * W + W - 1) * Cout + c]; }
        out[0 * Cout + c] = r0; out[1 * Cout + c] = r1; out[2 * Cout + c] = c0; out[3 * Cout + c] = c1;
        out[4 * Cout + c] = (double)f[c];
        out[5 * Cout + c] = (double)f[(int64_t)(W - 1) * Cout + c];
        out[6 * Cout + c] = (double)f[(int64_t)(H - 1) * W * Cout + c];
        out[7 * Cout + c] = (double)f[((int64_t)(H - 1) * W + W - 1) * Cout + c];
    }
}

// U[co][tap] of the pixels where `tap` falls into the padding, from the eight border sums v[0..7] of channel co
__device__ __forceinline__ float border_u_of(const double* v, int tap) {
    const int kh = tap / 3, kw = tap - 3 * kh;
    double r = (kh == 0 ? v[0] : 0.0) + (kh == 2 ? v[1] : 0.0) + (kw == 0 ? v[2] : 0.0) + (kw == 2 ? v[3] : 0.0);
    if (kh == 0 && kw == 0) r -= v[4];
    if (kh == 0 && kw == 2) r -= v[5];
    if (kh == 2 && kw == 0) r -= v[6];
    if (kh == 2 && kw == 2) r -= v[7];
    return (float)r;
}

__global__ __launch_bounds__(256) void wgrad_border_u_kernel(const double* __restrict__ parts, int N, int Cout, float* __restrict__ u) {
    __shared__ double s[32][8];
    const int cl = threadIdx.x & 31, j = threadIdx.x >> 5;
    const int c = blockIdx.x * 32 + cl;
    double a0 = 0, a1 = 0, a2 = 0, a3 = 0;
    if (c < Cout) {
        const double* q = parts + (int64_t)j * Cout + c;
        int n = 0;
        for (; n + 3 < N; n += 4) {
            a0 += q[(int64_t)n * 8 * Cout]; a1 += q[(int64_t)(n + 1) * 8 * Cout];
            a2 += q[(int64_t)(n + 2) * 8 * Cout]; a3 += q[(int64_t)(n + 3) * 8 * Cout];
        }
        for (; n < N; ++n) a0 += q[(int64_t)n * 8 * Cout];
    }
    s[cl][j] = (a0 + a1) + (a2 + a3);
    __syncthreads();
    for (int t = threadIdx.x; t < 32 * 9; t += 256) {
        const int cc = t / 9, tap = t - 9 * cc;
        if (blockIdx.x * 32 + cc < Cout) u[(int64_t)(blockIdx.x * 32 + cc) * 9 + tap] = border_u_of(s[cc], tap);
    }
}

// ------------------------------------------------------------------------------------------------
// LDS staging and the MFMA tile
// ------------------------------------------------------------------------------------------------
template <bool KC>
__device__ __forceinline__ void store_tile(float* l, const float4 (&r)[4], int tid) {
    if (KC) {
        const int c4 = (tid & 7) * 4, row = tid >> 3;
#pragma unroll
        for (int i = 0; i < 4; ++i) *reinterpret_cast<float4*>(&l[kc_off(row + 32 * i, c4 >> 2)]) = r[i];
    } else {
        const int r4 = (tid & 31) * 4, k = tid >> 5;
#pragma unroll
        for (int i = 0; i < 4; ++i) *reinterpret_cast<float4*>(&l[(k + 8 * i) * LDR + r4]) = r[i];
    }
}

// Fragment reads of one group (8 k) for the wave's two 32-row fragments of one operand.
//   K-contiguous image (kc_off): one ds_read_b128 per fragment = 4 MFMA steps of that fragment.
//   row-contiguous image [k][128]: one ds_read_b64 per MFMA step serves BOTH fragments: lane r takes rows 2r, 2r+1 of
//     the wave's 64-row strip, i.e. fragment f holds the rows 2i + f (i = MFMA row index) — store_acc() undoes it.
template <bool KC>
__device__ __forceinline__ void read_group(const float* l, int strip, int s, int r, int h, float (&f)[2][4]) {
    if (KC) {
#pragma unroll
        for (int q = 0; q < 2; ++q) {
            const float4 t = *reinterpret_cast<const float4*>(&l[kc_off(strip + q * 32 + r, 2 * s + h)]);
            f[q][0] = t.x; f[q][1] = t.y; f[q][2] = t.z; f[q][3] = t.w;
        }
    } else {
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const float2 t = *reinterpret_cast<const float2*>(&l[(8 * s + 4 * h + j) * LDR + strip + 2 * r]);
            f[0][j] = t.x; f[1][j] = t.y;
        }
    }
}

// One K-tile = 4 groups (8 k each) of 16 MFMAs on the wave's 2 x 2 accumulator tiles.
template <bool AKC, bool BKC>
__device__ __forceinline__ void compute_tile(const float* la, const float* lb, f32x16 (&acc)[2][2],
                                             int wm, int wn, int r, int h) {
#pragma unroll
    for (int s = 0; s < 4; ++s) {
        float a[2][4], b[2][4];
        read_group<AKC>(la, wm * 64, s, r, h, a);
        read_group<BKC>(lb, wn * 64, s, r, h, b);
#pragma unroll
        for (int j = 0; j < 4; ++j) {
#pragma unroll
            for (int fm = 0; fm < 2; ++fm)
#pragma unroll
                for (int fn = 0; fn < 2; ++fn)
                    acc[fm][fn] = __builtin_amdgcn_mfma_f32_32x32x2f32(a[fm][j], b[fn][j], acc[fm][fn], 0, 0, 0);
        }
    }
}

// One K-tile of the strip form: A fragments from the strip rows frag_base() picked for this tap, B as in compute_tile; the
// same MFMA sequence per accumulator as compute_tile.
template <bool BKC>
__device__ __forceinline__ void compute_tile_strip(const float* ls, const float* lb, f32x16 (&acc)[2][2],
                                                   const unsigned (&ab)[2], int wn, int r, int h) {
    static_assert(BKC, "K-contiguous B image");
    // B the same way (two offsets instead of eight loop-invariant addresses: the register budget of three blocks per CU)
    const unsigned bb = (unsigned)kc_off(wn * 64 + r, h) * 4;     // row + 32: the same swizzle, 4 KB further
#pragma unroll
    for (int s = 0; s < 4; ++s) {
        float a[2][4], b[2][4];
#pragma unroll
        for (int q = 0; q < 2; ++q) {
            const float4 t = *reinterpret_cast<const float4*>(reinterpret_cast<const char*>(ls) + (ab[q] ^ (unsigned)(s << 5)));
            a[q][0] = t.x; a[q][1] = t.y; a[q][2] = t.z; a[q][3] = t.w;
            const float4 u = *reinterpret_cast<const float4*>(reinterpret_cast<const char*>(lb) + ((bb ^ (unsigned)(s << 5)) + q * 32 * BK * 4));
            b[q][0] = u.x; b[q][1] = u.y; b[q][2] = u.z; b[q][3] = u.w;
        }
#pragma unroll
        for (int j = 0; j < 4; ++j) {
#pragma unroll
            for (int fm = 0; fm < 2; ++fm)
#pragma unroll
                for (int fn = 0; fn < 2; ++fn)
                    acc[fm][fn] = __builtin_amdgcn_mfma_f32_32x32x2f32(a[fm][j], b[fn][j], acc[fm][fn], 0, 0, 0);
        }
    }
}

// Main loop of the strip form (ConvAStripLoader, no split-K: K-tiles 0 .. 9 chunks - 1): one strip image, one B stage.
template <class AL, class BL>
__device__ __forceinline__ void conv_strip_loop(AL& al, BL& bl, float* ls, float* lb, f32x16 (&acc)[2][2], int ktiles,
                                                int tid, int wn, int r, int h) {
    float4 rs[STRIP_LOADS], rb[4];
    const int nchunks = ktiles / 9;
    if (tid < 8) *reinterpret_cast<float4*>(&ls[STRIP_ROWS * BK + tid * 4]) = f4zero();
    al.begin(0);
#pragma unroll
    for (int i = 0; i < STRIP_LOADS; ++i) rs[i] = al.load(0, i);
    bl.issue(0, rb);
    al.store(ls, rs, tid);
    bl.finish(rb);
    store_tile<BL::KC>(lb, rb, tid);
    __syncthreads();
    for (int chunk = 0; chunk < nchunks; ++chunk) {
        const bool next = chunk + 1 < nchunks;
#pragma unroll
        for (int tap = 0; tap < 9; ++tap) {
            const bool more = tap < 8 || next;
            if (more) bl.issue(chunk * 9 + tap + 1, rb);
            if (next) rs[tap] = al.load(chunk + 1, tap);  // one load of the next chunk's strip per tap, held until tap 8
            unsigned ab[2];
            al.frag_base(tap, ab);
            compute_tile_strip<BL::KC>(ls, lb, acc, ab, wn, r, h);
            __syncthreads();                              // every wave has read the B stage (and, at tap 8, the strip)
            if (more) {
                bl.finish(rb);
                store_tile<BL::KC>(lb, rb, tid);
            }
            if (tap == 8 && next) {
                al.begin(chunk + 1);                      // only now: rb's registers are free for the coefficients
                al.store(ls, rs, tid);
            }
            __syncthreads();
        }
    }
}

// ---- narrow outputs (N <= 64: conv2's data gradient has 64 output channels) -------------------------------------------------
// On the 128-wide tile half of every MFMA multiplied zero columns (measured: 66 TF/s of useful work). N64: the block tile is
// 128 x 64 — the four waves stack along M (32 rows each) and every wave computes 32 x 64 = 1 x 2 MFMA tiles; the LDS images and
// the loaders are unchanged (the B loader's rows 64..127 are out of range and read zeros), only K-contiguous operands.
__device__ __forceinline__ void compute_tile_n64(const float* la, const float* lb, f32x16 (&acc)[2], int wave, int r, int h) {
#pragma unroll
    for (int s = 0; s < 4; ++s) {
        const float4 ta = *reinterpret_cast<const float4*>(&la[kc_off(wave * 32 + r, 2 * s + h)]);
        const float4 tb0 = *reinterpret_cast<const float4*>(&lb[kc_off(r, 2 * s + h)]);
        const float4 tb1 = *reinterpret_cast<const float4*>(&lb[kc_off(32 + r, 2 * s + h)]);
        const float a[4] = {ta.x, ta.y, ta.z, ta.w}, b0[4] = {tb0.x, tb0.y, tb0.z, tb0.w}, b1[4] = {tb1.x, tb1.y, tb1.z, tb1.w};
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            acc[0] = __builtin_amdgcn_mfma_f32_32x32x2f32(a[j], b0[j], acc[0], 0, 0, 0);
            acc[1] = __builtin_amdgcn_mfma_f32_32x32x2f32(a[j], b1[j], acc[1], 0, 0, 0);
        }
    }
}

// epilogue of the 128 x 64 tile: D[row][col], col = lane & 31, row = (reg & 3) + 8 (reg >> 2) + 4 (lane >> 5)
__device__ __forceinline__ void store_acc_n64(const EpiP& ep, const f32x16 (&acc)[2], int tm, int tn, int split, int wave, int r, int h) {
    float* outp = ep.slab_stride > 0 ? (ep.slabs ? ep.slabs : ep.out) + (int64_t)split * ep.slab_stride : ep.out;
    const int mode = ep.slab_stride > 0 ? EPI_RAW : ep.mode;
    const int64_t ld = (ep.slab_stride > 0 && ep.slabs) ? (int64_t)ep.cols : ep.ld;
#pragma unroll
    for (int fn = 0; fn < 2; ++fn) {
        const int col = tn * 64 + fn * 32 + r;
        const bool colok = col < ep.cols;
        const int64_t row0 = (int64_t)tm * BM + wave * 32 + 4 * h;
        const float bv = (mode == EPI_BIAS_RELU && ep.bias) ? ep.bias[colok ? col : 0] : 0.f;
        const float lo = (mode == EPI_BIAS_RELU && ep.relu) ? 0.f : -INFINITY;
#pragma unroll
        for (int e = 0; e < 16; ++e) {
            const int64_t row = row0 + (e & 3) + 8 * (e >> 2);
            if (!(colok && row < ep.rows)) continue;
            const float v = acc[fn][e];
            if (mode == EPI_RAW) outp[row * ld + col] = v;
            else if (mode == EPI_BIAS_RELU) outp[row * ld + col] = fmaxf(v + bv, lo);
            else outp[row * ld + col] = epi_apply(ep, v, row, col);
        }
    }
}

// ---- the epilogue on buffer stores ------------------------------------------------------------------------------------------
// store_acc / store_acc_n64 recompute row * ld + col in 64 bits, compare a 64-bit row and branch for every one of a lane's 64 (32)
// stores: 367 (EPI_RAW) to 510 (EPI_BIAS_RELU) VALU instructions per wave and tile, 128 of them quarter-rate integer multiplies,
// and the fp32 MFMA shares its SIMD's issue slots with them (operand loaders, above). Here the stores go the loaders' way:
//   * one buffer resource per block, based at the tile's first output row, num_records = the tile's true extent
//     ((nrows - 1) ld + cols floats): whatever the addressing does, a store cannot leave the tile's own rows;
//   * the lane's part of the address is a loop-invariant voffset per fragment column (row-in-tile * ld + col, OOB when col >= cols:
//     the range check drops the store), the register's row term (32 fm + (e & 3) + 8 (e >> 2)) ld a scalar offset (SALU);
//   * rows: a tile with all its 128 rows inside the matrix (FULL) stores unconditionally, every row offset being inside num_records
//     by construction; the ragged last row tile selects OOB into the voffset per store. So no result depends on whether the scalar
//     offset takes part in the range check.
// The values are store_acc's: acc, or fmaxf(acc + bias, lo). epi_store_mode() (host) admits EPI_RAW (slabs included) and
// EPI_BIAS_RELU with 128 rows of ld inside one resource; everything else keeps store_acc.
// For a K-contiguous A operand only (fragment fm holds the rows fm * 32 + i). The kernels whose A is row-contiguous, the weight
// gradients, keep store_acc: their gain stayed inside the run-to-run spread, and with the second epilogue compiled in the one-stage
// forms (128 registers) reloaded one more spilled offset per K-tile (profiles/epi_store_kernel_stats.md).
// `pair` (B read row-contiguous = linear dX: a lane's fragments fn = 0, 1 are the adjacent columns 2r, 2r + 1, and cols % 4 == 0
// puts both on the same side of `cols`): one 8-byte store for the two, 256 contiguous bytes per row and half-wave (as adam_acc).
enum { EPI_ST_GLOBAL = 0, EPI_ST_BUF = 1, EPI_ST_BUF_PAIR = 2 };
typedef unsigned int u32x2 __attribute__((ext_vector_type(2)));

template <bool FULL>
__device__ __forceinline__ void bstore(__amdgpu_buffer_rsrc_t rs, float v, unsigned voff, unsigned soff, int rl, int nrows) {
    __builtin_amdgcn_raw_buffer_store_b32(__float_as_uint(v), rs, (int)((FULL || rl < nrows) ? voff : OOB), (int)soff, 0);
}

template <bool BIL, bool FULL>
__device__ __forceinline__ void store_acc_buf(const EpiP& ep, const f32x16 (&acc)[2][2], int tm, int tn, int split, int pair,
                                              int wm, int wn, int r, int h) {
    const bool slab = ep.slab_stride > 0;
    float* outp = slab ? (ep.slabs ? ep.slabs : ep.out) + (int64_t)split * ep.slab_stride : ep.out;
    const int64_t ld = (slab && ep.slabs) ? (int64_t)ep.cols : ep.ld;
    const int64_t trow0 = (int64_t)tm * BM;
    const int nrows = FULL ? BM : (int)(ep.rows - trow0);
    const __amdgpu_buffer_rsrc_t rs = make_rsrc(outp + trow0 * ld, (uint32_t)(((int64_t)(nrows - 1) * ld + ep.cols) * 4));
    const unsigned ld4 = (unsigned)ld * 4u;
    const int rl0 = wm * 64 + 4 * h;                                  // the lane's first row in the tile (fragment fm = 0)
    unsigned voff[2];
    float bv[2];
    const bool relu_mode = !slab && ep.mode == EPI_BIAS_RELU;
#pragma unroll
    for (int fn = 0; fn < 2; ++fn) {
        const int col = tn * BN + wn * 64 + (BIL ? 2 * r + fn : fn * 32 + r);
        voff[fn] = col < ep.cols ? (unsigned)rl0 * ld4 + (unsigned)col * 4u : OOB;
        bv[fn] = (relu_mode && ep.bias) ? ep.bias[col < ep.cols ? col : 0] : 0.f;
    }
    if (relu_mode) {
        const float lo = ep.relu ? 0.f : -INFINITY;
#pragma unroll
        for (int fm = 0; fm < 2; ++fm)
#pragma unroll
            for (int fn = 0; fn < 2; ++fn)
#pragma unroll
                for (int e = 0; e < 16; ++e) {
                    const int dr = fm * 32 + (e & 3) + 8 * (e >> 2);
                    bstore<FULL>(rs, fmaxf(acc[fm][fn][e] + bv[fn], lo), voff[fn], (unsigned)dr * ld4, rl0 + dr, nrows);
                }
        return;
    }
    if constexpr (BIL) {
        if (pair) {
#pragma unroll
            for (int fm = 0; fm < 2; ++fm)
#pragma unroll
                for (int e = 0; e < 16; ++e) {
                    const int dr = fm * 32 + (e & 3) + 8 * (e >> 2);
                    const u32x2 v = {__float_as_uint(acc[fm][0][e]), __float_as_uint(acc[fm][1][e])};
                    __builtin_amdgcn_raw_buffer_store_b64(v, rs, (int)((FULL || rl0 + dr < nrows) ? voff[0] : OOB), (int)((unsigned)dr * ld4), 0);
                }
            return;
        }
    }
#pragma unroll
    for (int fm = 0; fm < 2; ++fm)
#pragma unroll
        for (int fn = 0; fn < 2; ++fn)
#pragma unroll
            for (int e = 0; e < 16; ++e) {
                const int dr = fm * 32 + (e & 3) + 8 * (e >> 2);
                bstore<FULL>(rs, acc[fm][fn][e], voff[fn], (unsigned)dr * ld4, rl0 + dr, nrows);
            }
}

// the same for the 128 x 64 tile (store_acc_n64): the wave's rows are wave * 32 + 4 h + (e & 3) + 8 (e >> 2)
template <bool FULL>
__device__ __forceinline__ void store_acc_n64_buf(const EpiP& ep, const f32x16 (&acc)[2], int tm, int tn, int split, int wave, int r, int h) {
    const bool slab = ep.slab_stride > 0;
    float* outp = slab ? (ep.slabs ? ep.slabs : ep.out) + (int64_t)split * ep.slab_stride : ep.out;
    const int64_t ld = (slab && ep.slabs) ? (int64_t)ep.cols : ep.ld;
    const int64_t trow0 = (int64_t)tm * BM;
    const int nrows = FULL ? BM : (int)(ep.rows - trow0);
    const __amdgpu_buffer_rsrc_t rs = make_rsrc(outp + trow0 * ld, (uint32_t)(((int64_t)(nrows - 1) * ld + ep.cols) * 4));
    const unsigned ld4 = (unsigned)ld * 4u;
    const int rl0 = wave * 32 + 4 * h;
    const bool relu_mode = !slab && ep.mode == EPI_BIAS_RELU;
    const float lo = (relu_mode && ep.relu) ? 0.f : -INFINITY;
#pragma unroll
    for (int fn = 0; fn < 2; ++fn) {
        const int col = tn * 64 + fn * 32 + r;
        const unsigned voff = col < ep.cols ? (unsigned)rl0 * ld4 + (unsigned)col * 4u : OOB;
        const float bv = (relu_mode && ep.bias) ? ep.bias[col < ep.cols ? col : 0] : 0.f;
        if (relu_mode) {
#pragma unroll
            for (int e = 0; e < 16; ++e) {
                const int dr = (e & 3) + 8 * (e >> 2);
                bstore<FULL>(rs, fmaxf(acc[fn][e] + bv, lo), voff, (unsigned)dr * ld4, rl0 + dr, nrows);
            }
        } else {
#pragma unroll
            for (int e = 0; e < 16; ++e) {
                const int dr = (e & 3) + 8 * (e >> 2);
                bstore<FULL>(rs, acc[fn][e], voff, (unsigned)dr * ld4, rl0 + dr, nrows);
            }
        }
    }
}

// The K loop of one output tile as a function: loaders, LDS staging and MFMAs for K-tiles [kt0, kt1) of tile (tm, tn) into the
// wave's 2 x 2 accumulator tiles (128 x 128 tile, per-K-tile loaders). gemm_f32_epi_kernel runs it; gemm_f32_kernel keeps its own
// inline copy of the same statements: calling this function from it changed the register allocation of every instantiation
// (VGPRs and spills moved by 1-7), and those kernels are to compile as they did.
template <class AL, class BL, int STAGES>
__device__ __forceinline__ void gemm_mainloop(const typename AL::P& ap, const typename BL::P& bp, int tm, int tn, int kt0, int kt1,
                                              int tid, f32x16 (&acc)[2][2]) {
    static_assert(!AL::STRIP, "per-K-tile A loaders only");
    AL al(ap, tm * BM, tid);
    BL bl(bp, tn * BN, tid);

    const int lane = tid & 63, wave = tid >> 6;
    const int wm = wave >> 1, wn = wave & 1;
    const int r = lane & 31, h = lane >> 5;

#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int j = 0; j < 2; ++j)
#pragma unroll
            for (int e = 0; e < 16; ++e) acc[i][j][e] = 0.f;

    __shared__ __attribute__((aligned(16))) float lds[STAGES][2][OP_FLOATS];
    float4 ra[4], rb[4];
    if (kt0 < kt1) {
        al.issue(kt0, ra);
        bl.issue(kt0, rb);
        al.finish(ra);
        bl.finish(rb);
        store_tile<AL::KC>(lds[0][0], ra, tid);
        store_tile<BL::KC>(lds[0][1], rb, tid);
    }
    __syncthreads();
    for (int kt = kt0; kt < kt1; ++kt) {
        const int cur = STAGES == 1 ? 0 : (kt - kt0) & 1;
        const bool more = kt + 1 < kt1;
        if (more) {
            // the buffer being filled was last read in iteration kt-1, which every wave left through the barrier
            al.issue(kt + 1, ra);
            bl.issue(kt + 1, rb);
        }
        compute_tile<AL::KC, BL::KC>(lds[cur][0], lds[cur][1], acc, wm, wn, r, h);
        if constexpr (STAGES == 1) __syncthreads();      // one LDS stage: every wave has read it
        if (more) {
            al.finish(ra);
            bl.finish(rb);
            store_tile<AL::KC>(lds[STAGES == 1 ? 0 : cur ^ 1][0], ra, tid);
            store_tile<BL::KC>(lds[STAGES == 1 ? 0 : cur ^ 1][1], rb, tid);
        }
        __syncthreads();
    }
}

// ---- the kernel: 256 threads, every wave stages and computes, 2 blocks per CU ---------------------------------------
// Measured ceilings on conv3 forward (scripts/bench_gemm.py, N = 128, 2.37 GHz): 147 TFLOP/s with no staging in the
// loop, 135 with only the global loads or only the LDS writes, 127 with both. Two restructurings were built, found
// correct and measured without gain, and removed again (git history): 4 MFMA-only consumer waves + 4 staging-only
// producer waves per block (122), and LDS-DMA (`buffer_load ... lds`) staging of the operands that need no
// transform (123-127): the cost follows the bytes moved into LDS, not the instruction mix of the MFMA waves.
// Round 2: a two-deep register prefetch for the weight gradient (loads of K-tile kt + 2 issued before the MFMAs of tile kt,
// two register sets and loader instances alternating; 248 VGPRs, no spill) measured 116.4 vs 116.6 TF/s at 128 frames:
// memory latency is not what holds it at 0.69-0.74 of peak either. Removed.
// Kept: the strip A loader of the 3x3 convolution (ConvAStripLoader, `if constexpr (AL::STRIP)` below). It does not move the
// same bytes differently, it moves fewer: the nine K-tiles of a channel chunk are windows of one pixel strip, staged once
// (A bytes into LDS 144 -> 36 KB per chunk and block, the affine once per element, no select). 1024 frames, alternating in one
// process (scripts/bench_conv_strip.py, profiles/conv_strip_kernel_stats.md): conv3 forward 92.9 -> 88.0 ms (134.8 -> 142.2
// TF/s), conv3 data gradient 90.0 -> 86.5 (139.2 -> 144.8; three blocks per CU instead of four), conv2 forward 13.56 -> 12.54
// (122.0 -> 131.9); outputs bit-identical.
template <class AL, class BL, bool N64 = false, int STAGES = 2>
__global__ __launch_bounds__(256, STAGES == 1 ? (N64 ? 4 : AL::ONE_STAGE_BLOCKS) : 2) void gemm_f32_kernel(typename AL::P ap, typename BL::P bp, EpiP ep,
                                                          int tiles_m, int tiles_n, int flags,
                                                          int ktiles, int ktiles_per_split, int xcd_splits) {
    // flags: bit 0 = tiles walk M fastest, bits 1.. = EPI_ST_* (one word, so that the kernels keep their signature and with it
    // the names the profiles and bench.py know them by)
    const int m_fast = flags & 1, epi_st = flags >> 1;
    const int tid = threadIdx.x;
    int tm, tn, split;
    if (xcd_splits > 0) {
        // XCD-local split-K: blocks b, b + 8, ... share an XCD (round-robin dispatch) and start in that order, so XCD x walks
        // splits x, x + 8, ... with ALL output tiles of a split resident together: the split's slice of both operands is
        // fetched into that XCD's L2 once and re-hit by the other tiles, instead of once per XCD (profiles/r02_traffic.md)
        const int tiles = tiles_m * tiles_n;
        const int xcd = blockIdx.x & 7, j = blockIdx.x >> 3;
        int t;
        if (tiles > 64 && tiles <= 128) {
            // conv3's weight gradient has 72 tiles per split but an XCD holds 64 blocks: in plain order every round of 64 mixes
            // the tail of one split with the head of the next (two pixel ranges streaming through the L2 at once). Two-phase
            // order: first, per split, the 64 tiles that fill the XCD exactly (one pixel range at a time); then the remaining
            // tiles - 64 of all of the XCD's splits together.
            const int gs = (xcd_splits + 7) / 8, rest = tiles - 64, nA = gs * 64;
            int q;
            if (j < nA) { q = j >> 6; t = j & 63; }
            else { const int i = j - nA; q = i / rest; t = 64 + (i - q * rest); }
            split = q * 8 + xcd;
        } else {
            split = (j / tiles) * 8 + xcd;
            t = j - (j / tiles) * tiles;
        }
        if (split >= xcd_splits) return;                  // the grid is padded to whole groups of 8 splits
        if (m_fast) { tm = t % tiles_m; tn = t / tiles_m; } else { tn = t % tiles_n; tm = t / tiles_n; }
    } else {
        tile_of_block(tiles_m, tiles_n, m_fast, tm, tn);
        split = blockIdx.y;
    }
    const int kt0 = split * ktiles_per_split;
    const int kt1 = min(ktiles, kt0 + ktiles_per_split);

    static_assert(!N64 || (AL::KC && BL::KC), "the 128 x 64 tile reads K-contiguous LDS images");
    AL al(ap, tm * BM, tid);
    BL bl(bp, tn * (N64 ? 64 : BN), tid);

    const int lane = tid & 63, wave = tid >> 6;
    const int wm = wave >> 1, wn = wave & 1;
    const int r = lane & 31, h = lane >> 5;

    f32x16 acc[2][2];
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int j = 0; j < 2; ++j)
#pragma unroll
            for (int e = 0; e < 16; ++e) acc[i][j][e] = 0.f;

    if constexpr (AL::STRIP) {
        static_assert(!N64 && STAGES == 1 && BL::KC, "the strip form: 128 x 128 tile, one B stage");
        __shared__ __attribute__((aligned(16))) float lstrip[STRIP_FLOATS];
        __shared__ __attribute__((aligned(16))) float lbs[OP_FLOATS];
        conv_strip_loop(al, bl, lstrip, lbs, acc, kt1 - kt0, tid, wn, r, h);
    } else {
        __shared__ __attribute__((aligned(16))) float lds[STAGES][2][OP_FLOATS];
        float4 ra[4], rb[4];
        if (kt0 < kt1) {
            al.issue(kt0, ra);
            bl.issue(kt0, rb);
            al.finish(ra);
            bl.finish(rb);
            store_tile<AL::KC>(lds[0][0], ra, tid);
            store_tile<BL::KC>(lds[0][1], rb, tid);
        }
        __syncthreads();
        for (int kt = kt0; kt < kt1; ++kt) {
            const int cur = STAGES == 1 ? 0 : (kt - kt0) & 1;
            const bool more = kt + 1 < kt1;
            if (more) {
                // the buffer being filled was last read in iteration kt-1, which every wave left through the barrier
                al.issue(kt + 1, ra);
                bl.issue(kt + 1, rb);
            }
            if constexpr (N64) compute_tile_n64(lds[cur][0], lds[cur][1], acc[0], wave, r, h);
            else compute_tile<AL::KC, BL::KC>(lds[cur][0], lds[cur][1], acc, wm, wn, r, h);
            if constexpr (STAGES == 1) __syncthreads();      // one LDS stage (32 KB: three blocks per CU): every wave has read it
            if (more) {
                al.finish(ra);
                bl.finish(rb);
                store_tile<AL::KC>(lds[STAGES == 1 ? 0 : cur ^ 1][0], ra, tid);
                store_tile<BL::KC>(lds[STAGES == 1 ? 0 : cur ^ 1][1], rb, tid);
            }
            __syncthreads();
        }
    }
    const bool full = (int64_t)tm * BM + BM <= ep.rows;      // wave-uniform, as epi_st: one epilogue per block
    if constexpr (N64) {
        if (epi_st == EPI_ST_GLOBAL) store_acc_n64(ep, acc[0], tm, tn, split, wave, r, h);
        else if (full) store_acc_n64_buf<true>(ep, acc[0], tm, tn, split, wave, r, h);
        else store_acc_n64_buf<false>(ep, acc[0], tm, tn, split, wave, r, h);
    } else if constexpr (!AL::KC) {                          // the weight gradients: store_acc only (see store_acc_buf)
        store_acc<true, !BL::KC>(ep, acc, tm, tn, split, wm, wn, r, h);
    } else {
        if (epi_st == EPI_ST_GLOBAL) store_acc<false, !BL::KC>(ep, acc, tm, tn, split, wm, wn, r, h);
        else if (full) store_acc_buf<!BL::KC, true>(ep, acc, tm, tn, split, epi_st == EPI_ST_BUF_PAIR, wm, wn, r, h);
        else store_acc_buf<!BL::KC, false>(ep, acc, tm, tn, split, epi_st == EPI_ST_BUF_PAIR, wm, wn, r, h);
    }
    if (ep.tile_ctr) {                                       // fused split-K reduction: the tile's last block sums the slabs
        const int nsp = (ktiles + ktiles_per_split - 1) / ktiles_per_split;
        fused_splitk_reduce<N64 ? 64 : BN>(ep, tm, tn, tm * tiles_n + tn, nsp, tid);
    }
}

// ---- epilogues that consume the accumulators instead of (only) storing them ------------------------------------------
// gemm_f32_epi_kernel is gemm_f32_kernel's loop (gemm_mainloop) under an epilogue picked by a TEMPLATE parameter: a runtime
// branch inside store_acc's unrolled loop once sent the accumulators to scratch (gemm_common.h, EpiP::oscale). It is a
// kernel of its own, so the instantiations of gemm_f32_kernel keep their names (bench.py and the profiles name kernels by
// them) and their code. No split-K, 128 x 128 tile.
//
// EPIK_ADAM (linear5's weight gradient): the tile's accumulators ARE the gradient of 128 x 128 elements of the weight, and
// dw[j][k] (ld = K) is the arena layout, so p, m and v are addressed by the gradient's own index: load p / m / v, adam1,
// store p / m / v. No gradient is written; the 5.1 GB round trip of dW through HBM and the stand-alone pass's launch go, and
// the update's 30.8 GB move under an MFMA-bound kernel. With both operands row-contiguous a lane's fragments fn = 0, 1 are
// the adjacent columns 2r, 2r + 1: 8-byte accesses, 256 B contiguous per row and half-wave.
enum { EPIK_ADAM = 1 };

struct AdamEpi {
    float* p; float* m; float* v;
    double lr, beta1, beta2;
    float eps, gs;
    const int64_t* step; int64_t step_bias;
};

__device__ __forceinline__ float wave_uniform(float x) { return __int_as_float(__builtin_amdgcn_readfirstlane(__float_as_int(x))); }

// rows = J, cols = K (a multiple of 4: a lane's column pair is inside or outside together), ld = K.
__device__ __forceinline__ void adam_acc(const AdamEpi& ae, const AdamScalars& s, int rows, int cols, int64_t ld,
                                         const f32x16 (&acc)[2][2], int tm, int tn, int wm, int wn, int r, int h) {
    const int col = tn * GEMM_BN + wn * 64 + 2 * r;
    const bool colok = col < cols;
#pragma unroll
    for (int fm = 0; fm < 2; ++fm) {
        const int row0 = tm * GEMM_BM + wm * 64 + fm + 8 * h;
#pragma unroll
        for (int eb = 0; eb < 4; ++eb) {
            // four rows at a time: 12 loads in flight, then the arithmetic, then the stores. Lanes outside the matrix load
            // element 0 (a valid address) and store nothing: no branch around a load.
            float2 pp[4], mm[4], vv[4];
            int64_t idx[4];
            bool ok[4];
#pragma unroll
            for (int q = 0; q < 4; ++q) {
                const int row = row0 + 2 * (q + 8 * eb);
                ok[q] = colok && row < rows;
                idx[q] = ok[q] ? (int64_t)row * ld + col : 0;
                pp[q] = *reinterpret_cast<const float2*>(ae.p + idx[q]);
                mm[q] = *reinterpret_cast<const float2*>(ae.m + idx[q]);
                vv[q] = *reinterpret_cast<const float2*>(ae.v + idx[q]);
            }
#pragma unroll
            for (int q = 0; q < 4; ++q) {
                const int e = 4 * eb + q;
                adam1(pp[q].x, acc[fm][0][e], mm[q].x, vv[q].x, s.b2, s.omb1, s.omb2, ae.eps, s.step_size, s.bc2_sqrt, ae.gs);
                adam1(pp[q].y, acc[fm][1][e], mm[q].y, vv[q].y, s.b2, s.omb1, s.omb2, ae.eps, s.step_size, s.bc2_sqrt, ae.gs);
            }
#pragma unroll
            for (int q = 0; q < 4; ++q) {
                if (ok[q]) {
                    *reinterpret_cast<float2*>(ae.p + idx[q]) = pp[q];
                    *reinterpret_cast<float2*>(ae.m + idx[q]) = mm[q];
                    *reinterpret_cast<float2*>(ae.v + idx[q]) = vv[q];
                }
            }
        }
    }
}

template <class AL, class BL, int STAGES, int EPI>
__global__ __launch_bounds__(256, STAGES == 1 ? AL::ONE_STAGE_BLOCKS : 2) void gemm_f32_epi_kernel(typename AL::P ap, typename BL::P bp, AdamEpi ae,
                                                          int rows, int cols, int64_t ld, int tiles_m, int tiles_n, int m_fast, int ktiles) {
    static_assert(EPI == EPIK_ADAM && !AL::KC && !BL::KC, "the Adam epilogue: both operands row-contiguous");
    const int tid = threadIdx.x;
    int tm, tn;
    tile_of_block(tiles_m, tiles_n, m_fast, tm, tn);
    // the step's scalars before the loop, while no accumulator is live (fp64 pow), kept in scalar registers through it
    AdamScalars s = adam_scalars(ae.lr, ae.beta1, ae.beta2, *ae.step + ae.step_bias);
    s.step_size = wave_uniform(s.step_size); s.bc2_sqrt = wave_uniform(s.bc2_sqrt);
    s.b2 = wave_uniform(s.b2); s.omb1 = wave_uniform(s.omb1); s.omb2 = wave_uniform(s.omb2);
    const int lane = tid & 63, wave = tid >> 6;
    const int wm = wave >> 1, wn = wave & 1;
    const int r = lane & 31, h = lane >> 5;
    f32x16 acc[2][2];
    gemm_mainloop<AL, BL, STAGES>(ap, bp, tm, tn, 0, ktiles, tid, acc);
    adam_acc(ae, s, rows, cols, ld, acc, tm, tn, wm, wn, r, h);
}

template <class AL, class BL, int EPI>
int launch_gemm_epi(const char* name, const typename AL::P& ap, const typename BL::P& bp, const AdamEpi& ae, int64_t M, int64_t N,
                    int64_t ld, int ktiles, int m_fast, hipStream_t st) {
    const int64_t tiles_m = (M + BM - 1) / BM, tiles_n = (N + BN - 1) / BN;
    GN_REQUIRE(tiles_m * tiles_n < (1ll << 31), GOALNET_E_SHAPE, "%s: too many tiles", name);
    static const int force_stages = getenv("GOALNET_F32_STAGES") ? atoi(getenv("GOALNET_F32_STAGES")) : 0;      // as launch_gemm
    const dim3 grid((unsigned)(tiles_m * tiles_n), 1, 1);
    if (force_stages == 1 || (force_stages != 2 && AL::ONE_STAGE))
        hipLaunchKernelGGL((gemm_f32_epi_kernel<AL, BL, 1, EPI>), grid, dim3(256), 0, st, ap, bp, ae, (int)M, (int)N, ld, (int)tiles_m,
                           (int)tiles_n, m_fast, ktiles);
    else
        hipLaunchKernelGGL((gemm_f32_epi_kernel<AL, BL, 2, EPI>), grid, dim3(256), 0, st, ap, bp, ae, (int)M, (int)N, ld, (int)tiles_m,
                           (int)tiles_n, m_fast, ktiles);
    GN_LAUNCH_CHECK(name);
    return 0;
}

// sums `nsplit` raw slabs (deterministic order) and applies the epilogue. cols % 4 == 0.
__global__ __launch_bounds__(256) void splitk_reduce_kernel(const float* slabs, int nsplit, int64_t slab_stride, EpiP ep) {
    const int c4n = ep.cols >> 2;
    const int64_t total = (int64_t)ep.rows * c4n;
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (int64_t)gridDim.x * blockDim.x) {
        const int64_t row = i / c4n;
        const int col = (int)(i - row * c4n) * 4;
        const float* s = slabs + row * ep.cols + col;
        float4 a = *reinterpret_cast<const float4*>(s);
        for (int k = 1; k < nsplit; ++k) {
            const float4 b = *reinterpret_cast<const float4*>(s + (int64_t)k * slab_stride);
            a.x += b.x; a.y += b.y; a.z += b.z; a.w += b.w;
        }
        if (ep.oscale) { const int k = *ep.oscale; a.x = ldexpf(a.x, k); a.y = ldexpf(a.y, k); a.z = ldexpf(a.z, k); a.w = ldexpf(a.w, k); }   // scaled fp16 operands
        if (ep.corr_u) {       // fp32 conv weight gradient: what the padding taps accumulated through the BatchNorm shift
            const int tap = col / ep.corr_C, ci = col - tap * ep.corr_C;
            const float u = ep.corr_u[row * 9 + tap];
            const float4 shv = *reinterpret_cast<const float4*>(ep.corr_sh + ci);
            a.x = fmaf(-shv.x, u, a.x); a.y = fmaf(-shv.y, u, a.y); a.z = fmaf(-shv.z, u, a.z); a.w = fmaf(-shv.w, u, a.w);
        }
        float* o = ep.out + row * ep.ld + col;
        o[0] = epi_apply(ep, a.x, row, col);
        o[1] = epi_apply(ep, a.y, row, col + 1);
        o[2] = epi_apply(ep, a.z, row, col + 2);
        o[3] = epi_apply(ep, a.w, row, col + 3);
    }
}

// Few outputs, many slabs (the weight-streaming forward at <= 16 rows: 5 120 outputs x 81 slabs): 16 lanes (a DPP row) share
// one float4 of output, lane g sums slabs g, g+16, ...; row16_sum adds the 16 partial sums in a fixed order.
__global__ __launch_bounds__(256) void splitk_reduce_wide_kernel(const float* slabs, int nsplit, int64_t slab_stride, EpiP ep) {
    const int c4n = ep.cols >> 2;
    const int64_t total = (int64_t)ep.rows * c4n;
    const int g = threadIdx.x & 15;
    const int64_t step = (int64_t)gridDim.x * 16;
    const int64_t rounds = (total + step - 1) / step;                 // whole DPP rows stay together
    int64_t i = (int64_t)blockIdx.x * 16 + (threadIdx.x >> 4);
    for (int64_t r = 0; r < rounds; ++r, i += step) {
        const bool ok = i < total;
        const int64_t ic = ok ? i : 0;
        const int64_t row = ic / c4n;
        const int col = (int)(ic - row * c4n) * 4;
        const float* s = slabs + row * ep.cols + col;
        float4 a = make_float4(0.f, 0.f, 0.f, 0.f);
        for (int k = g; k < nsplit; k += 16) {
            const float4 b = *reinterpret_cast<const float4*>(s + (int64_t)k * slab_stride);
            a.x += b.x; a.y += b.y; a.z += b.z; a.w += b.w;
        }
        a.x = row16_sum(a.x); a.y = row16_sum(a.y); a.z = row16_sum(a.z); a.w = row16_sum(a.w);
        if (ep.oscale) { const int k = *ep.oscale; a.x = ldexpf(a.x, k); a.y = ldexpf(a.y, k); a.z = ldexpf(a.z, k); a.w = ldexpf(a.w, k); }
        if (ep.corr_u) {       // as in splitk_reduce_kernel
            const int tap = col / ep.corr_C, ci = col - tap * ep.corr_C;
            const float u = ep.corr_u[row * 9 + tap];
            const float4 shv = *reinterpret_cast<const float4*>(ep.corr_sh + ci);
            a.x = fmaf(-shv.x, u, a.x); a.y = fmaf(-shv.y, u, a.y); a.z = fmaf(-shv.z, u, a.z); a.w = fmaf(-shv.w, u, a.w);
        }
        if (ok && g == 0) {
            float* o = ep.out + row * ep.ld + col;
            o[0] = epi_apply(ep, a.x, row, col);
            o[1] = epi_apply(ep, a.y, row, col + 1);
            o[2] = epi_apply(ep, a.z, row, col + 2);
            o[3] = epi_apply(ep, a.w, row, col + 3);
        }
    }
}

// Which epilogue a launch takes (store_acc_buf, above). The buffer stores serve what a tile with a K-contiguous A operand writes as
// EPI_RAW (slabs included) or EPI_BIAS_RELU when 128 rows of the output's leading dimension fit one buffer resource; a wider `ld`,
// EPI_MUL / EPI_FULL and a row-contiguous A (the weight gradients) keep store_acc. 8-byte stores for linear dX, the role where they measured faster (profiles/epi_store_kernel_stats.md). GOALNET_F32_EPI_STORE,
// read per call: 0 forces store_acc everywhere, 1 the 4-byte buffer stores everywhere they apply (tests, A/B runs).
constexpr bool EPI_PAIR_DX = true;           // A K-contiguous, B row-contiguous: linear dX
static int epi_store_mode(const EpiP& ep, bool a_kc, bool b_kc) {
    const char* e = getenv("GOALNET_F32_EPI_STORE");
    if ((e && e[0] == '0') || !a_kc) return EPI_ST_GLOBAL;
    const bool slab = ep.slab_stride > 0;
    const int mode = slab ? EPI_RAW : ep.mode;
    const int64_t ld = (slab && ep.slabs) ? (int64_t)ep.cols : ep.ld;
    if (mode != EPI_RAW && mode != EPI_BIAS_RELU) return EPI_ST_GLOBAL;
    if (ep.rows <= 0 || ep.cols <= 0 || ld < ep.cols || (int64_t)BM * ld * 4 >= 0xFFFFFF00ll) return EPI_ST_GLOBAL;
    if (e && e[0] == '1') return EPI_ST_BUF;
    return (EPI_PAIR_DX && !b_kc && mode == EPI_RAW) ? EPI_ST_BUF_PAIR : EPI_ST_BUF;
}

template <class AL, class BL, bool N64 = false>
int launch_gemm(const char* name, const typename AL::P& ap, const typename BL::P& bp, const EpiP& ep,
                int64_t M, int64_t N, int ktiles, int nsplit, int m_fast, hipStream_t st) {
    const int64_t tiles_m = (M + BM - 1) / BM, tiles_n = (N + (N64 ? 64 : BN) - 1) / (N64 ? 64 : BN);
    GN_REQUIRE(tiles_m * tiles_n < (1ll << 31), GOALNET_E_SHAPE, "%s: too many tiles", name);
    GN_REQUIRE(nsplit >= 1 && nsplit <= 65535, GOALNET_E_SHAPE, "%s: bad split count %d", name, nsplit);
    const int kps = (ktiles + nsplit - 1) / nsplit;
    GN_REQUIRE(!ep.tile_ctr || (ktiles + kps - 1) / kps == nsplit, GOALNET_E_SHAPE, "%s: fused split-K needs every split non-empty", name);
    // >= 8 splits whose tiles fit an XCD's 64 resident blocks a few times over: XCD-local order (see the kernel)
    const bool xcd_local = nsplit >= 8 && tiles_m * tiles_n <= 256 && tiles_m * tiles_n * ((nsplit + 7) / 8 * 8) < (1ll << 31);
    dim3 grid((unsigned)(tiles_m * tiles_n), (unsigned)nsplit, 1);
    if (xcd_local) grid = dim3((unsigned)(tiles_m * tiles_n * ((nsplit + 7) / 8 * 8)), 1, 1);
    // One LDS stage (32 KB, two barriers per K-tile) lets three blocks share a CU instead of two: while one block sits in its
    // barrier / staging section two others have matrix work. Measured at 128 frames (TF/s, two stages -> one): conv3 forward
    // 130.4 -> 134.7, data gradient 133.4 -> 140.4, weight gradient 132.1 -> 133.4, conv2 forward 105.7 -> 109.5, linear5 dW
    // 91.3 -> 96.1; linear5 forward 121.9 -> 99.7 and dX 116.4 -> 114.7 (a K-contiguous A operand with a 10 MB row stride): by
    // the A loader's trait. GOALNET_F32_STAGES=1|2 forces one form (tests, A/B runs).
    static const int force_stages = getenv("GOALNET_F32_STAGES") ? atoi(getenv("GOALNET_F32_STAGES")) : 0;
    const int epi_st = epi_store_mode(ep, AL::KC, BL::KC);
    const bool one_stage = AL::STRIP || force_stages == 1 || (force_stages != 2 && AL::ONE_STAGE);     // the strip form has no two-stage variant
    if (one_stage) {        // the 128 x 64 tile as well: conv2's data gradient 108.9 -> 123.1 TF/s
        hipLaunchKernelGGL((gemm_f32_kernel<AL, BL, N64, 1>), grid, dim3(256), 0, st, ap, bp, ep, (int)tiles_m, (int)tiles_n,
                           (m_fast & 1) | (epi_st << 1), ktiles, kps, xcd_local ? nsplit : 0);
        GN_LAUNCH_CHECK(name);
        return 0;
    }
    if constexpr (!AL::STRIP) {
        hipLaunchKernelGGL((gemm_f32_kernel<AL, BL, N64>), grid, dim3(256), 0, st, ap, bp, ep, (int)tiles_m, (int)tiles_n,
                           (m_fast & 1) | (epi_st << 1), ktiles, kps, xcd_local ? nsplit : 0);
        GN_LAUNCH_CHECK(name);
    }
    return 0;
}

}  // namespace

namespace goalnet {
int launch_splitk_reduce(const char* name, const float* slabs, int nsplit, int64_t slab_stride, const EpiP& ep, hipStream_t st) {
    const int64_t total = (int64_t)ep.rows * (ep.cols >> 2);
    int64_t blocks = (total + 255) / 256;
    if (blocks > 4096) blocks = 4096;
    if (blocks < 1) blocks = 1;
    if (total < 65536 && nsplit >= 32) {
        int64_t wb = (total + 15) / 16;
        if (wb > 4096) wb = 4096;
        hipLaunchKernelGGL(splitk_reduce_wide_kernel, dim3((unsigned)wb), dim3(256), 0, st, slabs, nsplit, slab_stride, ep);
        GN_LAUNCH_CHECK(name);
        return 0;
    }
    hipLaunchKernelGGL(splitk_reduce_kernel, dim3((unsigned)blocks), dim3(256), 0, st, slabs, nsplit, slab_stride, ep);
    GN_LAUNCH_CHECK(name);
    return 0;
}

// split count so that the grid has about 1024 blocks but every split keeps >= 8 K-tiles
int pick_splits(int64_t tiles, int ktiles) {
    if (ktiles < 8 || (ktiles < 64 && tiles >= 128)) return 1;
    // short reductions with few output tiles (the fusion MLP at hundreds of frames: 8 - 40 tiles, 8 - 32 K-tiles) left most
    // CUs idle: ~256 blocks of >= 4 K-tiles each
    int64_t s = ((ktiles < 64 ? 256 : 1024) + tiles - 1) / tiles;
    const int64_t smax = ktiles < 64 ? ktiles / 4 : (ktiles / 8 > 1 ? ktiles / 8 : 1);
    if (s > smax) s = smax;
    if (s < 1) s = 1;
    const int kps = (int)((ktiles + s - 1) / s);
    return (ktiles + kps - 1) / kps;   // no empty splits
}

}  // namespace goalnet

// =================================================================================================
// C ABI
// =================================================================================================
extern "C" {

static int conv_splits_f32(int64_t M, int Cin, int Cout) {
    return conv_fwd_splits(((M + BM - 1) / BM) * ((Cout + BN - 1) / BN), 9 * Cin / BK);
}

// The strip A loader (ConvAStripLoader) serves a call when there is no split-K (it walks whole chunks), the strip fits
// its LDS image (W <= 79), the tile is 128 x 128 and the role is one where it measured faster: both did
// (profiles/conv_strip_kernel_stats.md). GOALNET_F32_CONV_STRIP=0, read per call, forces the per-tap loader (tests, A/B runs).
constexpr bool CONV_STRIP_FWD = true;        // with the affine: the forward
constexpr bool CONV_STRIP_DGRAD = true;      // without: the data gradient on flipped weights
static bool conv_strip_f32(int W, int nsplit, bool narrow, bool affine) {
    const char* e = getenv("GOALNET_F32_CONV_STRIP");
    if (e && e[0] == '0') return false;
    return nsplit == 1 && !narrow && W <= CONV_STRIP_MAX_W && (affine ? CONV_STRIP_FWD : CONV_STRIP_DGRAD);
}

size_t goalnet_conv3x3_fwd_ws_bytes(int N, int H, int W, int Cin, int Cout) {
    if (N <= 0 || H <= 0 || W <= 0 || Cin <= 0 || Cout <= 0) return 0;
    const int64_t M = (int64_t)N * H * W;
    const int s = conv_splits_f32(M, Cin, Cout);
    return s > 1 ? (size_t)s * (size_t)M * (size_t)Cout * sizeof(float) : 0;
}

int goalnet_conv3x3_fwd(const float* x, const float* scale, const float* shift, const float* w,
                        const float* bias, int relu, float* y, int N, int H, int W, int Cin, int Cout,
                        void* ws, size_t ws_bytes, int* tile_ctr, int n_ctr, void* stream) {
    GN_REQUIRE(x && w && y, GOALNET_E_NULL, "conv3x3_fwd: null pointer");
    GN_REQUIRE((scale == nullptr) == (shift == nullptr), GOALNET_E_NULL, "conv3x3_fwd: scale/shift must both be set or both NULL");
    GN_REQUIRE(N > 0 && H > 0 && W > 0 && Cin > 0 && Cout > 0, GOALNET_E_SHAPE, "conv3x3_fwd: non-positive dim");
    GN_REQUIRE(Cin % BK == 0, GOALNET_E_SHAPE, "conv3x3_fwd: Cin=%d must be a multiple of %d", Cin, BK);
    GN_REQUIRE(Cout % 4 == 0, GOALNET_E_SHAPE, "conv3x3_fwd: Cout=%d must be a multiple of 4", Cout);
    GN_REQUIRE(aligned16(x) && aligned16(w) && aligned16(y) && aligned16(scale) && aligned16(shift),
               GOALNET_E_ALIGN, "conv3x3_fwd: pointers must be 16-byte aligned");
    const int64_t M = (int64_t)N * H * W;
    GN_REQUIRE(M < (1ll << 31) - 256, GOALNET_E_SHAPE, "conv3x3_fwd: N*H*W too large");
    hipStream_t st = (hipStream_t)stream;
    KCLoader<false>::P bp{w, (int64_t)9 * Cin, Cout, nullptr, nullptr, 1, Cin};
    const EpiP efinal = epi_act(y, Cout, (int)M, Cout, bias, relu);
    EpiP ep = efinal;
    const int ktiles = 9 * Cin / BK;
    // split K only when the caller supplied the workspace goalnet_conv3x3_fwd_ws_bytes asks for
    int nsplit = ws ? conv_splits_f32(M, Cin, Cout) : 1;
    if (nsplit > 1) {
        GN_REQUIRE(aligned16(ws) && ws_bytes >= goalnet_conv3x3_fwd_ws_bytes(N, H, W, Cin, Cout), GOALNET_E_WORKSPACE,
                   "conv3x3_fwd: workspace too small or misaligned");
        ep = epi_slabs((float*)ws, (int)M, Cout);
    }
    const bool narrow = Cout <= 64 && !getenv("GOALNET_F32_N64_OFF");       // 128 x 64 tile (conv2's data gradient: 256 -> 64 channels)
    // the caller lent zeroed ticket counters, one per output tile: the last block of each tile reduces (no second launch)
    const bool fused = nsplit > 1 && tile_ctr && (int64_t)n_ctr >= ((M + BM - 1) / BM) * ((Cout + (narrow ? 64 : BN) - 1) / (narrow ? 64 : BN));
    if (fused) {
        ep = efinal;
        ep.slabs = (float*)ws; ep.slab_stride = M * Cout; ep.tile_ctr = tile_ctr;
    }
    const bool strip = conv_strip_f32(W, nsplit, narrow, scale != nullptr);
    int rc;
    if (strip && scale) {
        ConvAStripLoader<true>::P ap{x, H, W, Cin, M, scale, shift};
        rc = launch_gemm<ConvAStripLoader<true>, KCLoader<false>>("conv3x3_fwd", ap, bp, ep, M, Cout, ktiles, 1, 0, st);
    } else if (strip) {
        ConvAStripLoader<false>::P ap{x, H, W, Cin, M, nullptr, nullptr};
        rc = launch_gemm<ConvAStripLoader<false>, KCLoader<false>>("conv3x3_fwd", ap, bp, ep, M, Cout, ktiles, 1, 0, st);
    } else if (scale) {
        ConvALoader<true>::P ap{x, H, W, Cin, M, scale, shift};
        rc = narrow ? launch_gemm<ConvALoader<true>, KCLoader<false>, true>("conv3x3_fwd", ap, bp, ep, M, Cout, ktiles, nsplit, 0, st)
                    : launch_gemm<ConvALoader<true>, KCLoader<false>>("conv3x3_fwd", ap, bp, ep, M, Cout, ktiles, nsplit, 0, st);
    } else {
        ConvALoader<false>::P ap{x, H, W, Cin, M, nullptr, nullptr};
        rc = narrow ? launch_gemm<ConvALoader<false>, KCLoader<false>, true>("conv3x3_fwd", ap, bp, ep, M, Cout, ktiles, nsplit, 0, st)
                    : launch_gemm<ConvALoader<false>, KCLoader<false>>("conv3x3_fwd", ap, bp, ep, M, Cout, ktiles, nsplit, 0, st);
    }
    if (rc || nsplit == 1 || fused) return rc;
    return launch_splitk_reduce("conv3x3_fwd.reduce", (const float*)ws, nsplit, M * Cout, efinal, st);
}

}  // extern "C"
namespace {
// the kernel template a launch_gemm<AL, BL> call instantiates, as the compiler spells its arguments
template <class AL, class BL, bool N64, int STAGES> const char* gemm_f32_kernel_name_() { return __PRETTY_FUNCTION__; }
// as launch_gemm dispatches: one LDS stage by the A loader's trait, GOALNET_F32_STAGES forces one form
template <class AL, class BL, bool N64> const char* gemm_f32_kernel_name() {
    const int force = getenv("GOALNET_F32_STAGES") ? atoi(getenv("GOALNET_F32_STAGES")) : 0;
    const bool one = AL::STRIP || force == 1 || (force != 2 && AL::ONE_STAGE);
    return one ? gemm_f32_kernel_name_<AL, BL, N64, 1>() : gemm_f32_kernel_name_<AL, BL, N64, 2>();
}
}
extern "C" {

/* which kernel goalnet_conv3x3_fwd launches for these dims (the dispatch above, not executed): bench.py names its roofline
 * kernel from this instead of a hard-coded string */
const char* goalnet_conv3x3_fwd_kernel_name(int N, int H, int W, int Cin, int Cout, int affine) {
    const bool narrow = Cout <= 64 && !getenv("GOALNET_F32_N64_OFF");       // as in goalnet_conv3x3_fwd
    const int nsplit = (N > 0 && H > 0 && W > 0 && Cin > 0 && Cout > 0) ? conv_splits_f32((int64_t)N * H * W, Cin, Cout) : 1;
    if (conv_strip_f32(W, nsplit, narrow, affine != 0))
        return affine ? gemm_f32_kernel_name<ConvAStripLoader<true>, KCLoader<false>, false>()
                      : gemm_f32_kernel_name<ConvAStripLoader<false>, KCLoader<false>, false>();
    if (affine) return narrow ? gemm_f32_kernel_name<ConvALoader<true>, KCLoader<false>, true>() : gemm_f32_kernel_name<ConvALoader<true>, KCLoader<false>, false>();
    return narrow ? gemm_f32_kernel_name<ConvALoader<false>, KCLoader<false>, true>() : gemm_f32_kernel_name<ConvALoader<false>, KCLoader<false>, false>();
}

static int wgrad_splits(int64_t M, int Cin, int Cout) {
    const int64_t tiles = (int64_t)((Cout + BM - 1) / BM) * ((9 * Cin + BN - 1) / BN);
    const int ktiles = (int)((M + BK - 1) / BK);
    static const int wtarget = getenv("GOALNET_WGRAD_SPLIT_TARGET") ? atoi(getenv("GOALNET_WGRAD_SPLIT_TARGET")) : 2048;      // A/B runs
    int64_t s = (wtarget + tiles - 1) / tiles;
    const int64_t smax = ktiles / 4 > 1 ? ktiles / 4 : 1;      // >= 4 K-tiles per split (small sub-batches: few pixels)
    if (s > smax) s = smax;
    if (s > 512) s = 512;
    if (s >= 8) {
        // whole XCD groups (launch_gemm's XCD-local order), and among the multiples of 8 between s and 2 s the one whose
        // tiles x splits fills the chip's 512 resident blocks (256 CUs x 2) in whole rounds: conv3's 72 tiles x 32 splits were
        // 4.5 rounds, i.e. a last round with half the chip idle (measured: MFMA busy 67 %); 72 x 64 are 9 full ones
        int64_t best = (s + 7) / 8 * 8 <= smax ? (s + 7) / 8 * 8 : s / 8 * 8;
        double best_eff = 0.0;
        for (int64_t c = best; c <= 2 * s + 8 && c <= smax && c <= 1024; c += 8) {
            const int64_t blocks = tiles * c, rounds = (blocks + 511) / 512;
            const double eff = (double)blocks / (double)(rounds * 512);
            if (eff > best_eff + 1e-9) { best_eff = eff; best = c; }
        }
        s = best;
    }
    const int kps = (int)((ktiles + s - 1) / s);
    return (ktiles + kps - 1) / kps;
}

static size_t wgrad_codes_bytes(int64_t M) { return (size_t)((M + 31) / 32 * 32 + 255) / 256 * 256; }
static size_t wgrad_border_bytes(int N, int Cout) {      // per-frame border sums (fp64) + U[Cout][9]
    return ((size_t)N * 8 * Cout * sizeof(double) + 255) / 256 * 256 + ((size_t)Cout * 9 * sizeof(float) + 255) / 256 * 256;
}

size_t goalnet_conv3x3_wgrad_ws_bytes(int N, int H, int W, int Cin, int Cout) {
    const int64_t M = (int64_t)N * H * W;
    return wgrad_codes_bytes(M) + wgrad_border_bytes(N, Cout) + (size_t)wgrad_splits(M, Cin, Cout) * (size_t)Cout * 9 * Cin * sizeof(float);
}

int goalnet_conv3x3_wgrad_codes(uint32_t* codes, int N, int H, int W, void* stream) {
    GN_REQUIRE(codes && N > 0 && H > 0 && W > 0, GOALNET_E_NULL, "conv3x3_wgrad_codes: bad arguments");
    const int64_t M = (int64_t)N * H * W;
    GN_REQUIRE(M < (1ll << 31) - 256, GOALNET_E_SHAPE, "conv3x3_wgrad_codes: N*H*W too large");
    const int Mpad = (int)((M + 31) / 32 * 32);
    int blocks = (Mpad / 4 + 255) / 256;
    if (blocks > 4096) blocks = 4096;
    hipLaunchKernelGGL(border_codes_kernel, dim3(blocks), dim3(256), 0, (hipStream_t)stream, codes, (int)M, Mpad, H, W);
    GN_LAUNCH_CHECK("conv3x3_wgrad_codes");
    return 0;
}

size_t goalnet_conv3x3_wgrad_codes_bytes(int N, int H, int W) { return wgrad_codes_bytes((int64_t)N * H * W); }

int goalnet_conv3x3_wgrad(const float* x, const float* scale, const float* shift, const float* dy, float* dw,
                          void* ws, size_t ws_bytes, const uint32_t* codes_in, int* tile_ctr, int n_ctr,
                          int N, int H, int W, int Cin, int Cout, void* stream) {
    GN_REQUIRE(x && dy && dw && ws, GOALNET_E_NULL, "conv3x3_wgrad: null pointer");
    GN_REQUIRE((scale == nullptr) == (shift == nullptr), GOALNET_E_NULL, "conv3x3_wgrad: scale/shift must both be set or both NULL");
    GN_REQUIRE(N > 0 && H > 0 && W > 0, GOALNET_E_SHAPE, "conv3x3_wgrad: non-positive dim");
    GN_REQUIRE(Cin % 4 == 0 && Cout % 4 == 0 && Cin > 0 && Cout > 0, GOALNET_E_SHAPE, "conv3x3_wgrad: channels must be multiples of 4");
    GN_REQUIRE(aligned16(x) && aligned16(dy) && aligned16(dw) && aligned16(ws) && aligned16(scale) && aligned16(shift),
               GOALNET_E_ALIGN, "conv3x3_wgrad: pointers must be 16-byte aligned");
    const int64_t M = (int64_t)N * H * W;
    GN_REQUIRE(M < (1ll << 31) - 256, GOALNET_E_SHAPE, "conv3x3_wgrad: N*H*W too large");
    GN_REQUIRE(ws_bytes >= goalnet_conv3x3_wgrad_ws_bytes(N, H, W, Cin, Cout), GOALNET_E_WORKSPACE, "conv3x3_wgrad: workspace too small");
    hipStream_t st = (hipStream_t)stream;
    const int nsplit = wgrad_splits(M, Cin, Cout);
    const int ktiles = (int)((M + BK - 1) / BK);
    const int64_t slab = (int64_t)Cout * 9 * Cin;
    uint32_t* codes = (uint32_t*)ws;
    double* bparts = (double*)((char*)ws + wgrad_codes_bytes(M));
    float* bu = (float*)((char*)bparts + ((size_t)N * 8 * Cout * sizeof(double) + 255) / 256 * 256);
    float* slabs = (float*)((char*)ws + wgrad_codes_bytes(M) + wgrad_border_bytes(N, Cout));
    // few frames: data select in the loop, no correction pass (GOALNET_WGRAD_PATH=select|correct forces one: tests, A/B runs)
    const char* force = getenv("GOALNET_WGRAD_PATH");
    const bool dsel = force && force[0] == 's' ? true : force && force[0] == 'c' ? false : (int64_t)N * (H > W ? H : W) <= 4096;
    if (codes_in) {
        codes = const_cast<uint32_t*>(codes_in);      // the caller's table (goalnet_conv3x3_wgrad_codes: depends on N, H, W only)
    } else {
        const int Mpad = (int)((M + 31) / 32 * 32);
        int blocks = (Mpad / 4 + 255) / 256;
        if (blocks > 4096) blocks = 4096;
        hipLaunchKernelGGL(border_codes_kernel, dim3(blocks), dim3(256), 0, st, codes, (int)M, Mpad, H, W);
        GN_LAUNCH_CHECK("conv3x3_wgrad.codes");
    }
    if (scale && !dsel) {
        hipLaunchKernelGGL(wgrad_border_sums_kernel, dim3(N), dim3(256), 0, st, dy, bparts, H, W, Cout);
        GN_LAUNCH_CHECK("conv3x3_wgrad.border_sums");
        hipLaunchKernelGGL(wgrad_border_u_kernel, dim3((Cout + 31) / 32), dim3(256), 0, st, bparts, N, Cout, bu);
        GN_LAUNCH_CHECK("conv3x3_wgrad.border_u");
    }
    MCLoader<false>::P ap{dy, Cout, Cout, (int)M, nullptr, nullptr, 1};
    EpiP ep = epi_slabs(slabs, Cout, 9 * Cin);
    // few frames (no rank-one correction to apply): with ticket counters lent by the caller the last block of each tile reduces
    const bool fused = nsplit > 1 && tile_ctr && (dsel || !scale) &&
                       (int64_t)n_ctr >= (int64_t)((Cout + BM - 1) / BM) * ((9 * Cin + BN - 1) / BN);
    if (fused) {
        ep = epi_raw(dw, (int64_t)9 * Cin, Cout, 9 * Cin);
        ep.slabs = slabs; ep.slab_stride = slab; ep.tile_ctr = tile_ctr;
    }
    int rc;
    if (scale && dsel) {
        ConvWgradBLoader<true, true>::P bp{x, H, W, Cin, (int)M, scale, shift, codes};
        rc = launch_gemm<MCLoader<false>, ConvWgradBLoader<true, true>>("conv3x3_wgrad", ap, bp, ep, Cout, 9 * Cin, ktiles, nsplit, 1, st);
    } else if (scale) {
        ConvWgradBLoader<true>::P bp{x, H, W, Cin, (int)M, scale, shift, codes};
        rc = launch_gemm<MCLoader<false>, ConvWgradBLoader<true>>("conv3x3_wgrad", ap, bp, ep, Cout, 9 * Cin, ktiles, nsplit, 1, st);
    } else {
        ConvWgradBLoader<false>::P bp{x, H, W, Cin, (int)M, nullptr, nullptr, codes};
        rc = launch_gemm<MCLoader<false>, ConvWgradBLoader<false>>("conv3x3_wgrad", ap, bp, ep, Cout, 9 * Cin, ktiles, nsplit, 1, st);
    }
    if (rc || fused) return rc;
    EpiP er = epi_raw(dw, (int64_t)9 * Cin, Cout, 9 * Cin);
    if (scale && !dsel) { er.corr_u = bu; er.corr_sh = shift; er.corr_C = Cin; }
    return launch_splitk_reduce("conv3x3_wgrad.reduce", slabs, nsplit, slab, er, st);
}

static int linear_splits(int M, int64_t K, int J) {
    const int64_t tiles = (int64_t)((M + BM - 1) / BM) * ((J + BN - 1) / BN);
    return pick_splits(tiles, (int)(K / BK));
}

size_t goalnet_linear_fwd_ws_bytes(int M, int64_t K, int J) {
    if (M <= 0 || K <= 0 || J <= 0) return 0;
    if (M <= SKINNY_MAX_M) return skinny_fwd_ws_bytes(M, K, J);
    const int s = linear_splits(M, K, J);
    return s > 1 ? (size_t)s * (size_t)M * (size_t)J * sizeof(float) : 0;
}

int goalnet_linear_fwd(const float* x, int64_t ldx, const float* scale, const float* shift, int bnC,
                       const float* w, const float* bias, int relu, const float* dropmask, int64_t ldmask,
                       float* y, int64_t ldy, float* mult_out, int64_t ldmult,
                       int M, int64_t K, int J, void* ws, size_t ws_bytes, void* stream) {
    GN_REQUIRE(x && w && y, GOALNET_E_NULL, "linear_fwd: null pointer");
    GN_REQUIRE((scale == nullptr) == (shift == nullptr), GOALNET_E_NULL, "linear_fwd: scale/shift must both be set or both NULL");
    GN_REQUIRE(M > 0 && J > 0 && K > 0 && K < (1ll << 31) - 64, GOALNET_E_SHAPE, "linear_fwd: bad dims");
    GN_REQUIRE(K % BK == 0, GOALNET_E_SHAPE, "linear_fwd: K=%lld must be a multiple of %d", (long long)K, BK);
    GN_REQUIRE(J % 4 == 0, GOALNET_E_SHAPE, "linear_fwd: J=%d must be a multiple of 4", J);
    GN_REQUIRE(!scale || (bnC > 0 && bnC % 4 == 0), GOALNET_E_SHAPE, "linear_fwd: bnC must be a positive multiple of 4");
    GN_REQUIRE(aligned16(x) && aligned16(w) && aligned16(y) && aligned16(scale) && aligned16(shift) && ldx % 4 == 0 && ldy % 4 == 0,
               GOALNET_E_ALIGN, "linear_fwd: pointers / leading dims must be 16-byte aligned");
    hipStream_t st = (hipStream_t)stream;
    const EpiP efinal = epi_act(y, ldy, M, J, bias, relu, dropmask, ldmask, mult_out, ldmult);
    if (M <= SKINNY_MAX_M) {          // the reference's 10-frame sub-batches: weight-streaming kernels (skinny.hip)
        const size_t need = skinny_fwd_ws_bytes(M, K, J);
        GN_REQUIRE(need == 0 || (ws && aligned16(ws) && ws_bytes >= need), GOALNET_E_WORKSPACE, "linear_fwd: workspace too small");
        return skinny_linear_fwd(x, ldx, scale, shift, bnC, w, efinal, M, K, J, ws, st);
    }
    const int nsplit = linear_splits(M, K, J);
    const int ktiles = (int)(K / BK);
    KCLoader<false>::P bp{w, K, J, nullptr, nullptr, 1, 0};
    EpiP ep = efinal;
    if (nsplit > 1) {
        GN_REQUIRE(ws && aligned16(ws), GOALNET_E_WORKSPACE, "linear_fwd: split-K needs a 16-byte aligned workspace");
        GN_REQUIRE(ws_bytes >= goalnet_linear_fwd_ws_bytes(M, K, J), GOALNET_E_WORKSPACE, "linear_fwd: workspace too small");
        ep = epi_slabs((float*)ws, M, J);
    }
    int rc;
    if (scale) {
        KCLoader<true>::P ap{x, ldx, M, scale, shift, bnC, 0};
        rc = launch_gemm<KCLoader<true>, KCLoader<false>>("linear_fwd", ap, bp, ep, M, J, ktiles, nsplit, 0, st);
    } else {
        KCLoader<false>::P ap{x, ldx, M, nullptr, nullptr, 1, 0};
        rc = launch_gemm<KCLoader<false>, KCLoader<false>>("linear_fwd", ap, bp, ep, M, J, ktiles, nsplit, 0, st);
    }
    if (rc || nsplit == 1) return rc;
    return launch_splitk_reduce("linear_fwd.reduce", (const float*)ws, nsplit, (int64_t)M * J, efinal, st);
}

int goalnet_linear_bwd_dx(const float* dy, int64_t lddy, const float* w, const float* mult, int64_t ldmult,
                          float* dx, int64_t lddx, int M, int64_t K, int J, void* stream) {
    GN_REQUIRE(dy && w && dx, GOALNET_E_NULL, "linear_bwd_dx: null pointer");
    GN_REQUIRE(M > 0 && J > 0 && K > 0 && K < (1ll << 31) - 256, GOALNET_E_SHAPE, "linear_bwd_dx: bad dims");
    GN_REQUIRE(J % BK == 0, GOALNET_E_SHAPE, "linear_bwd_dx: J=%d must be a multiple of %d", J, BK);
    GN_REQUIRE(K % 4 == 0, GOALNET_E_SHAPE, "linear_bwd_dx: K must be a multiple of 4");
    GN_REQUIRE(aligned16(dy) && aligned16(w) && aligned16(dx) && lddy % 4 == 0 && lddx % 4 == 0,
               GOALNET_E_ALIGN, "linear_bwd_dx: pointers / leading dims must be 16-byte aligned");
    hipStream_t st = (hipStream_t)stream;
    if (M <= SKINNY_MAX_M && (!mult || (aligned16(mult) && ldmult % 4 == 0)))
        return skinny_linear_dx(dy, lddy, w, mult, ldmult, dx, lddx, M, K, J, st);
    KCLoader<false>::P ap{dy, lddy, M, nullptr, nullptr, 1, 0};
    MCLoader<false>::P bp{w, K, (int)K, J, nullptr, nullptr, 1};
    const EpiP ep = epi_mul(dx, lddx, M, (int)K, mult, ldmult);
    return launch_gemm<KCLoader<false>, MCLoader<false>>("linear_bwd_dx", ap, bp, ep, M, K, J / BK, 1, 1, st);
}

int goalnet_linear_bwd_dw(const float* dy, int64_t lddy, const float* x, int64_t ldx,
                          const float* scale, const float* shift, int bnC,
                          float* dw, float* db, int M, int64_t K, int J, void* stream) {
    GN_REQUIRE(dy && x && dw, GOALNET_E_NULL, "linear_bwd_dw: null pointer");
    GN_REQUIRE((scale == nullptr) == (shift == nullptr), GOALNET_E_NULL, "linear_bwd_dw: scale/shift must both be set or both NULL");
    GN_REQUIRE(M > 0 && J > 0 && K > 0 && K < (1ll << 31) - 256, GOALNET_E_SHAPE, "linear_bwd_dw: bad dims");
    GN_REQUIRE(J % 4 == 0 && K % 4 == 0, GOALNET_E_SHAPE, "linear_bwd_dw: J and K must be multiples of 4");
    GN_REQUIRE(!scale || (bnC > 0 && bnC % 4 == 0), GOALNET_E_SHAPE, "linear_bwd_dw: bnC must be a positive multiple of 4");
    GN_REQUIRE(aligned16(dy) && aligned16(x) && aligned16(dw) && aligned16(scale) && aligned16(shift) && lddy % 4 == 0 && ldx % 4 == 0,
               GOALNET_E_ALIGN, "linear_bwd_dw: pointers / leading dims must be 16-byte aligned");
    hipStream_t st = (hipStream_t)stream;
    if (M <= SKINNY_MAX_M) return skinny_linear_dw(dy, lddy, x, ldx, scale, shift, bnC, dw, db, M, K, J, st);
    if (db) { const int rc = goalnet_colsum(dy, lddy, M, J, db, stream); if (rc) return rc; }
    const int ktiles = (M + BK - 1) / BK;
    MCLoader<false>::P ap{dy, lddy, J, M, nullptr, nullptr, 1};
    const EpiP ep = epi_raw(dw, K, J, (int)K);
    if (scale) {
        MCLoader<true>::P bp{x, ldx, (int)K, M, scale, shift, bnC};
        return launch_gemm<MCLoader<false>, MCLoader<true>>("linear_bwd_dw", ap, bp, ep, J, K, ktiles, 1, 1, st);
    }
    MCLoader<false>::P bp{x, ldx, (int)K, M, nullptr, nullptr, 1};
    return launch_gemm<MCLoader<false>, MCLoader<false>>("linear_bwd_dw", ap, bp, ep, J, K, ktiles, 1, 1, st);
}

/* goalnet_linear_bwd_dw followed by goalnet_adam_step_dev on p / m / v [J][K] (1-based step count *step + step_bias), in one
 * launch and with the same bits: the Adam update runs in the GEMM's epilogue on the accumulators, the gradient is never
 * written (EPIK_ADAM). Served by the 128 x 128 tile only: M <= SKINNY_MAX_M is refused (the caller keeps the two launches). */
int goalnet_linear_bwd_dw_adam(const float* dy, int64_t lddy, const float* x, int64_t ldx,
                               const float* scale, const float* shift, int bnC,
                               float* p, float* m, float* v, float* db, int M, int64_t K, int J,
                               double lr, double beta1, double beta2, double eps, const int64_t* step, int64_t step_bias,
                               float grad_scale, void* stream) {
    GN_REQUIRE(dy && x && p && m && v && step, GOALNET_E_NULL, "linear_bwd_dw_adam: null pointer");
    GN_REQUIRE((scale == nullptr) == (shift == nullptr), GOALNET_E_NULL, "linear_bwd_dw_adam: scale/shift must both be set or both NULL");
    GN_REQUIRE(M > 0 && J > 0 && K > 0 && K < (1ll << 31) - 256, GOALNET_E_SHAPE, "linear_bwd_dw_adam: bad dims");
    GN_REQUIRE(J % 4 == 0 && K % 4 == 0, GOALNET_E_SHAPE, "linear_bwd_dw_adam: J and K must be multiples of 4");
    GN_REQUIRE(!scale || (bnC > 0 && bnC % 4 == 0), GOALNET_E_SHAPE, "linear_bwd_dw_adam: bnC must be a positive multiple of 4");
    GN_REQUIRE(M > SKINNY_MAX_M, GOALNET_E_SHAPE, "linear_bwd_dw_adam: M=%d is served by the weight-streaming kernels (M > %d here)", M, SKINNY_MAX_M);
    GN_REQUIRE(aligned16(dy) && aligned16(x) && aligned16(scale) && aligned16(shift) && lddy % 4 == 0 && ldx % 4 == 0,
               GOALNET_E_ALIGN, "linear_bwd_dw_adam: pointers / leading dims must be 16-byte aligned");
    GN_REQUIRE(aligned16(p) && aligned16(m) && aligned16(v), GOALNET_E_ALIGN, "linear_bwd_dw_adam: p, m and v must be 16-byte aligned");
    hipStream_t st = (hipStream_t)stream;
    if (db) { const int rc = goalnet_colsum(dy, lddy, M, J, db, stream); if (rc) return rc; }
    const int ktiles = (M + BK - 1) / BK;
    MCLoader<false>::P ap{dy, lddy, J, M, nullptr, nullptr, 1};
    const AdamEpi ae{p, m, v, lr, beta1, beta2, (float)eps, grad_scale, step, step_bias};
    if (scale) {
        MCLoader<true>::P bp{x, ldx, (int)K, M, scale, shift, bnC};
        return launch_gemm_epi<MCLoader<false>, MCLoader<true>, EPIK_ADAM>("linear_bwd_dw_adam", ap, bp, ae, J, K, K, ktiles, 1, st);
    }
    MCLoader<false>::P bp{x, ldx, (int)K, M, nullptr, nullptr, 1};
    return launch_gemm_epi<MCLoader<false>, MCLoader<false>, EPIK_ADAM>("linear_bwd_dw_adam", ap, bp, ae, J, K, K, ktiles, 1, st);
}

}  // extern "C"
