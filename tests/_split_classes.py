"""Split-K and tile-order classes of the fp32 GEMM engine (csrc/gemm_f32.hip, csrc/gemm_common.h), restated in plain Python, and the parameter
tables of tests/test_gpu_split_classes.py. No torch, no GPU: tests/test_split_classes_host.py holds the rules against the library's own
*_ws_bytes entry points, the block decoding against "every (tile, split) exactly once", and the tables against the rules.

Which block computes which (output tile, K-split) pair and which kernel sums the slabs is integer arithmetic on the shape. A class that no
test's shape selects is code that has never run below a whole training step; a table row here is what selects it. Defaults only: the
GOALNET_SPLIT_TARGET, GOALNET_SPLIT_MINKT and GOALNET_WGRAD_SPLIT_TARGET switches are read once per process, so no test sets them."""

BM = BN = 128             # csrc/gemm_f32.hip: output tile (the 128 x 64 tile where Cout <= 64: N64)
BK = 32                   # K-tile
SKINNY_MAX_M = 16         # csrc/skinny.h: up to 16 rows the linear layers take the weight-streaming kernels (tests/_bin_classes.py)


def cdiv(a, b):
    return -(-a // b)


# ---- csrc/gemm_common.h, conv_fwd_splits: ~512 blocks, >= 4 K-tiles per split ---------------------------------------------------------
def conv_fwd_splits(tiles, ktiles):
    if tiles >= 256 or ktiles < 8:
        return 1
    s = min(cdiv(512, tiles), ktiles // 4)
    s = max(s, 1)
    kps = cdiv(ktiles, s)
    return cdiv(ktiles, kps)                               # no empty splits


# ---- csrc/gemm_f32.hip, pick_splits: ~1024 blocks of >= 8 K-tiles; below 64 K-tiles ~256 blocks of >= 4 ----------------------------------
def pick_splits(tiles, ktiles):
    if ktiles < 8 or (ktiles < 64 and tiles >= 128):
        return 1
    s = cdiv(256 if ktiles < 64 else 1024, tiles)
    smax = ktiles // 4 if ktiles < 64 else max(ktiles // 8, 1)
    s = max(min(s, smax), 1)
    kps = cdiv(ktiles, s)
    return cdiv(ktiles, kps)


# ---- csrc/gemm_f32.hip, wgrad_splits: ~2048 blocks of >= 4 K-tiles, at most 512 splits; from 8 splits on whole groups of 8 and, among the
# multiples of 8 in [s, 2 s + 8], the first that fills the 512 resident blocks best -------------------------------------------------------
def wgrad_splits_of(tiles, ktiles):
    s = cdiv(2048, tiles)
    smax = max(ktiles // 4, 1)
    s = min(s, smax, 512)
    if s >= 8:
        best = cdiv(s, 8) * 8 if cdiv(s, 8) * 8 <= smax else s // 8 * 8
        best_eff = 0.0
        c = best
        while c <= 2 * s + 8 and c <= smax and c <= 1024:
            blocks = tiles * c
            eff = blocks / (cdiv(blocks, 512) * 512)
            if eff > best_eff + 1e-9:
                best_eff, best = eff, c
            c += 8
        s = best
    kps = cdiv(ktiles, s)
    return cdiv(ktiles, kps)


def wgrad_splits(m, cin, cout):
    return wgrad_splits_of(cdiv(cout, BM) * cdiv(9 * cin, BN), cdiv(m, BK))


# ---- the three roles: (output tiles the launch walks, split count) ----------------------------------------------------------------------
ROLES = ("conv_fwd", "wgrad", "linear_fwd")


def conv_fwd_plan(n, h, w, cin, cout):
    """goalnet_conv3x3_fwd with a workspace (forward, and the data gradient on flipped weights). conv_splits_f32 counts 128-wide tiles;
    launch_gemm<.., N64> walks 64-wide ones where Cout <= 64 (`narrow`): one column of tiles either way, so the counts agree."""
    m = n * h * w
    tiles = cdiv(m, BM) * cdiv(cout, 64 if cout <= 64 else BN)
    assert tiles == cdiv(m, BM) * cdiv(cout, BN)
    return tiles, conv_fwd_splits(tiles, 9 * cin // BK)


def wgrad_plan(n, h, w, cin, cout):
    """goalnet_conv3x3_wgrad: dW[Cout][9 Cin], reduced over the N H W pixels"""
    return cdiv(cout, BM) * cdiv(9 * cin, BN), wgrad_splits(n * h * w, cin, cout)


def linear_plan(m, k, j):
    """goalnet_linear_fwd above SKINNY_MAX_M rows (linear_splits)"""
    assert m > SKINNY_MAX_M
    tiles = cdiv(m, BM) * cdiv(j, BN)
    return tiles, pick_splits(tiles, k // BK)


PLAN = {"conv_fwd": conv_fwd_plan, "wgrad": wgrad_plan, "linear_fwd": linear_plan}


# ---- csrc/gemm_f32.hip, launch_gemm: `xcd_local = nsplit >= 8 && tiles <= 256` (the 2^31 clause needs 2^23 tiles); gemm_f32_kernel: the
# `tiles > 64 && tiles <= 128` two-phase branch inside `xcd_splits > 0` ---------------------------------------------------------------------
def order_class(tiles, nsplit):
    """("one",) | ("grid.y", "few" | "many") | ("xcd-plain" | "two-phase", "lo" | "mid" | "hi", "one-group" | "groups", "whole" | "padded").
    grid.y: splits on blockIdx.y, tiles through xcd_remap; "many" is 8 or more splits above 256 tiles. XCD-local: "lo" tiles <= 64,
    "mid" 65 .. 128 (two-phase), "hi" 129 .. 256; one group of 8 splits or several; the grid padded to whole groups or not."""
    if nsplit == 1:
        return ("one",)
    if nsplit < 8 or tiles > 256:
        return ("grid.y", "few" if nsplit < 8 else "many")
    band = "lo" if tiles <= 64 else "mid" if tiles <= 128 else "hi"
    return ("two-phase" if band == "mid" else "xcd-plain", band, "one-group" if nsplit <= 8 else "groups", "padded" if nsplit % 8 else "whole")


XCD_CLASSES = tuple((("two-phase" if band == "mid" else "xcd-plain"), band, g, p)
                    for band in ("lo", "mid", "hi") for g, p in (("one-group", "whole"), ("groups", "whole"), ("groups", "padded")))
ORDER_CLASSES = (("one",), ("grid.y", "few"), ("grid.y", "many")) + XCD_CLASSES
# one group is 8 splits exactly (XCD-local starts at 8), so a padded one-group grid does not exist
ORDER_IMPOSSIBLE = tuple((("two-phase" if band == "mid" else "xcd-plain"), band, "one-group", "padded") for band in ("lo", "mid", "hi"))


def grid_blocks(tiles, nsplit):
    """launch_gemm: blocks of the 1-D XCD-local grid"""
    return tiles * cdiv(nsplit, 8) * 8


def block_to_tile_split(block, tiles, nsplit):
    """gemm_f32_kernel, `if (xcd_splits > 0)`: (tile, split) of a block of the XCD-local grid; the kernel returns where split >= nsplit (the
    padding of the last group). `block` is an int or a numpy array of ints: the select between the two phases is arithmetic."""
    xcd, j = block & 7, block >> 3
    if 64 < tiles <= 128:
        gs, rest = cdiv(nsplit, 8), tiles - 64
        n_a = gs * 64
        first = (j < n_a) * 1                               # phase one: per split, the 64 tiles that fill the XCD
        i = j - n_a
        qb = i // rest
        q = first * (j >> 6) + (1 - first) * qb
        t = first * (j & 63) + (1 - first) * (64 + (i - qb * rest))
        split = q * 8 + xcd
    else:
        split = (j // tiles) * 8 + xcd
        t = j - (j // tiles) * tiles
    return t, split


def xcd_remap(bid, nwg):
    """csrc/common.h xcd_remap: the tile of blockIdx.x in the grid.y order (tile_of_block)"""
    q, r = nwg >> 3, nwg & 7
    xcd, slot = bid & 7, bid >> 3
    base = xcd * (q + 1) if xcd < r else r * (q + 1) + (xcd - r) * q
    return base + slot


# ---- csrc/gemm_f32.hip, launch_splitk_reduce --------------------------------------------------------------------------------------------
REDUCE_GRID = 4096


def reduce_class(outputs4, nsplit):
    """outputs4 = rows * cols / 4 float4 outputs. "wide": splitk_reduce_wide_kernel (16 lanes per output); "plain": splitk_reduce_kernel, one
    output per thread; "plain-loop": more than 4 096 blocks of 256, the stride loop runs again"""
    if outputs4 < 65536 and nsplit >= 32:
        return "wide"
    return "plain-loop" if cdiv(outputs4, 256) > REDUCE_GRID else "plain"


REDUCE_CLASSES = ("wide", "plain", "plain-loop")


def reduce_of(role, dims):
    """reduce_class of a row (None without a split: conv / linear forward store through their epilogue; the weight gradient always reduces)"""
    tiles, nsplit = PLAN[role](*dims)
    if role == "wgrad":
        n, h, w, cin, cout = dims
        return reduce_class(cout * 9 * cin // 4, nsplit)
    if nsplit == 1:
        return None
    rows, cols = (dims[0] * dims[1] * dims[2], dims[4]) if role == "conv_fwd" else (dims[0], dims[2])
    return reduce_class(rows * cols // 4, nsplit)


# ---- csrc/gemm_f32.hip, goalnet_conv3x3_wgrad: `dsel`, and the layout of its workspace -----------------------------------------------------
def wgrad_path(n, h, w):
    """few frames: the padding taps are zeroed in the loop ("select"); else they load zeros and the BatchNorm shift they picked up is
    subtracted in the slab reduction ("correct")"""
    return "select" if n * max(h, w) <= 4096 else "correct"


def _up256(b):
    return cdiv(b, 256) * 256


def wgrad_ws_fixed_bytes(n, h, w, cout):
    """wgrad_codes_bytes + wgrad_border_bytes: what goalnet_conv3x3_wgrad_ws_bytes holds in front of the slabs"""
    m = n * h * w
    codes = _up256(cdiv(m, 32) * 32)
    border = _up256(n * 8 * cout * 8) + _up256(cout * 9 * 4)
    return codes + border


# ======================================================================================================================================
# tables of tests/test_gpu_split_classes.py; tests/test_split_classes_host.py states the tiles, splits and classes of every row
# ======================================================================================================================================
# (n, h, w, cin, cout, affine, bias, relu) of goalnet_conv3x3_fwd: the forward with BatchNorm on the load, bias and ReLU, and the data-gradient
# form on flipped weights (no affine, no bias). Every row also runs with ws = NULL, which is the role's ("one",) class.
CONV_FWD_ROWS = (
    (17, 11, 11, 256, 512, True, True, True),        # 68 tiles, 8 splits: two-phase; 17 .. 19 frames of 40 x 40 select it on conv3
    (34, 11, 11, 512, 256, False, False, False),     # 66 tiles: two-phase, the data gradient
    (33, 11, 11, 512, 256, False, False, False),     # 64 tiles: the neighbour across 64 | 65
    (147, 4, 4, 256, 512, True, True, True),         # 76 tiles, 7 splits on grid.y: the other side of 7 | 8
    (10, 11, 11, 512, 256, False, False, False),     # 20 tiles, 24 splits: three whole groups
    (4, 11, 11, 256, 512, True, True, True),         # 16 tiles, 18 splits: three groups, padded grid
    (2, 13, 13, 256, 64, False, False, False),       # the 128 x 64 tile (conv2's data gradient): 3 tiles, 18 splits
    (520, 4, 4, 128, 128, True, True, True),         # 65 tiles exactly: the second phase holds one tile per split (`rest` = 1)
)
CONV_FWD_CTR = CONV_FWD_ROWS[0]        # the two-phase forward row that also runs with ticket counters

# (n, h, w, cin, cout, affine) of goalnet_conv3x3_wgrad, each under GOALNET_WGRAD_PATH = select, correct and unset
WGRAD_TWO_PHASE = (
    (17, 11, 11, 256, 512, True),     # 72 tiles, 13 splits: two groups, padded grid; the 17-frame step at 40 x 40
    (128, 4, 4, 256, 512, True),      # 16 splits: two whole groups
    (256, 4, 4, 256, 512, True),      # 32 splits: four groups
    (63, 4, 4, 256, 512, True),       # 8 splits: one group
)
WGRAD_ABI_ONLY = (                    # channel counts the header permits and no model here uses
    (64, 4, 4, 512, 512, True),       # 144 tiles: XCD-plain above 128, one group
    (128, 4, 4, 512, 512, True),      # the same order, two groups
    (129, 4, 4, 512, 512, True),      # 13 splits: padded grid
    (64, 4, 4, 1024, 512, True),      # 288 tiles: grid.y with 8 splits; 1.18 M float4 outputs, the reduce on its capped grid
)
WGRAD_RAGGED = (                      # 9 Cin = 324 columns in 128-wide tiles, Cout below one tile
    (3, 5, 4, 36, 60, True),          # no split
    (127, 4, 4, 36, 60, True),        # 3 tiles, 16 splits
    (129, 4, 4, 36, 60, False),       # 13 splits, no affine
)
WGRAD_FEW = (
    (15, 4, 4, 64, 256, True),        # conv2's 10 tiles, 2 splits on grid.y
    (63, 4, 4, 64, 256, True),        # 8 splits: one group
)
WGRAD_ROWS = WGRAD_TWO_PHASE + WGRAD_ABI_ONLY + WGRAD_RAGGED + WGRAD_FEW
WGRAD_CTR = WGRAD_TWO_PHASE            # on the select path these also run with ticket counters
# unforced only, and bit-equal to the forced form of the path wgrad_path names: N max(H, W) = 4 096 and 4 100. 3 tiles, 96 and 77 splits:
# the wide reduce kernel
WGRAD_THRESHOLD = ((1024, 4, 3, 32, 128, True), (1025, 4, 3, 32, 128, True))

# (m, k, j, affine, mask, ldextra) of goalnet_linear_fwd, with the saved multiplier, into a column slice where ldextra > 0
LINEAR_ROWS = (
    (2176, 2048, 512, False, True, 128),     # 68 tiles, 8 splits: two-phase, one group
    (2176, 4096, 512, True, True, 128),      # 16 splits: two-phase, two groups
    (2500, 3328, 512, False, True, 0),       # 80 tiles, 13 splits: two-phase, padded grid
    (4096, 2048, 512, False, True, 0),       # 128 tiles exactly, 8 splits: the widest two-phase grid (`rest` = 64)
    (17, 2048, 128, False, True, 0),         # one tile, 8 splits
    (100, 4096, 128, True, True, 128),       # one tile, 16 splits
    (100, 1152, 128, False, False, 0),       # one tile, 9 splits: padded grid
    (5400, 2048, 260, False, True, 0),       # 129 tiles (43 x 3, the last column 4 wide), 8 splits: XCD-plain above 128
    (37, 640, 512, False, True, 0),          # 4 tiles, 5 splits on grid.y
    (130, 224, 132, False, False, 128),      # 7 K-tiles: no split
)

ROWS = {"conv_fwd": tuple(r[:5] for r in CONV_FWD_ROWS), "wgrad": tuple(r[:5] for r in WGRAD_ROWS + WGRAD_THRESHOLD),
        "linear_fwd": tuple(r[:3] for r in LINEAR_ROWS)}

# ---- rows of tests/test_gpu_ops.py from before these tables: (n, h, w, cin, cout) of test_conv3x3_fwd and test_conv3x3_wgrad, (m, k, j) of
# test_linear_fwd above SKINNY_MAX_M rows ---------------------------------------------------------------------------------------------------
OPS_CONV_FWD = ((2, 7, 5, 64, 256), (3, 13, 13, 64, 256), (2, 11, 11, 256, 512), (2, 11, 11, 512, 256), (2, 13, 13, 256, 64), (16, 11, 11, 512, 256),
                (16, 11, 11, 256, 512), (1, 3, 3, 64, 128), (40, 26, 22, 256, 64), (3, 9, 7, 64, 32), (2, 5, 5, 128, 60))
OPS_WGRAD = ((2, 7, 5, 64, 256), (3, 13, 13, 64, 256), (2, 11, 11, 256, 512), (5, 9, 6, 64, 128), (16, 11, 11, 256, 512), (16, 13, 13, 64, 256),
             (40, 13, 13, 64, 256), (2, 1, 9, 64, 128), (3, 4, 1, 64, 128), (1, 1, 1, 64, 128))
OPS_LINEAR_FWD = ((37, 640, 512), (130, 512, 256), (17, 41472, 512))
