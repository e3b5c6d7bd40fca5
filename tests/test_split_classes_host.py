"""CPU: the split-K and tile-order rules of the fp32 GEMM engine restated in tests/_split_classes.py, against the library (the *_ws_bytes entry
points need no GPU), against "every (tile, split) exactly once", and against the tables of tests/test_gpu_split_classes.py: every class that
a shape can reach is reached by a row, on both sides of every boundary, and a row that is the only cover of a class cannot be removed
without an assertion here failing. A class that no shape reaches has its reason stated as an assertion."""
import numpy as np
import pytest

import _split_classes as S
from cvml_goalnet_amd import _lib

ONE = ("one",)
FEW, MANY = ("grid.y", "few"), ("grid.y", "many")
LO1, LOG, LOP = ("xcd-plain", "lo", "one-group", "whole"), ("xcd-plain", "lo", "groups", "whole"), ("xcd-plain", "lo", "groups", "padded")
MID1, MIDG, MIDP = ("two-phase", "mid", "one-group", "whole"), ("two-phase", "mid", "groups", "whole"), ("two-phase", "mid", "groups", "padded")
HI1, HIG, HIP = ("xcd-plain", "hi", "one-group", "whole"), ("xcd-plain", "hi", "groups", "whole"), ("xcd-plain", "hi", "groups", "padded")

# dims of a row -> (tiles, splits, order class, reduce class)
EXPECT = {
    "conv_fwd": {
        (17, 11, 11, 256, 512): (68, 8, MID1, "plain"),
        (34, 11, 11, 512, 256): (66, 8, MID1, "plain"),
        (33, 11, 11, 512, 256): (64, 8, LO1, "plain"),
        (147, 4, 4, 256, 512): (76, 7, FEW, "plain"),
        (10, 11, 11, 512, 256): (20, 24, LOG, "plain"),
        (4, 11, 11, 256, 512): (16, 18, LOP, "plain"),
        (2, 13, 13, 256, 64): (3, 18, LOP, "plain"),
        (520, 4, 4, 128, 128): (65, 8, MID1, "plain"),
    },
    "wgrad": {
        (17, 11, 11, 256, 512): (72, 13, MIDP, "plain"),
        (128, 4, 4, 256, 512): (72, 16, MIDG, "plain"),
        (256, 4, 4, 256, 512): (72, 32, MIDG, "plain"),
        (63, 4, 4, 256, 512): (72, 8, MID1, "plain"),
        (64, 4, 4, 512, 512): (144, 8, HI1, "plain"),
        (128, 4, 4, 512, 512): (144, 16, HIG, "plain"),
        (129, 4, 4, 512, 512): (144, 13, HIP, "plain"),
        (64, 4, 4, 1024, 512): (288, 8, MANY, "plain-loop"),
        (3, 5, 4, 36, 60): (3, 1, ONE, "plain"),
        (127, 4, 4, 36, 60): (3, 16, LOG, "plain"),
        (129, 4, 4, 36, 60): (3, 13, LOP, "plain"),
        (15, 4, 4, 64, 256): (10, 2, FEW, "plain"),
        (63, 4, 4, 64, 256): (10, 8, LO1, "plain"),
        (1024, 4, 3, 32, 128): (3, 96, LOG, "wide"),
        (1025, 4, 3, 32, 128): (3, 77, LOP, "wide"),
    },
    "linear_fwd": {
        (2176, 2048, 512): (68, 8, MID1, "plain"),
        (2176, 4096, 512): (68, 16, MIDG, "plain"),
        (2500, 3328, 512): (80, 13, MIDP, "plain"),
        (4096, 2048, 512): (128, 8, MID1, "plain"),
        (17, 2048, 128): (1, 8, LO1, "plain"),
        (100, 4096, 128): (1, 16, LOG, "plain"),
        (100, 1152, 128): (1, 9, LOP, "plain"),
        (5400, 2048, 260): (129, 8, HI1, "plain"),
        (37, 640, 512): (4, 5, FEW, "plain"),
        (130, 224, 132): (4, 1, ONE, None),
    },
}
# what a shape of each role can reach (test_reachable_classes_are_these derives it from the rules)
REACHABLE = {
    "conv_fwd": {ONE, FEW, LO1, LOG, LOP, MID1},
    "linear_fwd": {ONE, FEW, LO1, LOG, LOP, MID1, MIDG, MIDP, HI1},
    "wgrad": {ONE, FEW, MANY, LO1, LOG, LOP, MID1, MIDG, MIDP, HI1, HIG, HIP},
}


def _row_class(role, dims):
    tiles, nsplit = S.PLAN[role](*dims)
    return tiles, nsplit, S.order_class(tiles, nsplit), S.reduce_of(role, dims)


# ---- mirror equals the library --------------------------------------------------------------------------------------------------------
def _lib_conv_fwd_splits(lib, n, h, w, cin, cout):
    b = lib.goalnet_conv3x3_fwd_ws_bytes(n, h, w, cin, cout)
    assert b % (4 * n * h * w * cout) == 0
    return b // (4 * n * h * w * cout) if b else 1            # 0 bytes: no split


def _lib_wgrad_splits(lib, n, h, w, cin, cout):
    b = lib.goalnet_conv3x3_wgrad_ws_bytes(n, h, w, cin, cout) - S.wgrad_ws_fixed_bytes(n, h, w, cout)
    assert b > 0 and b % (4 * cout * 9 * cin) == 0
    return b // (4 * cout * 9 * cin)


def _lib_linear_splits(lib, m, k, j):
    b = lib.goalnet_linear_fwd_ws_bytes(m, k, j)
    assert b % (4 * m * j) == 0
    return b // (4 * m * j) if b else 1


LIB_SPLITS = {"conv_fwd": _lib_conv_fwd_splits, "wgrad": _lib_wgrad_splits, "linear_fwd": _lib_linear_splits}


def test_every_table_row_has_the_split_count_the_library_gives():
    lib = _lib.load()
    for role in S.ROLES:
        for dims in S.ROWS[role] + {"conv_fwd": S.OPS_CONV_FWD, "wgrad": S.OPS_WGRAD, "linear_fwd": S.OPS_LINEAR_FWD}[role]:
            assert LIB_SPLITS[role](lib, *dims) == S.PLAN[role](*dims)[1], (role, dims)


@pytest.mark.parametrize("hw", [11, 13, 72, 74])
def test_split_rules_equal_the_library_over_a_sweep_of_frame_counts(hw):
    """conv3 and conv2 geometry, forward, data gradient and weight gradient, at the conv-output sizes of 40 x 40 and 224 x 224 frames"""
    lib = _lib.load()
    for cin, cout in ((256, 512), (512, 256), (64, 256), (256, 64)):
        for n in list(range(1, 301)) + [1024]:
            dims = (n, hw, hw, cin, cout)
            assert _lib_conv_fwd_splits(lib, *dims) == S.conv_fwd_plan(*dims)[1], ("conv_fwd", dims)
            assert _lib_wgrad_splits(lib, *dims) == S.wgrad_plan(*dims)[1], ("wgrad", dims)


def test_linear_split_rule_equals_the_library_over_a_sweep():
    lib = _lib.load()
    for m in list(range(17, 400, 3)) + [1024, 2049, 2176, 4096, 4097, 10000, 18000, 40000]:
        for k in (224, 256, 512, 640, 1152, 2016, 2048, 3328, 4096, 41472):
            for j in (4, 128, 132, 260, 512):
                assert _lib_linear_splits(lib, m, k, j) == S.linear_plan(m, k, j)[1], (m, k, j)
    # up to 16 rows the weight-streaming kernels serve the call: their workspace is tests/_bin_classes.py's subject
    assert S.SKINNY_MAX_M == 16


# ---- the block decoding is a bijection ------------------------------------------------------------------------------------------------
def _decoded(tiles, nsplit):
    """sorted tile * nsplit + split of the blocks that compute, and the number of padding blocks"""
    blocks = np.arange(S.grid_blocks(tiles, nsplit), dtype=np.int64)
    t, split = S.block_to_tile_split(blocks, tiles, nsplit)
    live = split < nsplit
    assert (t >= 0).all() and (t < tiles).all() and (split >= 0).all()
    return np.sort(t[live] * nsplit + split[live]), int((~live).sum())


def test_every_tile_and_split_is_computed_exactly_once():
    pairs = [(t, s) for t in range(1, 257) for s in range(8, 81)]
    pairs += [(tiles, nsplit) for role in S.ROLES for tiles, nsplit, cls, _ in EXPECT[role].values() if cls[0] in ("xcd-plain", "two-phase")]
    for tiles, nsplit in pairs:
        assert S.grid_blocks(tiles, nsplit) == tiles * 8 * S.cdiv(nsplit, 8)
        keys, padding = _decoded(tiles, nsplit)
        assert np.array_equal(keys, np.arange(tiles * nsplit)), (tiles, nsplit)
        assert padding == tiles * (8 * S.cdiv(nsplit, 8) - nsplit)
    # blocks b, b + 8, ... share an XCD: a split stays on XCD split % 8, which is what makes the order XCD-local
    for tiles, nsplit in ((72, 13), (144, 16), (3, 96), (65, 8), (128, 8)):
        blocks = np.arange(S.grid_blocks(tiles, nsplit), dtype=np.int64)
        _, split = S.block_to_tile_split(blocks, tiles, nsplit)
        assert ((split & 7) == (blocks & 7)).all()


def test_the_scalar_and_the_array_decoding_agree():
    for tiles, nsplit in ((72, 13), (65, 8), (128, 16), (64, 8), (129, 9), (3, 77)):
        blocks = np.arange(S.grid_blocks(tiles, nsplit), dtype=np.int64)
        t, split = S.block_to_tile_split(blocks, tiles, nsplit)
        for b in range(0, len(blocks), 7):
            assert S.block_to_tile_split(b, tiles, nsplit) == (t[b], split[b])


def test_two_phase_order_runs_64_tiles_of_one_split_then_the_rest_of_all():
    """72 tiles, 13 splits (two groups, three padding splits): XCD 2 walks tiles 0 .. 63 of split 2, then of split 10, then tiles 64 .. 71
    of split 2 and of split 10; XCD 7's second split (15) does not exist"""
    seq = [S.block_to_tile_split(8 * j + 2, 72, 13) for j in range(2 * 72)]
    assert seq == ([(t, 2) for t in range(64)] + [(t, 10) for t in range(64)] + [(t, 2) for t in range(64, 72)] + [(t, 10) for t in range(64, 72)])
    seq7 = [S.block_to_tile_split(8 * j + 7, 72, 13) for j in range(2 * 72)]
    assert [p for p in seq7 if p[1] < 13] == [(t, 7) for t in range(72)] and {p[1] for p in seq7} == {7, 15}
    # the band's edges, 16 splits: at 65 tiles XCD 0's 65th block starts split 8, at 64 and at 129 tiles the splits follow each other whole
    assert [S.block_to_tile_split(8 * j, 65, 16) for j in (63, 64, 128, 129)] == [(63, 0), (0, 8), (64, 0), (64, 8)]
    assert [S.block_to_tile_split(8 * j, 64, 16) for j in (63, 64)] == [(63, 0), (0, 8)]
    assert [S.block_to_tile_split(8 * j, 128, 16) for j in (64, 128, 192)] == [(0, 8), (64, 0), (64, 8)]
    assert [S.block_to_tile_split(8 * j, 129, 16) for j in (64, 128, 129)] == [(64, 0), (128, 0), (0, 8)]


def test_grid_y_order_visits_every_tile_once():
    for nwg in list(range(1, 300)) + [1007, 4096]:
        assert sorted(S.xcd_remap(b, nwg) for b in range(nwg)) == list(range(nwg))


# ---- coverage -------------------------------------------------------------------------------------------------------------------------
def test_rows_have_the_classes_stated_here():
    for role in S.ROLES:
        assert {d: _row_class(role, d) for d in S.ROWS[role]} == EXPECT[role]
    assert set(S.ORDER_CLASSES) == {ONE, FEW, MANY, LO1, LOG, LOP, MID1, MIDG, MIDP, HI1, HIG, HIP}


def test_reachable_classes_are_these():
    """the split rules over every tile count up to 400 and every reduction length a layer could have"""
    got = {r: set() for r in S.ROLES}
    kts = list(range(1, 700)) + list(range(700, 30000, 97))
    for tiles in range(1, 401):
        for cin in range(32, 2049, 32):                   # goalnet_conv3x3_fwd: Cin % 32 == 0
            got["conv_fwd"].add(S.order_class(tiles, S.conv_fwd_splits(tiles, 9 * cin // S.BK)))
        for kt in kts:
            got["linear_fwd"].add(S.order_class(tiles, S.pick_splits(tiles, kt)))
            got["wgrad"].add(S.order_class(tiles, S.wgrad_splits_of(tiles, kt)))
    assert got == REACHABLE


def test_every_reachable_class_has_a_row_and_sole_covers_are_known():
    cover = {role: {} for role in S.ROLES}
    for role in S.ROLES:
        for dims in S.ROWS[role]:
            cover[role].setdefault(_row_class(role, dims)[2], []).append(dims)
    # conv forward without a split: every row's ws = NULL run (with a workspace it takes 256 tiles: 32 768 pixels)
    assert ONE not in cover["conv_fwd"] and S.conv_fwd_splits(256, 72) == 1 and S.conv_fwd_splits(255, 72) == 3
    cover["conv_fwd"][ONE] = list(S.ROWS["conv_fwd"])
    for role in S.ROLES:
        assert set(cover[role]) == REACHABLE[role], (role, REACHABLE[role] ^ set(cover[role]))
    sole = {(role, cls): rows[0] for role in S.ROLES for cls, rows in cover[role].items() if len(rows) == 1}
    assert sole == {
        ("conv_fwd", FEW): (147, 4, 4, 256, 512), ("conv_fwd", LO1): (33, 11, 11, 512, 256), ("conv_fwd", LOG): (10, 11, 11, 512, 256),
        ("wgrad", ONE): (3, 5, 4, 36, 60), ("wgrad", FEW): (15, 4, 4, 64, 256), ("wgrad", MANY): (64, 4, 4, 1024, 512),
        ("wgrad", LO1): (63, 4, 4, 64, 256), ("wgrad", MID1): (63, 4, 4, 256, 512), ("wgrad", MIDP): (17, 11, 11, 256, 512),
        ("wgrad", HI1): (64, 4, 4, 512, 512), ("wgrad", HIG): (128, 4, 4, 512, 512), ("wgrad", HIP): (129, 4, 4, 512, 512),
        ("linear_fwd", ONE): (130, 224, 132), ("linear_fwd", FEW): (37, 640, 512), ("linear_fwd", LO1): (17, 2048, 128),
        ("linear_fwd", LOG): (100, 4096, 128), ("linear_fwd", LOP): (100, 1152, 128), ("linear_fwd", MIDG): (2176, 4096, 512),
        ("linear_fwd", MIDP): (2500, 3328, 512), ("linear_fwd", HI1): (5400, 2048, 260),
    }
    # the reduce kernels: the wide one and the capped grid have the weight gradient's rows only
    red = {}
    for role in S.ROLES:
        for dims in S.ROWS[role]:
            red.setdefault(S.reduce_of(role, dims), []).append((role, dims))
    assert set(red) == set(S.REDUCE_CLASSES) | {None}
    assert red["wide"] == [("wgrad", (1024, 4, 3, 32, 128)), ("wgrad", (1025, 4, 3, 32, 128))]
    assert red["plain-loop"] == [("wgrad", (64, 4, 4, 1024, 512))] and 512 * 9 * 1024 // 4 == 1179648 > S.REDUCE_GRID * 256
    # the rows that run with ticket counters are two-phase rows
    assert all(_row_class("wgrad", r[:5])[2][0] == "two-phase" for r in S.WGRAD_CTR) and len(S.WGRAD_CTR) == 4
    assert {_row_class("wgrad", r[:5])[2] for r in S.WGRAD_CTR} == {MID1, MIDG, MIDP}
    assert _row_class("conv_fwd", S.CONV_FWD_CTR[:5])[2] == MID1


def test_rows_sit_on_both_sides_of_every_boundary():
    xcd = {role: sorted((t, s) for t, s, cls, _ in EXPECT[role].values() if cls[0] in ("xcd-plain", "two-phase")) for role in S.ROLES}
    # 64 | 65 tiles: the forward rows at exactly 64 and exactly 65 tiles (one tile in the second phase)
    assert (64, 8) in xcd["conv_fwd"] and (65, 8) in xcd["conv_fwd"]
    assert S.order_class(64, 8) == LO1 and S.order_class(65, 8) == MID1
    # 128 | 129 tiles: linear forward at exactly 128 and 129 tiles
    assert (128, 8) in xcd["linear_fwd"] and (129, 8) in xcd["linear_fwd"]
    assert S.order_class(128, 8) == MID1 and S.order_class(129, 8) == HI1
    # 256 | 257: 144 and 288 tiles of the weight gradient; the conv forward stops splitting at 256 and linear forward at 8 splits above 146
    assert S.order_class(256, 8) == HI1 and S.order_class(257, 8) == MANY
    assert EXPECT["wgrad"][(64, 4, 4, 512, 512)][:2] == (144, 8) and EXPECT["wgrad"][(64, 4, 4, 1024, 512)][:2] == (288, 8)
    # 7 | 8 splits at a two-phase tile count: 76 tiles on grid.y, 68 in the XCD-local order
    assert EXPECT["conv_fwd"][(147, 4, 4, 256, 512)][:3] == (76, 7, FEW) and EXPECT["conv_fwd"][(17, 11, 11, 256, 512)][:3] == (68, 8, MID1)
    assert S.order_class(76, 7) == FEW and S.order_class(76, 8) == MID1
    # one group | several, whole | padded, in every band some role reaches
    for role in S.ROLES:
        assert {c for _, _, c, _ in EXPECT[role].values()} >= REACHABLE[role] - ({ONE} if role == "conv_fwd" else set())
    # select | correct: N max(H, W) = 4 096 and 4 100, the nearest multiples of H = 4 around the threshold
    a, b = S.WGRAD_THRESHOLD
    assert (a[0] * max(a[1:3]), b[0] * max(b[1:3])) == (4096, 4100)
    assert (S.wgrad_path(*a[:3]), S.wgrad_path(*b[:3])) == ("select", "correct")
    assert S.wgrad_path(4096, 1, 1) == "select" and S.wgrad_path(4097, 1, 1) == "correct" and S.wgrad_path(1, 4097, 2) == "correct"
    # every other weight-gradient row is far below the threshold: without GOALNET_WGRAD_PATH it takes "select", forced it takes both
    assert all(S.wgrad_path(*r[:3]) == "select" for r in S.WGRAD_ROWS)
    # reduce: 65 536 outputs and 32 splits bound the wide kernel
    assert S.reduce_class(65535, 32) == "wide" and S.reduce_class(65536, 32) == "plain" and S.reduce_class(65535, 31) == "plain"
    assert S.reduce_class(4096 * 256, 8) == "plain" and S.reduce_class(4096 * 256 + 1, 8) == "plain-loop"


# ---- unreachable classes, each with its reason ------------------------------------------------------------------------------------------
def test_a_padded_grid_needs_more_than_one_group():
    assert all(c not in S.ORDER_CLASSES for c in S.ORDER_IMPOSSIBLE)
    for nsplit in range(1, 600):
        for tiles in (1, 64, 65, 128, 129, 256):
            assert S.order_class(tiles, nsplit) not in S.ORDER_IMPOSSIBLE         # XCD-local starts at 8 splits, which is one whole group


def test_conv_forward_cannot_reach_8_splits_above_73_tiles():
    """~512 blocks: ceil(512 / tiles) is the most splits, 8 at 65 .. 73 tiles and 7 from 74 on; so no two-phase grid of several groups, no
    XCD-local order at 129 .. 256 tiles, and from 256 tiles on no split at all"""
    assert [t for t in range(1, 1000) if S.cdiv(512, t) >= 8] == list(range(1, 74))
    assert all(S.cdiv(512, t) == 8 for t in range(65, 74))
    for tiles in range(1, 1000):
        for kt in range(9, 1200, 9):
            assert S.conv_fwd_splits(tiles, kt) <= max(S.cdiv(512, tiles), 1)
            assert tiles < 256 or S.conv_fwd_splits(tiles, kt) == 1
    assert not REACHABLE["conv_fwd"] & {MIDG, MIDP, HI1, HIG, HIP, MANY}


def test_linear_forward_cannot_reach_more_than_8_splits_above_128_tiles():
    """~1024 blocks: ceil(1024 / tiles) is 8 at 129 .. 146 tiles and 7 from 147 on (short reductions: ~256 blocks, one split from 128 tiles)"""
    assert [t for t in range(129, 1000) if S.cdiv(1024, t) >= 8] == list(range(129, 147))
    assert all(S.cdiv(1024, t) == 8 for t in range(129, 147))
    for tiles in range(129, 600):
        for kt in list(range(1, 200)) + [1296, 5000]:
            assert S.pick_splits(tiles, kt) <= 8 and (tiles <= 146 or S.pick_splits(tiles, kt) < 8)
    assert not REACHABLE["linear_fwd"] & {HIG, HIP, MANY}


def test_the_wide_reduce_kernel_never_runs_a_second_round():
    """launch_splitk_reduce: wb = ceil(total / 16) blocks of 16 outputs, capped at 4 096; `total < 65536` keeps wb at or under the cap, so
    the grid covers every output and splitk_reduce_wide_kernel's `rounds` is 1"""
    assert S.cdiv(65535, 16) == 4096 == S.REDUCE_GRID
    for total in (1, 15, 16, 17, 4860, 9216, 65520, 65521, 65535):
        wb = min(S.cdiv(total, 16), S.REDUCE_GRID)
        assert S.cdiv(total, wb * 16) == 1
    assert S.reduce_class(65536, 64) != "wide"


# ---- the rows tests/test_gpu_ops.py had before ---------------------------------------------------------------------------------------------
def _ops_rows(fn, ndims):
    marks = [m for m in fn.pytestmark if m.name == "parametrize" and m.args[0].count(",") >= ndims - 1]
    return tuple(tuple(r[:ndims]) for r in marks[0].args[1])


def test_existing_rows_of_the_kernel_tests_have_these_classes():
    import test_gpu_ops as T
    assert _ops_rows(T.test_conv3x3_fwd, 5) == S.OPS_CONV_FWD and _ops_rows(T.test_conv3x3_wgrad, 5) == S.OPS_WGRAD
    assert tuple(r for r in _ops_rows(T.test_linear_fwd, 3) if r[0] > S.SKINNY_MAX_M) == S.OPS_LINEAR_FWD
    assert {d: _row_class("conv_fwd", d) for d in S.OPS_CONV_FWD} == {
        (2, 7, 5, 64, 256): (2, 4, FEW, "plain"), (3, 13, 13, 64, 256): (8, 4, FEW, "plain"), (2, 11, 11, 256, 512): (8, 18, LOP, "plain"),
        (2, 11, 11, 512, 256): (4, 36, LOP, "wide"), (2, 13, 13, 256, 64): (3, 18, LOP, "plain"), (16, 11, 11, 512, 256): (32, 16, LOG, "plain"),
        (16, 11, 11, 256, 512): (64, 8, LO1, "plain"), (1, 3, 3, 64, 128): (1, 4, FEW, "plain"), (40, 26, 22, 256, 64): (179, 3, FEW, "plain"),
        (3, 9, 7, 64, 32): (2, 4, FEW, "plain"), (2, 5, 5, 128, 60): (1, 9, LOP, "plain")}
    assert {d: _row_class("wgrad", d) for d in S.OPS_WGRAD} == {
        (2, 7, 5, 64, 256): (10, 1, ONE, "plain"), (3, 13, 13, 64, 256): (10, 4, FEW, "plain"), (2, 11, 11, 256, 512): (72, 2, FEW, "plain"),
        (5, 9, 6, 64, 128): (5, 2, FEW, "plain"), (16, 11, 11, 256, 512): (72, 8, MID1, "plain"), (16, 13, 13, 64, 256): (10, 15, LOP, "plain"),
        (40, 13, 13, 64, 256): (10, 43, LOP, "wide"), (2, 1, 9, 64, 128): (5, 1, ONE, "plain"), (3, 4, 1, 64, 128): (5, 1, ONE, "plain"),
        (1, 1, 1, 64, 128): (5, 1, ONE, "plain")}
    assert {d: _row_class("linear_fwd", d) for d in S.OPS_LINEAR_FWD} == {
        (37, 640, 512): (4, 5, FEW, "plain"), (130, 512, 256): (4, 4, FEW, "plain"), (17, 41472, 512): (4, 162, LOP, "wide")}
    # what they left to the tables above: no two-phase grid but the weight gradient's one group of 8, nothing above 128 tiles in the
    # XCD-local order, no 8 splits on grid.y, no capped reduce grid; and the weight gradient's path always forced
    old = {_row_class(role, d)[2] for role, rows in (("conv_fwd", S.OPS_CONV_FWD), ("wgrad", S.OPS_WGRAD), ("linear_fwd", S.OPS_LINEAR_FWD)) for d in rows}
    assert old == {ONE, FEW, LO1, LOG, LOP, MID1}
