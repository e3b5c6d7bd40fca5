"""Frame-width classes of the conv1 and max-pool / BatchNorm kernels, restated in plain Python, and the parameter tables of the GPU tests
that run every class (tests/test_gpu_width_classes.py and the rows it adds to the bit-identity tests of tests/test_gpu_ops.py,
tests/test_gpu_eval.py and tests/test_gpu_fp16.py). No torch, no GPU: tests/test_width_classes_host.py holds the tables against the rules.

The kernels of block 1 and of the three pool / BatchNorm rounds are compiled once per class of row width (staging slots per thread,
passes of 32 pixels per row). A class that no test's frame selects is code that has never run; a table row here is what selects it."""

LDS = 64 * 1024           # bytes of LDS a block may ask for: every "fits" below is the dispatcher's own `lds <= 64 * 1024`
CS = 32                   # channels per block slice of the pool / BatchNorm kernels (csrc/pool_bn.hip: CS)


def conv1_out(x):
    """Conv2d(k3, stride 3, pad 3): csrc/conv1.hip conv1_out"""
    return (x + 3) // 3 + 1


# ---- csrc/conv1.hip, goalnet_conv1_fwd: `lds`, `ns` and the if / else-if chain that launches conv1_fwd_v3_kernel<3|6|9|12>, v2 or v1 ----
def conv1_fwd_class(w):
    wo = conv1_out(w)
    lds = (27 * 64 + 9 * 3 * wo) * 4                       # the transposed weights and nine staged row segments
    ns = (9 * 3 * wo + 255) // 256                         # staging slots per thread
    if lds <= LDS and ns <= 12:
        return "v3<%d>" % (3 if ns <= 3 else 6 if ns <= 6 else 9 if ns <= 9 else 12)
    return "v2" if lds <= LDS else "v1"


CONV1_FWD_CLASSES = ("v3<3>", "v3<6>", "v3<9>", "v3<12>", "v2", "v1")
CONV1_FWD_GRID = 2048     # goalnet_conv1_fwd: `if (blocks > 2048) blocks = 2048`; a block prefetches row + 2048 while it computes row


# ---- csrc/conv1.hip, goalnet_conv1_wgrad: `lds` and the three launches (v3 when Wo % 4 == 0, v2, v1 past the LDS limit) ----------------
def conv1_wgrad_class(w):
    wo = conv1_out(w)
    lds = (9 * 3 * wo + wo * 64) * 4                       # nine staged row segments and one output row of dy
    if lds <= LDS:
        return "v3" if wo % 4 == 0 else "v2"
    return "v1"


CONV1_WGRAD_CLASSES = ("v3", "v2", "v1")
CONV1_WGRAD_GRID = 768    # WG_PARTS: blocks of every weight-gradient kernel


def rows_per_block(n, h, grid):
    """(fewest, most) output rows (n, oh) a block of the row-staged conv1 kernels walks: rows blockIdx, blockIdx + grid, ..."""
    rows = n * conv1_out(h)
    blocks = min(rows, grid)
    return rows // blocks, -(-rows // blocks)


# ---- csrc/pool_bn.hip, goalnet_pool_bnstats_fwd / goalnet_pool_bn_eval_fwd: `lds` of three conv rows, then launch_pool_fwd_v2's
# `switch ((Wc + 31) / 32)` over pool_bnstats_fwd_v2_kernel<.., NPW, STATS> --------------------------------------------------------------
def pool_fwd_class(wc):
    if 3 * wc * CS * 4 <= LDS:
        return ("v2", (wc + 31) // 32)
    return ("v1",)


POOL_FWD_CLASSES = tuple(("v2", k) for k in range(1, 7)) + (("v1",),)


# ---- csrc/pool_bn.hip, launch_pool_fwd_k16 (`wide`: 64-channel slices, WPL = 4, where C % 64 == 0) and launch_pool_fwd_k16_w's
# `switch ((Wc + 31) / 32)` over pool_bnstats_fwd_k16_kernel<F16, NPW, WPL, STATS>; the entry points require the v2 LDS limit -------------
def pool_fwd_k16_class(wc, c):
    assert c % CS == 0 and 3 * wc * CS * 4 <= LDS, "goalnet_pool_bnstats_fwd_p16 refuses this shape"
    wpl = 4 if c % 64 == 0 and 3 * wc * 64 * 2 <= LDS else 2
    return (wpl, (wc + 31) // 32)


POOL_K16_CLASSES = tuple((wpl, k) for wpl in (2, 4) for k in range(1, 7))


# ---- csrc/pool_bn.hip, goalnet_bnpool_bwd*: `lds` of three ring rows of Wc + 2 pixels (a float and an argmax byte per channel), then
# launch_bnpool_bwd_v2's `np`, `nc` and `switch (np * 2 + (nc - np))` over bnpool_bwd_v2_kernel<.., NPV, NCV, F16> ------------------------
def pool_bwd_class(wc):
    if 3 * (wc + 2) * CS * 5 <= LDS:
        return ((wc - 2 + 31) // 32, (wc + 31) // 32)       # passes of 32 pixels per pooled row, per conv row
    return ("v1",)


POOL_BWD_CLASSES = ((1, 1), (1, 2), (2, 2), (2, 3), (3, 3), (3, 4), (4, 4), (4, 5), (5, 5), ("v1",))
POOL_BWD_UNREACHABLE = (5, 6)      # the switch's `default`: needs a conv row of 161 pixels, the LDS limit stops at 134


def row_bands(parts, n, rows):
    """csrc/pool_bn.hip row_bands: partial rows beyond one per frame become bands of >= 3 rows (forward: pooled rows, backward: conv rows)"""
    return max(1, min(parts // n, rows // 3))


# ======================================================================================================================================
# tables of tests/test_gpu_width_classes.py
# ======================================================================================================================================
# (n, h, w) of conv1_case. Heights of 7 .. 9 pixels (four output rows, the first and the last of them padding only in part): a case is
# a few milliseconds on the device and its float64 reference a few more.
CONV1_FWD_EDGES = (           # the last width of a forward class and the first of the next
    (2, 7, 80), (2, 7, 81), (2, 8, 164), (2, 7, 165), (2, 9, 251), (2, 7, 252), (2, 7, 335), (2, 7, 336),
)
CONV1_FWD_V1 = ((1, 4, 1623),)                      # the first width whose nine row segments no longer fit LDS beside the weights
CONV1_WGRAD_ROWS = (
    (2, 7, 8),        # Wo = 4, the narrowest v3
    (2, 8, 44),       # Wo = 16
    (2, 7, 536),      # Wo = 180, the widest v3: 65 520 of the 65 536 bytes
    (1, 7, 537),      # Wo = 181: v1 with no switch set
    (2, 7, 81),       # Wo = 29: v2 (listed with the forward edges; named here for the host check)
)
CONV1_ROW_LOOPS = (
    (1030, 7, 8),     # 4 120 rows: forward blocks walk 2 or 3 with the prefetch, weight-gradient blocks 5 or 6; v3 in both
    (513, 7, 252),    # 2 052 rows: only blocks 0 .. 3 prefetch a second row; v3<12>
)
CONV1_ROWS = tuple(dict.fromkeys(CONV1_FWD_EDGES + CONV1_FWD_V1 + CONV1_WGRAD_ROWS + CONV1_ROW_LOOPS))

# (n, hc, wc, c, parts) of pool_bn_case; parts = 0: one partial row per frame
POOL_WIDTHS = (32, 33, 34, 35, 64, 65, 66, 67, 96, 97, 98, 99, 128, 129, 130, 131, 134, 135, 160, 161, 170, 171)
POOL_WIDTHS_C64 = (34, 98, 130, 170)
POOL_ROWS = (tuple((2, 5, wc, 32, parts) for wc in POOL_WIDTHS for parts in (0, 12))
             + tuple((2, 5, wc, 64, parts) for wc in POOL_WIDTHS_C64 for parts in (0, 12)))
# At hc = 5 a frame has three pooled rows, which row_bands() keeps in ONE band whatever `parts` is: the ten idle partial rows of parts = 12
# are all that those rows add. Nine conv rows and 12 partial rows give two forward bands (3 + 4 pooled rows) and three backward bands per
# frame: the widest width of every backward class, the (k, k + 1) ones first among them, runs with a band's ring warm-up and guard rows.
POOL_BAND_ROWS = tuple((2, 9, wc, 32, 12) for wc in (34, 66, 98, 130, 134, 170))

# ---- rows added to the bit-identity tests (16-bit and eval forms against the fp32 kernels held to fp64 above) ---------------------------
# test_gpu_eval.py::test_pool_bn_eval_fwd_equals_pool_bnstats_fwd (c, wc, kind); n = 2, hc = 9 there
EVAL_FWD_ROWS = (tuple((64, wc, "f32") for wc in (34, 66, 98, 130))
                 + tuple((64, wc, kind) for wc in (98, 130) for kind in ("bf16", "fp16", "bf16_y16", "fp16_y16")))
# test_gpu_ops.py::test_integer_key_pool_is_bit_identical_to_the_compare_and_select_kernel (n, hc, wc, c, kind)
K16_ROWS = ((2, 5, 98, 64, "relu"), (2, 5, 130, 64, "special"), (2, 5, 162, 64, "signed"), (2, 5, 170, 64, "relu"),
            (2, 5, 40, 32, "relu"), (2, 5, 98, 32, "special"), (2, 5, 170, 32, "signed"),
            (2, 5, 66, 32, "signed"), (2, 5, 130, 32, "relu"))        # the last two: WPL = 2 at three and five passes
K16_EXISTING = ((13, 256), (11, 512), (40, 64), (74, 64), (3, 32))   # (wc, c) of the rows that test had before
# test_bf16_pooled_activation_variants_..., test_batchnorm_backward_passes_with_bf16_gradient_input (test_gpu_ops.py) and
# test_fp16_pool_and_batchnorm_passes_... (test_gpu_fp16.py): (n, hc, wc, c)
H16_ROWS = tuple((2, 5, wc, 32) for wc in (34, 66, 98, 130, 134))

# ---- two whole-step cells on a 40 x 300 frame: (precision, head, audio, mode, n, (H, W)) of _mode_case.Cell ----------------------------
STEP_HW = (40, 300)
# conv-output sizes (hc, wc) of y1, y2, y3 and the pooled p3, by hand from (h + 3) // 3 + 1 and three times "- 2"
STEP_GEOMETRY = ((15, 102), (13, 100), (11, 98), (9, 96))
STEP_CELLS = (
    ("fp32", "regression", True, "train", 10, STEP_HW),
    ("bf16", "regression", False, "train", 10, STEP_HW),
)
# launches of (ops.pool_bn_fwd_small, ops.pool_bnstats_fwd, ops.pool_bn_eval_fwd): block 1 is 10 * 15 * 102 * 64 = 979 200 <= 2^20 fp32
# elements, the one-launch kernel in both precisions; block 2 (10 * 13 * 100 * 256 = 3 328 000) and block 3 (10 * 11 * 98 * 512) are over
STEP_LAUNCHES = (1, 2, 0)
SMALL_BN_ELEMS = 1 << 20
# what the frame is here for: conv1's widest row-prefetching kernel, and the pool / BatchNorm kernels of blocks 2 and 3 (conv rows of
# 100 and 98 pixels) at four forward passes and at (4, 4) / (3, 4) backward passes
STEP_CLASSES = {"conv1_fwd": "v3<12>", "pool_fwd": (("v2", 4), ("v2", 4)), "pool_bwd": ((4, 4), (3, 4))}
