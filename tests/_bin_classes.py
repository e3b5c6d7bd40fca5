"""Audio bin-length classes of AudBl, restated in plain Python, and the parameter tables of the GPU tests that run every class
(tests/test_gpu_bin_classes.py, the cells tests/test_gpu_mode_matrix.py takes from here). No torch, no GPU:
tests/test_bin_classes_host.py holds the tables against the rules, and the rules against the library's own query.

The audio input is (N, 30, B) with B = bin_length = skip_frames, a number the user picks (15, 30 and 60 are usual). B selects code:
whether a Conv1d layer's one-launch backward fits LDS, which skinny kernel runs audbl.linear3 (K = 128 * l2), and how the last window of
a stride-2, pad-1 Conv1d is cut. A class that no test's B selects is code that has never run; a table row here is what selects it."""

SMALL_LDS = 48 * 1024     # csrc/small.hip goalnet_conv1d_bwd_small_ok: `N * cpb * Lo * sizeof(float) <= 48 * 1024`
SMALL_MAX_N = 63          # the same function: `N < 64`
SKINNY_MAX_M = 16         # csrc/skinny.h SKINNY_MAX_M: rows up to which the linear layers run the weight-streaming kernels
KT = 512                  # csrc/skinny.hip `constexpr int KT = 512`: K-slab per block of the skinny forward

CONV1 = (30, 64)          # (Cin, Cout) of audbl.conv1; its L is B
CONV2 = (64, 128)         # audbl.conv2; its L is l1(B)


def conv1d_out(length, stride=2, pad=1):
    """csrc/small.hip, every conv1d entry point: `Lo = (L + 2 * pad - 3) / stride + 1`"""
    return (length + 2 * pad - 3) // stride + 1


def l1(b):
    """cvml_goalnet_amd/avm.py forward_device: `l1 = (bins - 1) // 2 + 1` = ceil(B / 2)"""
    return (b - 1) // 2 + 1


def l2(b):
    """forward_device: `l2 = (l1 - 1) // 2 + 1` = ceil(l1 / 2); audbl.linear3 has K = 128 * l2"""
    return (l1(b) - 1) // 2 + 1


def k3(b):
    return 128 * l2(b)


# ---- csrc/small.hip, goalnet_conv1d_bwd_small_ok: `cpb = 256 / Cin`, the dz rows of cpb output channels for all N frames in LDS ---------
def small_fits(n, cin, length, stride=2, pad=1):
    if not (0 < n <= SMALL_MAX_N and 0 < cin <= 256 and length > 0 and length + 2 * pad >= 3):
        return False
    return n * (256 // cin) * conv1d_out(length, stride, pad) * 4 <= SMALL_LDS


def conv1_fits(n, b):
    return small_fits(n, CONV1[0], b)


def conv2_fits(n, b):
    return small_fits(n, CONV2[0], l1(b))


def refused_from(fits, b):
    """the first n < 64 the one-launch form does not serve at bin length b, None where it serves them all"""
    return next((n for n in range(1, SMALL_MAX_N + 1) if not fits(n, b)), None)


# ---- csrc/skinny.hip: `skinny_fwd_splits(K) = (K + KT - 1) / KT`; launch_skinny_fwd: `if (KS >= 8)` <MR, 4, 1> else <MR, 1, 1>, and
# `if (KS == 1) return 0` (no workspace, epilogue inside the kernel) ---------------------------------------------------------------------
def skinny_fwd_splits(k):
    return (k + KT - 1) // KT


def skinny_fwd_class(k):
    ks = skinny_fwd_splits(k)
    return "direct" if ks == 1 else "<MR,4,1>" if ks >= 8 else "<MR,1,1>"


# ---- csrc/skinny.hip launch_skinny_dx / launch_skinny_dw: `if (K > 4096)` the <MR, 16> kernels, else <MR, 4> -------------------------
def skinny_bwd_class(k):
    return "<MR,16>" if k > 4096 else "<MR,4>"


def linear3_engine(m):
    return "skinny" if m <= SKINNY_MAX_M else "gemm"


# the refusal table of DESIGN.md §5: bin length -> the first batch size below 64 that the one-launch backward of audbl.conv1 / conv2 does
# not serve (on those AVM.backward_device takes relu_bwd + conv1d_bwd)
CONV1_REFUSED_FROM = {60: 52, 61: 50, 64: 49, 100: 31, 120: 26, 200: 16, 256: 13}
CONV2_REFUSED_FROM = {200: 62, 256: 49}

# ======================================================================================================================================
# tables of tests/test_gpu_bin_classes.py
# ======================================================================================================================================
# (n, B) of test_gpu_ops.audbl_conv1d_case
CONV1D_EXISTING = ((1, 30), (10, 30), (33, 17), (70, 30), (257, 21), (515, 30))     # the rows test_gpu_ops.py::test_audbl_conv1d had before
CONV1D_EDGES = (          # B = 1, 2, 3 (l1 <= 2, l2 = 1), every B mod 4 at short and usual lengths, both sides of skinny KS 1 | 2
    (2, 1), (2, 2), (2, 3), (2, 4), (2, 5), (10, 15), (10, 16), (10, 17), (10, 31), (10, 32), (10, 33),
)
CONV1D_LONG = ((10, 60), (10, 61), (3, 200), (3, 256))
CONV1D_FIT = (            # the last n a layer's one-launch backward serves and the first it does not, through the dispatch AVM uses
    (51, 60), (52, 60),   # conv1 at B = 60: 51 * 30 = 1530 <= 1536 < 52 * 30
    (63, 60),             # the last n below the many-frame kernels: conv1 multi-launch, conv2 one launch
    (61, 200), (62, 200),  # conv2 at B = 200 (l1 = 100, l2 = 50): 61 * 50 = 3050 <= 3072 < 62 * 50; conv1 fits neither
)
CONV1D_MANY = ((64, 60), (70, 61), (515, 60))          # the many-frame kernels; >= 512: frame slices
CONV1D_ROWS = CONV1D_EDGES + CONV1D_LONG + CONV1D_FIT + CONV1D_MANY

# audbl.linear3: J = 128, K = 128 * l2
LINEAR3_M = (10, 16, 17, 60)                           # 16 | 17: the last skinny row count and the first on the GEMM engine
LINEAR3_L2 = (1, 4, 5, 15, 28, 29, 32, 33)             # KS 1 | 2 at l2 4 | 5, KS 7 | 8 at 28 | 29, K 4096 | 4224 at 32 | 33; 15: B = 60
LINEAR3_ROWS = tuple((m, k) for m in LINEAR3_M for k in LINEAR3_L2)

# ---- whole steps, all audio-on at 40 x 40: (precision, head, mode, n, B) and the classes the cell is here for --------------------------
STEP_CELLS = (
    # skinny linear3 at KS = 4 with a ragged last slab (K = 1920 = 3 * 512 + 384); both Conv1d backwards in one launch
    (("fp32", "regression", "train", 10, 60), {"l1": 30, "l2": 15, "ks": 4, "engine": "skinny", "conv1_fits": True, "conv2_fits": True}),
    # the region the one-launch conv1 backward refused (60 * 30 = 1800 > 1536); conv2 still fits; linear3 on the GEMM engine
    (("fp32", "regression", "train", 60, 60), {"l1": 30, "l2": 15, "ks": 4, "engine": "gemm", "conv1_fits": False, "conv2_fits": True}),
    # KS = 1: no workspace, the epilogue inside the kernel
    (("fp32", "regression", "train", 10, 15), {"l1": 8, "l2": 4, "ks": 1, "engine": "skinny", "conv1_fits": True, "conv2_fits": True}),
    # l1 = l2 = 1, K = 128: every Conv1d window is cut on both sides
    (("fp32", "regression", "train", 10, 2), {"l1": 1, "l2": 1, "ks": 1, "engine": "skinny", "conv1_fits": True, "conv2_fits": True}),
    # odd B, odd l1
    (("fp32", "classifier", "eval", 32, 17), {"l1": 9, "l2": 5, "ks": 2, "engine": "gemm", "conv1_fits": True, "conv2_fits": True}),
    # AudBl stays fp32 under a 16-bit step
    (("bf16", "regression", "train", 32, 60), {"l1": 30, "l2": 15, "ks": 4, "engine": "gemm", "conv1_fits": True, "conv2_fits": True}),
)


def step_classes(n, b):
    return {"l1": l1(b), "l2": l2(b), "ks": skinny_fwd_splits(k3(b)), "engine": linear3_engine(n), "conv1_fits": conv1_fits(n, b),
            "conv2_fits": conv2_fits(n, b)}


INPUTGRAD_CELL = ("fp32", 3, 60)                       # precision, n, B of the input-gradient cell
LOOP_ROW = (23, 10, (60, 59))                          # frames, sub-batch, the two bin lengths (the same l2) of the graph-loop row
