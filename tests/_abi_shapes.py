"""Shape tables of tests/test_gpu_abi_contract.py, kept apart from it so that tests/test_abi_contract_host.py can read them on a
machine without a GPU. WS_ROWS lists, per workspace-taking entry point of the GPU table, its *_ws_bytes function, the dims of its
rows as that function takes them, and whether the header makes the workspace optional."""

CONV_FWD = [   # n, h, w, cin, cout, affine, bias, relu: rows of test_conv3x3_fwd
    (2, 7, 5, 64, 256, True, True, True),          # M below one tile
    (3, 9, 7, 64, 32, True, True, True),           # ragged Cout (128 x 64 tile, 32 columns valid)
    (2, 5, 5, 128, 60, False, True, False),        # ragged Cout
    (40, 26, 22, 256, 64, False, False, False),    # ragged last M-tile (split-K once a workspace is lent)
    (64, 26, 22, 64, 64, True, True, False),       # ragged last M-tile, ws_bytes = 0: no split, ws = NULL
]
CONV_FWD_SPLIT = (10, 11, 11, 256, 512, True, True, True)      # split-K: ws_bytes > 0
CONV_WGRAD = [(16, 13, 13, 64, 256, True), (2, 1, 9, 64, 128, True), (1, 1, 1, 64, 128, True)]      # rows of test_conv3x3_wgrad
LINEAR_FWD = [(16, 1056, 260, False, True, 0), (7, 41472, 512, True, False, 128), (17, 41472, 512, True, True, 0)]
LINEAR_DX = [(16, 1000, 96, True)]
LINEAR_DW = [(16, 1028, 36, False)]

# entry point -> (its *_ws_bytes function, dims of every row as that function takes them, workspace optional?)
BN_SMALL = [(3, 3, 5, 256), (16, 15, 13, 64)]      # n, hc, wc, c: rows of test_small_pool_batchnorm_forward_and_backward_vs_fp64
MLP_ROWS = [(1, 640, True), (9, 640, True), (16, 640, True)]      # n, k0, masks: rows of test_fused_mlp_forward_and_backward_vs_fp64
CONV1D = [(515, 30), (70, 30), (63, 21)]           # n, bins: frame slices (ws_bytes > 0), many frames without slices, the one-launch form

WS_ROWS = {
    "goalnet_conv3x3_fwd": ("goalnet_conv3x3_fwd_ws_bytes", [r[:5] for r in CONV_FWD + [CONV_FWD_SPLIT]], True),
    "goalnet_conv3x3_wgrad": ("goalnet_conv3x3_wgrad_ws_bytes", [r[:5] for r in CONV_WGRAD], False),
    "goalnet_linear_fwd": ("goalnet_linear_fwd_ws_bytes", [r[:3] for r in LINEAR_FWD], False),
    "goalnet_pool_bn_fwd_small": ("goalnet_bn_small_ws_bytes", [r[3:] for r in BN_SMALL], False),
    "goalnet_bn_bwd_reduce_small": ("goalnet_bn_small_ws_bytes", [r[3:] for r in BN_SMALL], False),
    "goalnet_bn_bwd_reduce_small_eval": ("goalnet_bn_small_ws_bytes", [r[3:] for r in BN_SMALL], False),
    "goalnet_bnpool_bwd_small": ("goalnet_bn_small_ws_bytes", [r[3:] for r in BN_SMALL], False),
    "goalnet_mlp_bwd": ("goalnet_mlp_bwd_ws_bytes", [r[:1] for r in MLP_ROWS], False),
    "goalnet_conv1d_bwd": ("goalnet_conv1d_bwd_ws_bytes", [(n, 64, 128) for n, _ in CONV1D[:2]] + [(n, 30, 64) for n, _ in CONV1D[:2]], True),
}

CONV1 = [(3, 41, 38), (3, 33, 9)]                  # n, h, w: rows of test_conv1_fwd_and_wgrad
POOL = [(2, 76, 9, 64, 37), (2, 40, 37, 32, 16)]   # n, hc, wc, c, nparts: C % 32 == 0, ragged pooled pixel counts
# the 16-bit engine: the smallest and the most ragged shape of each parametrisation of tests/test_gpu_ops.py
BF16_CONV = [(1, 7, 5, 64, 256, True, True), (3, 7, 7, 64, 260, False, False), (3, 9, 7, 64, 32, True, True)]     # the last: 128 x 64 tile
BF16_WGRAD = [(2, 7, 5, 64, 256), (5, 9, 6, 64, 128)]
BF16_LINEAR_FWD = [(37, 640, 512), (300, 8192, 320)]
BF16_LINEAR_BWD = [(37, 640, 512, True), (300, 4168, 320, False)]
O16_CONV = (3, 9, 11, 64, 72)                      # test_bf16_gradient_outputs_equal_the_fp32_outputs_rounded_once
O16_LINEAR = (70, 1032, 128)
SPLIT_CONV = (2, 9, 11, 64, 256, True, True)
SPLIT_LINEAR = (320, 66048 + 64, 256, 64)          # m, k, j, bnC: the linear_split_ok shape of test_linear5_on_split_operands_forward_dx_dw_vs_fp64

WS_ROWS.update({
    "goalnet_conv1_wgrad": ("goalnet_conv1_wgrad_ws_bytes", CONV1, False),
    "goalnet_conv3x3_fwd_bf16p": ("goalnet_conv3x3_fwd_bf16p_ws_bytes", [r[:5] for r in BF16_CONV], False),
    "goalnet_conv3x3_wgrad_bf16": ("goalnet_conv3x3_wgrad_bf16_ws_bytes", BF16_WGRAD, False),
    "goalnet_linear_fwd_bf16": ("goalnet_linear_fwd_bf16_ws_bytes", BF16_LINEAR_FWD, False),
    "goalnet_conv3x3_wgrad_split": ("goalnet_conv3x3_wgrad_split_ws_bytes", [(parts,) + SPLIT_CONV[:5] for parts in (3, 2)], False),
    "goalnet_linear_fwd_split": ("goalnet_linear_fwd_split_ws_bytes", [(parts,) + SPLIT_LINEAR[:3] for parts in (3, 2)], False),
})
