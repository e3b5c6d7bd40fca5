"""CPU: the split counts of the 256 x 256 tile's two split-K roles (wgrad_splits_256 / linear_fwd_splits_256 of gemm_bf16_256.hip, one
function each for plain operands, scaled fp16 pairs and bf16 triples), pinned through the *_ws_bytes entry points that show them.
The values were recorded from the build before the per-form helpers were folded into those two functions; the shapes reach both
clamps (>= 64 K-tiles per split, the cap on the count) and the rounding to whole 256-CU rounds / XCD groups. A workspace is whole
slabs, so the tables hold slab counts. Plain operands: the entry point sizes for the larger of the 128 x 128 and the 256 x 256
tile's count."""
import pytest

from cvml_goalnet_amd import _lib

# (N, H, W, Cin, Cout) -> slabs of [Cout][9 Cin] fp32 for (plain, parts = 2, parts = 3)
WGRAD = {
    (2, 9, 11, 64, 256): (1, 1, 1),
    (16, 56, 56, 256, 512): (29, 39, 78),
    (128, 74, 74, 64, 256): (203, 534, 680),
    (1024, 36, 36, 256, 512): (128, 128, 128),
}
# (M, K, J) -> slabs of [M][J] fp32 for (plain, parts = 2, parts = 3)
LINEAR_FWD = {
    (256, 65536, 256): (128, 48, 96),
    (512, 2 ** 18, 512): (64, 192, 256),
    (1024, 2506752, 512): (128, 128, 128),
}


@pytest.mark.parametrize("dims", WGRAD, ids=lambda d: "x".join(map(str, d)))
def test_wgrad_workspace_is_the_pinned_number_of_slabs(dims):
    lib = _lib.load()
    n, h, w, cin, cout = dims
    slab = cout * 9 * cin * 4
    got = (lib.goalnet_conv3x3_wgrad_bf16_ws_bytes(*dims),) + tuple(lib.goalnet_conv3x3_wgrad_split_ws_bytes(p, *dims) for p in (2, 3))
    assert got == tuple(s * slab for s in WGRAD[dims])


@pytest.mark.parametrize("dims", LINEAR_FWD, ids=lambda d: "x".join(map(str, d)))
def test_linear_fwd_workspace_is_the_pinned_number_of_slabs(dims):
    lib = _lib.load()
    m, k, j = dims
    slab = m * j * 4
    assert all(lib.goalnet_linear_split_ok(p, m, k, j) for p in (2, 3))
    got = (lib.goalnet_linear_fwd_bf16_ws_bytes(*dims),) + tuple(lib.goalnet_linear_fwd_split_ws_bytes(p, *dims) for p in (2, 3))
    assert got == tuple(s * slab for s in LINEAR_FWD[dims])
