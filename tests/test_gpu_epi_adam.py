"""GPU: linear5's weight gradient with the Adam update in the GEMM's epilogue (goalnet_linear_bwd_dw_adam, EPIK_ADAM in
csrc/gemm_f32.hip) against the two launches it replaces: ops.linear_bwd_dw into a gradient buffer, then ops.adam_step_dev on it.

The fused launch computes each 128 x 128 tile of the gradient with the same K loop (same MFMA sequence per output) and runs
csrc/adam.h's adam1 under adam_scalars — the code adam_kernel runs — on the accumulators, so p, m and v must be the same bits
(torch.equal) after every step. Shapes M (frames) x J x K, the smallest that reach every edge of the tile walk above the
weight-streaming rows (M > 16):
  40 x 132 x 260   ragged K-tile (40 = 32 + 8), ragged row tile (132 = 128 + 4), ragged column tile (260 = 2 x 128 + 4), with the
                   BatchNorm affine on x over bnC = 52 channels (260 = 5 x 52: a tile's columns wrap the channel index)
  33 x 128 x 128   one full tile, one K-tile plus one row, no affine
Two steps under the device step counter (bias 1, the counter ticked between them as train_step does) and grad_scale = 0.37 (no
power of two: the scaled gradient is rounded, by the same instruction in both paths)."""
import pytest
import torch

pytestmark = pytest.mark.gpu

from _abi_guard import Bands  # noqa: E402
from cvml_goalnet_amd import _lib, ops  # noqa: E402

DEV = "cuda:0"
LR, B1, B2, EPS, GS = 1e-3, 0.9, 0.999, 1e-8, 0.37
SHAPES = [(40, 132, 260, 52), (33, 128, 128, 0)]


def rnd(*shape, seed=0, lo=-1.0, hi=1.0):
    g = torch.Generator().manual_seed(seed)
    return (torch.rand(*shape, generator=g, dtype=torch.float64) * (hi - lo) + lo).float().to(DEV)


def inputs(M, J, K, bnC, step):
    dy = rnd(M, J, seed=10 * step + 1)
    x = rnd(M, K, seed=10 * step + 2)
    sc = rnd(bnC, seed=3, lo=0.5, hi=1.5) if bnC else None
    sh = rnd(bnC, seed=4, lo=-0.5, hi=0.5) if bnC else None
    return dy, x, sc, sh


@pytest.mark.parametrize("M,J,K,bnC", SHAPES, ids=lambda v: str(v))
def test_fused_update_is_the_two_launches_bit_for_bit(M, J, K, bnC):
    bands = Bands(DEV)
    p0, m0, v0 = rnd(J * K, seed=5), torch.zeros(J * K, device=DEV), torch.zeros(J * K, device=DEV)
    # the reference: gradient buffer, then the stand-alone pass
    pr, mr, vr = p0.clone(), m0.clone(), v0.clone()
    pf, mf, vf = bands.guarded(J * K, torch.float32, fill=p0, name="p"), bands.guarded(J * K, torch.float32, fill=m0, name="m"), \
        bands.guarded(J * K, torch.float32, fill=v0, name="v")
    step_r, step_f = torch.zeros(1, dtype=torch.int64, device=DEV), torch.zeros(1, dtype=torch.int64, device=DEV)
    for step in (1, 2):
        dy, x, sc, sh = inputs(M, J, K, bnC, step)
        g = torch.full((J * K,), float("nan"), device=DEV)
        ops.linear_bwd_dw(dy, x, g, scale=sc, shift=sh, bnC=bnC)
        ops.adam_step_dev(pr, g, mr, vr, LR, B1, B2, EPS, step_r, grad_scale=GS, step_bias=1)
        ops.counter_add(step_r, 1)
        ops.linear_bwd_dw_adam(dy, x, pf, mf, vf, LR, B1, B2, EPS, step_f, scale=sc, shift=sh, bnC=bnC, grad_scale=GS, step_bias=1)
        ops.counter_add(step_f, 1)
        torch.cuda.synchronize()
        for name, a, b in (("p", pf, pr), ("m", mf, mr), ("v", vf, vr)):
            d = (a - b).abs().max().item()
            print(f"[epi_adam] {M}x{J}x{K} step {step} {name}: max|fused - two launches| = {d:.3e}, differing elements = {(a != b).sum().item()}")
            assert torch.equal(a, b), f"step {step}: {name} differs"
        assert not torch.equal(pf, p0) and mf.abs().max().item() > 0 and vf.abs().max().item() > 0, "the update ran"
    bands.assert_bands_intact()


def test_bias_gradient_comes_with_it():
    M, J, K, bnC = SHAPES[1]
    dy, x, _, _ = inputs(M, J, K, bnC, 1)
    p, m, v = rnd(J * K, seed=5), torch.zeros(J * K, device=DEV), torch.zeros(J * K, device=DEV)
    db, want = torch.full((J,), float("nan"), device=DEV), torch.empty(J, device=DEV)
    ops.linear_bwd_dw_adam(dy, x, p, m, v, LR, B1, B2, EPS, torch.zeros(1, dtype=torch.int64, device=DEV), db=db, step_bias=1)
    ops.colsum(dy, want)
    assert torch.equal(db, want)


@pytest.mark.parametrize("what", ["misaligned_m", "weight_streaming_rows"])
def test_refused_call_leaves_the_arrays_alone(what):
    M, J, K, bnC = SHAPES[1]
    if what == "weight_streaming_rows":
        M = 16
    dy, x, _, _ = inputs(M, J, K, bnC, 1)
    bands = Bands(DEV)
    p = bands.guarded(J * K, torch.float32, fill=rnd(J * K, seed=5), name="p")
    v = bands.guarded(J * K, torch.float32, fill=0.25, name="v")
    mbuf = bands.guarded(J * K + 4, torch.float32, fill=0.5, name="m")
    m = mbuf[1:J * K + 1] if what == "misaligned_m" else mbuf[:J * K]           # 4 bytes off a 16-byte boundary
    before = [t.clone() for t in (p, mbuf, v)]
    with pytest.raises(_lib.GoalnetError):
        ops.linear_bwd_dw_adam(dy, x, p, m, v, LR, B1, B2, EPS, torch.zeros(1, dtype=torch.int64, device=DEV), step_bias=1)
    torch.cuda.synchronize()
    for t, b in zip((p, mbuf, v), before):
        assert torch.equal(t, b)
    bands.assert_bands_intact()
