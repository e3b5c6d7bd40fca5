"""GPU, op level: the data gradients behind AVM.input_gradients, through the raw C ABI with guard bands (tests/_abi_guard.py).

  goalnet_conv1_dgrad        against the fp64 CPU gradient of F.conv2d(stride=3, padding=3) wrt its input
  goalnet_conv1d_bwd(_small) the dx output at Cin = 30 (audbl.conv1: until now dx was only ever asked for at Cin = 64)

Bounds are derived, not tuned. An fp32 chain of n fused multiply-adds over exact products has |err| <= n u sum|terms| with
u = 2^-24 (each of the n roundings is at most u times a partial sum, itself at most sum|terms| (1 + n u)); inputs are fp32 on both
sides, so there is no input rounding to account for:
    conv1_dgrad   n = 64 (co)          |err| <= 64 * 2^-24 * sum_co |dy * w|
    conv1d dx     n = 64 * 3 (co, k)   |err| <= 192 * 2^-24 * sum_co,k |dz * w|       (any summation order of the 192 terms)
"""
import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

from _abi_guard import Bands, bits_equal, ptr  # noqa: E402
from cvml_goalnet_amd import _lib, ops  # noqa: E402

DEV = "cuda:0"
U = 2.0 ** -24


def _stream():
    return torch.cuda.current_stream().cuda_stream


def _conv1_case(n, h, w, seed):
    gen = torch.Generator().manual_seed(seed)
    ho, wo = (h + 3) // 3 + 1, (w + 3) // 3 + 1
    dy = torch.randn(n, ho, wo, 64, generator=gen) * torch.rand(n, ho, wo, 64, generator=gen).gt(0.3)      # NHWC, 30 % exact zeros
    wt = torch.randn(64, 3, 3, 3, generator=gen) * 0.2                                                      # OIHW
    return dy, wt


def _conv1_truth(dy_nhwc, w_oihw, n, h, w):
    """(fp64 gradient of conv2d wrt x, sum_co |dy * w| per element), both (N, 3, H, W)"""
    d = dy_nhwc.permute(0, 3, 1, 2).double()
    out = []
    for dd, ww in ((d, w_oihw.double()), (d.abs(), w_oihw.double().abs())):
        x = torch.zeros(n, 3, h, w, dtype=torch.float64, requires_grad=True)
        (F.conv2d(x, ww, stride=3, padding=3) * dd).sum().backward()
        out.append(x.grad)
    return out


def _run_conv1_dgrad(n, h, w, seed=11):
    dy, wt = _conv1_case(n, h, w, seed)
    truth, mag = _conv1_truth(dy, wt, n, h, w)
    lib = _lib.load()
    bands = Bands(DEV)
    dy_d = bands.place(dy.to(DEV))
    w_d = bands.place(wt.permute(0, 2, 3, 1).contiguous().to(DEV))           # OHWI, the arena's layout
    dx = bands.guarded((n, 3, h, w), torch.float32, name="dx")               # left holding NaN: an element never written shows
    sal = bands.guarded((n, h, w), torch.float32, name="sal")
    assert lib.goalnet_conv1_dgrad(ptr(dy_d), ptr(w_d), ptr(dx), 0, n, h, w, _stream()) == 0, lib.goalnet_last_error()
    assert lib.goalnet_conv1_dgrad(ptr(dy_d), ptr(w_d), ptr(sal), 1, n, h, w, _stream()) == 0, lib.goalnet_last_error()
    bands.assert_bands_intact()
    got = dx.cpu()
    assert torch.isfinite(got).all(), f"{int((~torch.isfinite(got)).sum())} elements of dx were never written"
    err = (got.double() - truth).abs()
    bound = 64 * U * mag
    worst = (err / bound.clamp_min(1e-300)).max().item()
    print(f"conv1_dgrad ({n},{h},{w}): max|err| {err.max().item():.3e}, max|dx| {truth.abs().max().item():.3e}, "
          f"worst err / (64 u sum|dy w|) = {worst:.3f}")
    assert (err <= bound).all(), f"{int((err > bound).sum())} elements beyond 64 u sum_co |dy w|; worst ratio {worst:.3f}"
    assert bits_equal(sal, dx.abs().amax(1)), "reduce=1 is not abs().amax(1) of reduce=0 bit for bit"
    return got


@pytest.mark.parametrize("n,h,w", [(1, 40, 40), (3, 41, 52), (2, 42, 40), (1, 224, 224)])
def test_conv1_dgrad_is_the_conv2d_data_gradient(n, h, w):
    """(3,41,52): non-square, W % 3 = 1 and H % 3 = 2; (2,42,40): H % 3 = 0, the last window row is all padding;
    (1,224,224): 5 776 output pixels = 91 chunks of 64, the last one partial"""
    _run_conv1_dgrad(n, h, w)


def test_conv1_dgrad_beyond_one_pass_of_the_grid():
    """600 x 15 x 15 = 135 000 output pixels: more than the 2 048 blocks x 64 pixels of one pass, so blocks take a second chunk"""
    _run_conv1_dgrad(600, 40, 40, seed=12)


def _conv1d_truth(x, dz_eff, wt):
    """fp64 dx of Conv1d(k3, s2, p1) and sum |dz * w| per element"""
    out = []
    for dd, ww in ((dz_eff.double(), wt.double()), (dz_eff.double().abs(), wt.double().abs())):
        xx = torch.zeros(x.shape, dtype=torch.float64, requires_grad=True)
        (F.conv1d(xx, ww, stride=2, padding=1) * dd).sum().backward()
        out.append(xx.grad)
    return out


def _conv1d_case(n, cin, L, cout, seed):
    gen = torch.Generator().manual_seed(seed)
    lo = (L + 2 - 3) // 2 + 1
    x = torch.randn(n, cin, L, generator=gen)
    wt = torch.randn(cout, cin, 3, generator=gen) * 0.1
    y = F.relu(torch.randn(n, cout, lo, generator=gen))                      # the layer's ReLU output: about half the gates closed
    dz = torch.randn(n, cout, lo, generator=gen)
    return x, wt, y, dz


def _check_dx(tag, got, truth, mag):
    err = (got.double() - truth).abs()
    bound = 192 * U * mag
    worst = (err / bound.clamp_min(1e-300)).max().item()
    print(f"{tag}: max|err| {err.max().item():.3e}, max|dx| {truth.abs().max().item():.3e}, worst err / (192 u sum|dz w|) = {worst:.3f}")
    assert torch.isfinite(got).all() and (err <= bound).all(), f"{tag}: worst ratio {worst:.3f}"


@pytest.mark.parametrize("bins", [30, 31])
def test_conv1d_bwd_small_dx_at_cin_30(bins):
    """audbl.conv1's shape at N = 3: dx asked for at Cin = 30; dw / db are bit-equal to the call without dx (the existing use)"""
    n, cin, cout = 3, 30, 64
    x, wt, y, dz = _conv1d_case(n, cin, bins, cout, 20 + bins)
    truth, mag = _conv1d_truth(x, dz * (y > 0), wt)
    lib = _lib.load()
    bands = Bands(DEV)
    xd, dzd, yd, wd = (bands.place(t.to(DEV)) for t in (x, dz, y, wt))
    dx = bands.guarded((n, cin, bins), torch.float32, name="dx")
    dw, db = bands.guarded((cout, cin, 3), torch.float32, name="dw"), bands.guarded(cout, torch.float32, name="db")
    dw0, db0 = bands.guarded((cout, cin, 3), torch.float32, name="dw0"), bands.guarded(cout, torch.float32, name="db0")
    rc = lib.goalnet_conv1d_bwd_small(ptr(xd), ptr(dzd), ptr(yd), ptr(wd), ptr(dx), ptr(dw), ptr(db), n, cin, bins, cout, 2, 1, _stream())
    assert rc == 0, lib.goalnet_last_error()
    rc = lib.goalnet_conv1d_bwd_small(ptr(xd), ptr(dzd), ptr(yd), ptr(wd), None, ptr(dw0), ptr(db0), n, cin, bins, cout, 2, 1, _stream())
    assert rc == 0, lib.goalnet_last_error()
    bands.assert_bands_intact()
    _check_dx(f"conv1d_bwd_small dx (N=3, Cin=30, B={bins})", dx.cpu(), truth, mag)
    assert bits_equal(dw, dw0) and bits_equal(db, db0), "asking for dx changed dw / db"


@pytest.mark.parametrize("n", [64, 515])
def test_conv1d_bwd_dx_at_cin_30(n):
    """the many-frame kernels (N >= 64), and at N = 515 with the frame-sliced weight gradient's workspace lent"""
    cin, cout, bins = 30, 64, 30
    x, wt, _, dz = _conv1d_case(n, cin, bins, cout, 40 + n)
    truth, mag = _conv1d_truth(x, dz, wt)
    lib = _lib.load()
    need = lib.goalnet_conv1d_bwd_ws_bytes(n, cin, cout)
    assert (need > 0) == (n == 515)
    bands = Bands(DEV)
    xd, dzd, wd = (bands.place(t.to(DEV)) for t in (x, dz, wt))
    dx = bands.guarded((n, cin, bins), torch.float32, name="dx")
    dw, db = bands.guarded((cout, cin, 3), torch.float32, name="dw"), bands.guarded(cout, torch.float32, name="db")
    dw0, db0 = bands.guarded((cout, cin, 3), torch.float32, name="dw0"), bands.guarded(cout, torch.float32, name="db0")
    ws = bands.guarded(need // 8, torch.float64, name="ws") if need else None
    for dxp, dwp, dbp in ((dx, dw, db), (None, dw0, db0)):
        rc = lib.goalnet_conv1d_bwd(ptr(xd), ptr(dzd), ptr(wd), ptr(dxp), ptr(dwp), ptr(dbp), n, cin, bins, cout, 2, 1, ptr(ws), need, _stream())
        assert rc == 0, lib.goalnet_last_error()
    bands.assert_bands_intact()
    _check_dx(f"conv1d_bwd dx (N={n}, Cin=30)", dx.cpu(), truth, mag)
    assert bits_equal(dw, dw0) and bits_equal(db, db0), "asking for dx changed dw / db"


def test_ops_wrapper_refuses_wrong_shapes():
    dy = torch.zeros(1, 15, 15, 64, device=DEV)
    wt = torch.zeros(64 * 27, device=DEV)
    with pytest.raises(RuntimeError):
        ops.conv1_dgrad(dy, wt, torch.empty(1, 3, 40, 41, device=DEV), 0, 1, 40, 40)
    with pytest.raises(RuntimeError):
        ops.conv1_dgrad(dy, wt, torch.empty(1, 3, 40, 40, device=DEV), 1, 1, 40, 40)          # reduce=1 writes (N, H, W)
    out = ops.conv1_dgrad(dy, wt, torch.full((1, 40, 40), float("nan"), device=DEV), 1, 1, 40, 40)
    assert bool((out == 0).all())
