"""GPU: the buffer-store epilogue of the fp32 GEMM tiles (store_acc_buf / store_acc_n64_buf, csrc/gemm_f32.hip) against the
per-store-predicated epilogue it replaces (store_acc / store_acc_n64).

The new epilogue changes addressing only: one buffer resource per block spanning the tile's rows, the lane's row and column in a
32-bit voffset (out of range past `cols`), the register's row term in a scalar offset, 8-byte stores where a lane's two fragments
are adjacent columns. The values are the same expressions, so every case runs once per setting of GOALNET_F32_EPI_STORE (read per
call: unset = default dispatch, 1 = 4-byte buffer stores only, 0 = the old epilogue) and the results must agree bit for bit
(torch.equal on int32 views). Every output lies inside a buffer filled with a sentinel bit pattern: the bands around it (and, for
column slices, the neighbouring columns) must come back untouched and no sentinel may survive inside the output. The shapes are
the smallest at which the addressing can go wrong: a one-row tile, ragged row tiles next to a full one, columns past `cols`, the
128 x 64 tile, raw split-K slabs with and without the fused reduction, ld > cols, a leading dimension too wide for one resource.
The weight gradient (both operands row-contiguous) keeps the old epilogue under every setting: its case pins that the switch
leaves it alone."""
import ctypes
import os

import pytest
import torch

pytestmark = pytest.mark.gpu

from cvml_goalnet_amd import ops  # noqa: E402
from cvml_goalnet_amd._lib import check  # noqa: E402

DEV = "cuda:0"
SENT = 0x7FC5A5A5       # a quiet NaN with a payload no arithmetic here produces
PAD = 1024              # floats of guard band on either side (16-byte aligned)
ENV = "GOALNET_F32_EPI_STORE"
SETTINGS = (None, "1", "0")


def rnd(*shape, seed=0, lo=-1.0, hi=1.0):
    g = torch.Generator().manual_seed(seed)
    return ((torch.rand(*shape, generator=g, dtype=torch.float64) * (hi - lo) + lo).float()).to(DEV)


class Guarded:
    """`numel` floats of output between two sentinel bands"""

    def __init__(self, numel):
        self.n = numel
        self.buf = torch.empty(numel + 2 * PAD, dtype=torch.int32, device=DEV)
        self.out = self.buf[PAD:PAD + numel].view(torch.float32)

    def reset(self):
        self.buf.fill_(SENT)

    def bits(self):
        return self.buf[PAD:PAD + self.n]

    def bands_untouched(self):
        return bool((self.buf[:PAD] == SENT).all()) and bool((self.buf[PAD + self.n:] == SENT).all())


def run_settings(g, call, written=None, name=""):
    """call() under every setting of the switch; returns nothing, asserts guard bands, full coverage and bitwise agreement.
    written: boolean mask over g.bits() of the elements the call must write (default: all of them)"""
    saved = os.environ.get(ENV)
    results = []
    try:
        for s in SETTINGS:
            if s is None:
                os.environ.pop(ENV, None)
            else:
                os.environ[ENV] = s
            g.reset()
            call()
            torch.cuda.synchronize()
            bits = g.bits().clone()
            assert g.bands_untouched(), f"{name} [{ENV}={s}]: a guard band was written"
            if written is None:
                assert not bool((bits == SENT).any()), f"{name} [{ENV}={s}]: output elements left unwritten"
            else:
                assert not bool((bits[written] == SENT).any()), f"{name} [{ENV}={s}]: output elements left unwritten"
                assert bool((bits[~written] == SENT).all()), f"{name} [{ENV}={s}]: elements outside the output were written"
            results.append(bits)
    finally:
        if saved is None:
            os.environ.pop(ENV, None)
        else:
            os.environ[ENV] = saved
    for s, b in zip(SETTINGS[:-1], results[:-1]):
        assert torch.equal(b, results[-1]), f"{name}: {ENV}={s} and {ENV}=0 differ in {int((b != results[-1]).sum())} elements"


def conv_fwd(x, sc, sh, wt, b, relu, y, n, h, w, cin, cout, ws=None, ctr=None):
    """goalnet_conv3x3_fwd as the C ABI takes it: without a workspace there is no split-K, i.e. the tile's own epilogue stores y"""
    check(ops.lib().goalnet_conv3x3_fwd(x.data_ptr(), ops._p(sc), ops._p(sh), wt.data_ptr(), ops._p(b), int(relu), y.data_ptr(),
                                        n, h, w, cin, cout, ops._p(ws), 0 if ws is None else ws.numel() * 4, ops._p(ctr),
                                        0 if ctr is None else ctr.numel(), ops._s()), "conv3x3_fwd")


def conv_case(n, h, w, cin, cout, bias, relu, split=None):
    x = rnd(n, h, w, cin, seed=1)
    sc, sh = rnd(cin, seed=2, lo=0.5, hi=1.5), rnd(cin, seed=3, lo=-0.5, hi=0.5)
    wt = rnd(cout, 3, 3, cin, seed=4, lo=-0.05, hi=0.05)
    b = rnd(cout, seed=5) if bias else None
    g = Guarded(n * h * w * cout)
    ws = ctr = None
    if split is not None:
        nbytes = ops.lib().goalnet_conv3x3_fwd_ws_bytes(n, h, w, cin, cout)
        assert nbytes > 0, "this shape was chosen to take split-K"
        ws = torch.empty(nbytes // 4, dtype=torch.float32, device=DEV)
        if split == "fused":
            ctr = torch.zeros(ops.N_TILE_CTR, dtype=torch.int32, device=DEV)
    run_settings(g, lambda: conv_fwd(x, sc, sh, wt, b, relu, g.out, n, h, w, cin, cout, ws, ctr),
                 name=f"conv3x3_fwd {n}x{h}x{w} {cin}->{cout} split={split}")
    if ctr is not None:
        assert not bool(ctr.any()), "the ticket counters are zero again on exit"


@pytest.mark.parametrize("n,h,w", [(1, 1, 1), (1, 1, 127), (1, 3, 43), (3, 5, 7)], ids=["M1", "M127", "M129", "M105"])
def test_ragged_row_tiles(n, h, w):
    conv_case(n, h, w, 32, 128, bias=True, relu=True)


@pytest.mark.parametrize("cout", [4, 68, 132])
def test_ragged_columns(cout):
    conv_case(1, 3, 43, 32, cout, bias=True, relu=True)


@pytest.mark.parametrize("cout", [4, 64])
def test_narrow_tile_without_bias(cout):
    conv_case(1, 3, 43, 32, cout, bias=False, relu=False)


@pytest.mark.parametrize("split", ["plain", "fused"])
@pytest.mark.parametrize("cout", [132, 64])
def test_split_k_slabs(cout, split):
    conv_case(2, 6, 6, 64, cout, bias=True, relu=True, split=split)


@pytest.mark.parametrize("m", [17, 130])
def test_linear_fwd_into_a_column_slice(m):
    k, j, ldy, c0 = 64, 132, 640, 128
    x, wt, b = rnd(m, k, seed=1), rnd(j, k, seed=2, lo=-0.1, hi=0.1), rnd(j, seed=3)
    g = Guarded(m * ldy)
    y = g.out.view(m, ldy)[:, c0:c0 + j]
    written = torch.zeros(m, ldy, dtype=torch.bool, device=DEV)
    written[:, c0:c0 + j] = True
    run_settings(g, lambda: ops.linear_fwd(x, wt, b, y, relu=True), written=written.view(-1), name=f"linear_fwd M={m}")


@pytest.mark.parametrize("k", [4, 132, 260])
@pytest.mark.parametrize("m", [17, 129])
def test_linear_dx_ragged_columns(m, k):
    j, lddx = 32, k + 12
    dy, wt = rnd(m, j, seed=1), rnd(j, k, seed=2, lo=-0.1, hi=0.1)
    g = Guarded(m * lddx)
    dx = g.out.view(m, lddx)[:, :k]
    written = torch.zeros(m, lddx, dtype=torch.bool, device=DEV)
    written[:, :k] = True
    run_settings(g, lambda: ops.linear_bwd_dx(dy, wt, dx), written=written.view(-1), name=f"linear_bwd_dx M={m} K={k}")


def test_linear_dx_leading_dimension_too_wide_for_one_resource():
    """128 rows of lddx = 2^23 + 128 floats span more than 4 GB: the host keeps the old epilogue. Only the written columns and the
    band of columns next to them are touched by the test (the buffer is torch.empty)."""
    m, k, j, lddx = 17, 128, 32, (1 << 23) + 128
    dy, wt = rnd(m, j, seed=1), rnd(j, k, seed=2, lo=-0.1, hi=0.1)
    big = torch.empty(m * lddx, dtype=torch.int32, device=DEV).view(m, lddx)
    dx = big[:, :k].view(torch.float32)
    saved = os.environ.get(ENV)
    results = []
    try:
        for s in SETTINGS:
            if s is None:
                os.environ.pop(ENV, None)
            else:
                os.environ[ENV] = s
            big[:, :2 * k].fill_(SENT)
            ops.linear_bwd_dx(dy, wt, dx)
            torch.cuda.synchronize()
            assert not bool((big[:, :k] == SENT).any()) and bool((big[:, k:2 * k] == SENT).all()), f"{ENV}={s}"
            results.append(big[:, :k].clone())
    finally:
        if saved is None:
            os.environ.pop(ENV, None)
        else:
            os.environ[ENV] = saved
    assert torch.equal(results[0], results[2]) and torch.equal(results[1], results[2])


def test_conv_weight_gradient_slabs():
    n, h, w, cin, cout = 2, 5, 7, 32, 36
    x, dy = rnd(n, h, w, cin, seed=1), rnd(n, h, w, cout, seed=2)
    sc, sh = rnd(cin, seed=3, lo=0.5, hi=1.5), rnd(cin, seed=4, lo=-0.5, hi=0.5)
    g = Guarded(cout * 9 * cin)
    run_settings(g, lambda: ops.conv3x3_wgrad(x, sc, sh, dy, g.out, n, h, w, cin, cout), name="conv3x3_wgrad")
