"""GPU: what include/goalnet_hip.h promises besides values, checked through the raw C ABI (cvml_goalnet_amd._lib).

Every row calls one entry point with each output and each workspace in a guarded view (tests/_abi_guard.py): the workspace is
exactly *_ws_bytes(dims) long, inputs sit between NaN bands. Then: parity with the fp64 restatement and the tolerance of the
kernel's existing test (tests/test_gpu_ops.py: same seeds, same `close`), all bands intact, and, where the entry point takes
ticket counters, counters zero again on exit and a second call on the same counters bit-identical to the first.

tests/_abi_shapes.py holds the shapes and WS_ROWS (per workspace-taking entry point of this file, its *_ws_bytes function and the
dims of its rows); tests/test_abi_contract_host.py asserts on the CPU that the table holds a shape with a non-zero workspace (and, where the
workspace is optional, one with none), so that "exactly ws_bytes" is never vacuous.

The rows: conv1, the fp32 conv3 forward and weight gradient, the fp32 linear layers, the pool / BatchNorm kernels (large: fp32 and
16-bit pooled activations, train and eval; small: with their `ctr`), the 16-bit engine under both GOALNET_BF16_TILE values and in
both formats, the split engine with parts 3 and 2, the fused MLP with `sync`, AudBl's conv1d (with and without the frame-slice
workspace), both heads and the broadcast MSE, the elementwise and reduction helpers and the row copies."""

import ctypes

import pytest
import torch
import torch.nn.functional as F

from _abi_guard import Bands, bits_equal, ptr
from _decisions import saved_mult_check
from cvml_goalnet_amd import _lib, synth
from oracle import avm_ref
from test_gpu_ops import _scale_of, _split_host, close, nchw, nhwc, rnd

pytestmark = pytest.mark.gpu

F32 = torch.float32

from _abi_shapes import (BF16_CONV, BF16_LINEAR_BWD, BF16_LINEAR_FWD, BF16_WGRAD, BN_SMALL, CONV1, CONV1D, CONV_FWD, CONV_FWD_SPLIT,  # noqa: E402
                         CONV_WGRAD, LINEAR_DW, LINEAR_DX, LINEAR_FWD, MLP_ROWS, O16_CONV, O16_LINEAR, POOL, SPLIT_CONV, SPLIT_LINEAR)


from _abi_cases import (_conv_fwd_call, _conv_fwd_case, _conv_wgrad_call, _conv_wgrad_case, _counters_clean, _linear_fwd_call,  # noqa: E402
                        _linear_fwd_case, _ok, _s, _tiles128, _ws)


# ---------------------------------------------------------------------------------------------------------------------------
# conv3x3_fwd
# ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n,h,w,cin,cout,affine,bias,relu", CONV_FWD)
def test_conv3x3_fwd_guarded(n, h, w, cin, cout, affine, bias, relu):
    lib = _lib.load()
    case = _conv_fwd_case(n, h, w, cin, cout, affine, bias, relu)
    for mode in ("null", "ws", "ctr"):              # "null": the unsplit store path, what a caller without a workspace gets
        bands = Bands()
        y, ctr, call = _conv_fwd_call(lib, bands, case, (n, h, w, cin, cout), relu, mode)
        close(f"conv3x3_fwd[{n}x{h}x{w}x{cin}->{cout}] {mode}", y, case[5], rtol=5e-6)
        bands.assert_bands_intact()
        if ctr is not None:
            _counters_clean(ctr, "conv3x3_fwd")
            first = y.clone()
            y.fill_(float("nan"))
            call()
            assert bits_equal(y, first), "second call on the same counters differs"
            _counters_clean(ctr, "conv3x3_fwd, second call")
            bands.assert_bands_intact()


def test_conv3x3_fwd_split_k_three_ways():
    """ten 11 x 11 frames, 256 -> 512 channels: split-K. ws = NULL (no split), ws (two launches), ws + tile_ctr (fused: the last
    block of a tile sums its slabs) — the header: "same bits as the two-launch form"."""
    lib = _lib.load()
    n, h, w, cin, cout, affine, bias, relu = CONV_FWD_SPLIT
    dims = (n, h, w, cin, cout)
    assert lib.goalnet_conv3x3_fwd_ws_bytes(*dims) > 0
    case = _conv_fwd_case(*CONV_FWD_SPLIT)
    got = {}
    for mode in ("null", "ws", "ctr"):
        bands = Bands()
        y, ctr, call = _conv_fwd_call(lib, bands, case, dims, relu, mode)
        close(f"conv3x3_fwd split-K, {mode}", y, case[5], rtol=5e-6)
        bands.assert_bands_intact()
        got[mode] = y.clone()
        if ctr is not None:
            _counters_clean(ctr, "conv3x3_fwd fused split-K")
            y.fill_(float("nan"))
            call()
            assert bits_equal(y, got[mode]), "second call on the same counters differs"
            _counters_clean(ctr, "conv3x3_fwd fused split-K, second call")
            bands.assert_bands_intact()
    assert bits_equal(got["ws"], got["ctr"]), "fused split-K reduction differs from the two-launch form"


# ---------------------------------------------------------------------------------------------------------------------------
# conv3x3_wgrad
# ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("path", ["select", "correct"])
@pytest.mark.parametrize("n,h,w,cin,cout,affine", CONV_WGRAD)
def test_conv3x3_wgrad_guarded(n, h, w, cin, cout, affine, path, monkeypatch):
    """With counters the reduction is fused where no border correction is pending ('select', or no affine) and must then give the
    bits of the two-launch form; elsewhere the counters are not used, so the results are the same launches: identical either way."""
    monkeypatch.setenv("GOALNET_WGRAD_PATH", path)
    lib = _lib.load()
    case = _conv_wgrad_case(n, h, w, cin, cout, affine)
    ref = case[4]
    got = {}
    for mode in ("ws", "ctr", "nocodes"):
        bands = Bands()
        dw, ctr, call = _conv_wgrad_call(lib, bands, case, (n, h, w, cin, cout), mode)
        close(f"conv3x3_wgrad[{n}x{h}x{w}x{cin}->{cout}] {path} {mode}", dw, ref, rtol=5e-6)
        bands.assert_bands_intact()
        got[mode] = dw.clone()
        if ctr is not None:
            _counters_clean(ctr, "conv3x3_wgrad")
            dw.fill_(float("nan"))
            call()
            assert bits_equal(dw, got[mode]), "second call on the same counters differs"
            _counters_clean(ctr, "conv3x3_wgrad, second call")
            bands.assert_bands_intact()
    assert bits_equal(got["ws"], got["ctr"]), "with ticket counters the weight gradient differs from the two-launch form"
    assert bits_equal(got["ws"], got["nocodes"]), "the caller's code table and the one built inside ws give different results"


# ---------------------------------------------------------------------------------------------------------------------------
# linear layers
# ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("m,k,j,affine,mask,ldextra", LINEAR_FWD)
def test_linear_fwd_guarded(m, k, j, affine, mask, ldextra):
    lib = _lib.load()
    case = _linear_fwd_case(m, k, j, affine, mask)
    dm, pre, ref = case[5:]
    bands = Bands()
    y, mult, _ = _linear_fwd_call(lib, bands, case, (m, k, j), ldextra)
    close(f"linear_fwd[{m}x{k}->{j}]", y, ref, rtol=3e-6)
    want_mult = (pre > 0).double() * (dm.double() if mask else 1.0)
    safe = pre.abs() > 1e-4
    assert torch.equal(mult.cpu().double()[safe], want_mult[safe])
    bands.assert_bands_intact()


@pytest.mark.parametrize("m,k,j,use_mult", LINEAR_DX)
def test_linear_bwd_dx_guarded(m, k, j, use_mult):
    lib = _lib.load()
    dy = rnd(m, j, seed=28)
    w = rnd(j, k, seed=29, lo=-0.05, hi=0.05)
    mult = (torch.rand(m, k, generator=torch.Generator().manual_seed(30)) >= 0.5).float() * 1.25 if use_mult else None
    ref = dy.double() @ w.double()
    if use_mult:
        ref = ref * mult.double()
    bands = Bands()
    dyg, wg = bands.place(dy, "dy"), bands.place(w, "w")
    mg = None if mult is None else bands.place(mult, "mult")
    dx = bands.guarded_rows(m, k, k + 8, F32, name="dx")
    _ok(lib.goalnet_linear_bwd_dx(ptr(dyg), j, ptr(wg), ptr(mg), k, ptr(dx), k + 8, m, k, j, _s()), "linear_bwd_dx")
    close(f"linear_bwd_dx[{m}x{j}->{k}]", dx, ref, rtol=3e-6)
    bands.assert_bands_intact()


@pytest.mark.parametrize("m,k,j,affine", LINEAR_DW)
def test_linear_bwd_dw_guarded(m, k, j, affine):
    lib = _lib.load()
    dy = rnd(m, j, seed=31)
    x = rnd(m, k, seed=32)
    ref = dy.double().t() @ x.double()
    bands = Bands()
    dyg, xg = bands.place(dy, "dy"), bands.place(x, "x")
    dw = bands.guarded((j, k), F32, name="dw")
    db = bands.guarded(j, F32, name="db")
    _ok(lib.goalnet_linear_bwd_dw(ptr(dyg), j, ptr(xg), k, 0, 0, 0, ptr(dw), ptr(db), m, k, j, _s()), "linear_bwd_dw")
    close(f"linear_bwd_dw[{m}: {j}x{k}]", dw, ref, rtol=3e-6)
    close("linear_bwd_dw.db", db, dy.double().sum(0), rtol=1e-6)
    bands.assert_bands_intact()


# ---------------------------------------------------------------------------------------------------------------------------
# the small elementwise / reduction entry points
# ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("m,j,lds", [(7, 37, (40, 48, 44)), (130, 512, (516, 512, 640)), (1, 1, (1, 1, 1))])
def test_mul_guarded_bit_exact(m, j, lds):
    """y = x * mult over [M][J] with three different leading dimensions: one fp32 multiply per element, so torch's fp32 product is
    the exact answer; the gaps between the rows of y are bands"""
    lib = _lib.load()
    x, mu = rnd(m, j, seed=70, lo=-3, hi=3), rnd(m, j, seed=71, lo=-3, hi=3)
    bands = Bands()
    xg, mg = bands.place_rows(x, lds[0], "x"), bands.place_rows(mu, lds[1], "mult")
    y = bands.guarded_rows(m, j, lds[2], F32, name="y")
    _ok(lib.goalnet_mul(ptr(xg), lds[0], ptr(mg), lds[1], ptr(y), lds[2], m, j, _s()), "mul")
    assert bits_equal(y.cpu(), x * mu)
    bands.assert_bands_intact()


@pytest.mark.parametrize("m,j,ld", [(13, 70, 76), (16, 36, 36), (300, 33, 40)])
def test_colsum_guarded(m, j, ld):
    lib = _lib.load()
    x = rnd(m, j, seed=72)
    bands = Bands()
    xg = bands.place_rows(x, ld, "x")
    out = bands.guarded(j, F32, name="out")
    _ok(lib.goalnet_colsum(ptr(xg), ld, m, j, ptr(out), _s()), "colsum")
    close("colsum", out, x.double().sum(0), rtol=1e-6)          # tolerance of test_linear_bwd_dw's colsum check
    bands.assert_bands_intact()


@pytest.mark.parametrize("n", [1, 1003, 8192 * 256 + 77])           # the last: more elements than the largest grid has threads
def test_scale_guarded_bit_exact(n):
    """x *= s: one fp32 multiply per element, torch's fp32 product is the exact answer"""
    lib = _lib.load()
    x = rnd(n, seed=73, lo=-100, hi=100)
    bands = Bands()
    xg = bands.place(x, "x")
    _ok(lib.goalnet_scale(ptr(xg), n, 0.3, _s()), "scale")
    assert bits_equal(xg.cpu(), x * torch.tensor(0.3, dtype=F32))
    bands.assert_bands_intact()


@pytest.mark.parametrize("n", [1, 1003, 4096 * 256 + 5])
def test_relu_bwd_guarded(n):
    """dz = dy * (y > 0): exact by construction (a product with 0 or 1; the sign of a zero is not pinned)"""
    lib = _lib.load()
    dy, y = rnd(n, seed=74), F.relu(rnd(n, seed=75))
    bands = Bands()
    dyg, yg = bands.place(dy, "dy"), bands.place(y, "y")
    dz = bands.guarded(n, F32, name="dz")
    _ok(lib.goalnet_relu_bwd(ptr(dyg), ptr(yg), ptr(dz), n, _s()), "relu_bwd")
    assert torch.equal(dz.cpu(), dy * (y > 0))
    bands.assert_bands_intact()


@pytest.mark.parametrize("nparts,c,stride", [(1024, 70, 96), (5, 512, 512), (1, 3, 3)])
def test_partials_sums_guarded(nparts, c, stride):
    """out[c] = sum over parts of partials[part][c]. partials_sum_f64 against the exactly rounded sum (math.fsum) to 1e-15 relative, the
    reorder bound of at most 1024 rows; the fp32-output forms add one rounding of the double sum to float (2^-24 relative)."""
    import math
    lib = _lib.load()
    pa = rnd(nparts, c, seed=76).double() * 1.000000123          # not fp32-representable: all 53 bits in play
    want = torch.tensor([math.fsum(pa[:, k].tolist()) for k in range(c)], dtype=torch.float64)
    bands = Bands()
    pg = bands.place_rows(pa, stride, "partials")
    o64 = bands.guarded(c, torch.float64, name="out64")
    _ok(lib.goalnet_partials_sum_f64(ptr(pg), nparts, stride, c, ptr(o64), _s()), "partials_sum_f64")
    close("partials_sum_f64", o64, want, rtol=1e-15)
    o32 = bands.guarded(c, F32, name="out32")
    _ok(lib.goalnet_partials_sum(ptr(pg), nparts, stride, c, ptr(o32), _s()), "partials_sum")
    close("partials_sum", o32, want, rtol=2.0 ** -24 + 1e-15)
    # two arrays in one launch (contiguous rows)
    pb = rnd(7, 33, seed=77).double() / 3.0
    pac, pbc = bands.place(pa, "pa"), bands.place(pb, "pb")
    oa, ob = bands.guarded(c, F32, name="oa"), bands.guarded(33, F32, name="ob")
    _ok(lib.goalnet_partials_sum2(ptr(pac), nparts, c, ptr(oa), ptr(pbc), 7, 33, ptr(ob), _s()), "partials_sum2")
    close("partials_sum2.a", oa, want, rtol=2.0 ** -24 + 1e-15)
    close("partials_sum2.b", ob, torch.tensor([math.fsum(pb[:, k].tolist()) for k in range(33)], dtype=torch.float64), rtol=2.0 ** -24 + 1e-15)
    bands.assert_bands_intact()


# ---------------------------------------------------------------------------------------------------------------------------
# row gathers / scatters around a device cursor: table rows before and behind the window keep their bits
# ---------------------------------------------------------------------------------------------------------------------------
ROWS, RW = 20, 6


def _table():
    return torch.arange(ROWS * RW, dtype=F32).view(ROWS, RW) + 0.5


@pytest.mark.parametrize("cursor,nrows", [(0, 1), (5, 3), (17, 3)])
def test_rows_gather_and_scatter_guarded(cursor, nrows):
    lib = _lib.load()
    bands = Bands()
    table = bands.place(_table(), "table")
    cur = torch.tensor([cursor], dtype=torch.int64, device="cuda")
    block = bands.guarded((nrows, RW), F32, name="block")
    _ok(lib.goalnet_rows_gather(ptr(table), ptr(block), RW * 4, nrows, ptr(cur), _s()), "rows_gather")
    assert bits_equal(block.cpu(), _table()[cursor:cursor + nrows]) and bits_equal(table.cpu(), _table())
    src = bands.place(-rnd(nrows, RW, seed=78) - 2.0, "src")
    _ok(lib.goalnet_rows_scatter(ptr(src), ptr(table), RW * 4, nrows, ptr(cur), _s()), "rows_scatter")
    want = _table()
    want[cursor:cursor + nrows] = src.cpu()
    assert bits_equal(table.cpu(), want), "rows outside [cursor, cursor + nrows) changed"
    bands.assert_bands_intact()


@pytest.mark.parametrize("tick", [False, True], ids=["rows_copy_batch", "rows_scatter_tick"])
def test_rows_copy_batch_and_tick_guarded(tick):
    """one gather and one scatter segment with cursor biases; rows_scatter_tick then advances the four counters, after the copies"""
    lib = _lib.load()
    bands = Bands()
    table_a, table_b = bands.place(_table(), "table_a"), bands.place(-_table(), "table_b")
    counters = bands.guarded(4, torch.int64, fill=torch.tensor([3, 9, 4, 1]), name="counters")
    block = bands.guarded((2, RW), F32, name="block")
    src = bands.place(rnd(3, RW, seed=79) + 100.0, "src")
    segs = (_lib.RowCopy * 2)(
        _lib.RowCopy(ptr(table_a), ptr(block), RW * 4, 2, 1, ptr(counters[2:3]), 2),        # gather rows [4 + 2, 4 + 2 + 2) of table_a
        _lib.RowCopy(ptr(src), ptr(table_b), RW * 4, 3, 0, ptr(counters[3:4]), 0))          # scatter to rows [1, 4) of table_b
    if tick:
        _ok(lib.goalnet_rows_scatter_tick(segs, 2, ptr(counters), 1, 2, 10, 1, None, _s()), "rows_scatter_tick")
        assert counters.tolist() == [4, 11, 14, 2]
    else:
        _ok(lib.goalnet_rows_copy_batch(segs, 2, _s()), "rows_copy_batch")
        assert counters.tolist() == [3, 9, 4, 1]
    assert bits_equal(block.cpu(), _table()[6:8]) and bits_equal(table_a.cpu(), _table())
    want = -_table()
    want[1:4] = src.cpu()
    assert bits_equal(table_b.cpu(), want), "rows outside the scattered window changed"
    bands.assert_bands_intact()


# ---------------------------------------------------------------------------------------------------------------------------
# the small pool / BatchNorm launches: ws of goalnet_bn_small_ws_bytes(C), ctr zero on entry and zero again on exit
# ---------------------------------------------------------------------------------------------------------------------------
def _twice(call, outs, ctr, what, bands):
    """the counter contract: zero after the call; a second call on the same counters gives the same bits and leaves them zero"""
    call()
    _counters_clean(ctr, what)
    first = [t.clone() for t in outs]
    for t in outs:
        t.view(torch.uint8).fill_(0xA5) if t.dtype == torch.uint8 else t.fill_(float("nan"))
    call()
    _counters_clean(ctr, what + ", second call")
    for a, b in zip(outs, first):
        assert bits_equal(a, b), f"{what}: second call on the same counters differs"
    bands.assert_bands_intact()


@pytest.mark.parametrize("n,hc,wc,c", BN_SMALL)
def test_small_pool_batchnorm_guarded(n, hc, wc, c):
    """references and tolerances of test_small_pool_batchnorm_forward_and_backward_vs_fp64 (tests/test_gpu_small.py) and, for the
    eval-mode reduce, of tests/test_gpu_eval.py (dgamma, dbeta as the train-mode ones; coef3 = (gamma invstd, 0, 0) to 1e-6)"""
    from cvml_goalnet_amd import ops
    lib = _lib.load()
    z = rnd(n, hc, wc, c, seed=16)
    y = F.relu(z)
    gamma, beta = rnd(c, seed=17, lo=0.5, hi=1.5), rnd(c, seed=18, lo=-0.5, hi=0.5)
    rm0, rv0 = rnd(c, seed=19), rnd(c, seed=20, lo=0.5, hi=2.0)
    zd = nchw(z.double()).requires_grad_(True)
    pd, pidx = F.max_pool2d(F.relu(zd), 3, 1, 0, return_indices=True)
    rm, rv = rm0.double().clone(), rv0.double().clone()
    gd, bd = gamma.double().requires_grad_(True), beta.double().requires_grad_(True)
    od = F.batch_norm(pd, rm, rv, gd, bd, training=True, momentum=0.1, eps=1e-5)
    G = rnd(*od.shape, seed=21).double()
    (od * G).sum().backward()
    hp, wp = hc - 2, wc - 2
    nbytes = lib.goalnet_bn_small_ws_bytes(c)
    assert nbytes > 0
    bands = Bands()
    yg, gg, bg = bands.place(y, "y"), bands.place(gamma, "gamma"), bands.place(beta, "beta")
    p = bands.guarded((n, hp, wp, c), F32, name="p")
    idx = bands.guarded(n * hp * wp * c, torch.uint8, name="idx")
    rmg, rvg = bands.guarded(c, F32, fill=rm0, name="running_mean"), bands.guarded(c, F32, fill=rv0, name="running_var")
    st = [bands.guarded(c, F32, name=nm) for nm in ("mean", "invstd", "scale", "shift")]
    ws = _ws(bands, nbytes)
    ctr = bands.guarded(1, torch.int32, fill=0, name="ctr")

    def fwd():
        rmg.copy_(rm0), rvg.copy_(rv0)
        _ok(lib.goalnet_pool_bn_fwd_small(ptr(yg), ptr(p), ptr(idx), ptr(gg), ptr(bg), ptr(rmg), ptr(rvg), 0.1, 1e-5, *(ptr(t) for t in st),
                                          ptr(ws), nbytes, ptr(ctr), n, hc, wc, c, _s()), "pool_bn_fwd_small")
    _twice(fwd, [p, idx, rmg, rvg] + st, ctr, "pool_bn_fwd_small", bands)
    close("maxpool", p, nhwc(pd), rtol=0.0)
    ih, iw = pidx // wc, pidx % wc
    tap = ((ih - torch.arange(hp).view(1, 1, hp, 1)) * 3 + (iw - torch.arange(wp).view(1, 1, 1, wp))).to(torch.uint8)
    assert torch.equal(ops.idx_to_nhwc(idx, n, hp, wp, c).cpu(), nhwc(tap)), "argmax positions differ from ATen's"
    close("bn.mean", st[0], pd.mean(dim=(0, 2, 3)), rtol=1e-6)
    close("bn.invstd", st[1], 1.0 / torch.sqrt(pd.var(dim=(0, 2, 3), unbiased=False) + 1e-5), rtol=1e-6)
    close("bn.running_mean", rmg, rm, rtol=1e-6)
    close("bn.running_var", rvg, rv, rtol=1e-6)
    close("bn.apply(scale,shift)", p * st[2] + st[3], nhwc(od), rtol=2e-6)
    # ---- backward: reduce + finalise, then max-pool / ReLU backward + bias gradient
    dbn = bands.place(nhwc(G.float()), "dz")
    dgamma, dbeta, coef3 = bands.guarded(c, F32, name="dgamma"), bands.guarded(c, F32, name="dbeta"), bands.guarded(3 * c, F32, name="coef3")
    _twice(lambda: _ok(lib.goalnet_bn_bwd_reduce_small(ptr(dbn), ptr(p), ptr(st[0]), ptr(st[1]), ptr(gg), ptr(dgamma), ptr(dbeta), ptr(coef3), ptr(ws),
                                                       nbytes, ptr(ctr), n, hc, wc, c, _s()), "bn_bwd_reduce_small"),
           [dgamma, dbeta, coef3], ctr, "bn_bwd_reduce_small", bands)
    close("bn.dgamma", dgamma, gd.grad, rtol=5e-6)
    close("bn.dbeta", dbeta, bd.grad, rtol=5e-6)
    dy, dbias = bands.guarded((n, hc, wc, c), F32, name="dy"), bands.guarded(c, F32, name="dbias")
    _twice(lambda: _ok(lib.goalnet_bnpool_bwd_small(ptr(dbn), ptr(p), ptr(idx), ptr(coef3), ptr(dy), ptr(dbias), ptr(ws), nbytes, ptr(ctr),
                                                    n, hc, wc, c, _s()), "bnpool_bwd_small"), [dy, dbias], ctr, "bnpool_bwd_small", bands)
    close("block.dz (bn+pool+relu bwd)", dy, nhwc(zd.grad), rtol=1e-5)
    close("block.dbias", dbias, zd.grad.sum(dim=(0, 2, 3)), rtol=0.0, atol=3e-6 * zd.grad.abs().max().item() * (n * hc * wc) ** 0.5)
    # ---- eval mode: mean / invstd are constants (the running statistics)
    mean_e, invstd_e = rnd(c, seed=19), 1.0 / torch.sqrt(rnd(c, seed=20, lo=0.5, hi=2.0) + 1e-5)
    me, ie = bands.place(mean_e, "mean_eval"), bands.place(invstd_e, "invstd_eval")
    dg_e, db_e, c3_e = bands.guarded(c, F32, name="dgamma_e"), bands.guarded(c, F32, name="dbeta_e"), bands.guarded(3 * c, F32, name="coef3_e")
    _twice(lambda: _ok(lib.goalnet_bn_bwd_reduce_small_eval(ptr(dbn), ptr(p), ptr(me), ptr(ie), ptr(gg), ptr(dg_e), ptr(db_e), ptr(c3_e), ptr(ws),
                                                            nbytes, ptr(ctr), n, hc, wc, c, _s()), "bn_bwd_reduce_small_eval"),
           [dg_e, db_e, c3_e], ctr, "bn_bwd_reduce_small_eval", bands)
    Gp, pp = nhwc(G), nhwc(pd.detach())
    xhat = (pp - mean_e.double()) * invstd_e.double()
    close("eval.dgamma", dg_e, (Gp * xhat).sum(dim=(0, 1, 2)), rtol=5e-6)
    close("eval.dbeta", db_e, Gp.sum(dim=(0, 1, 2)), rtol=5e-6)
    assert torch.allclose(c3_e[:c].cpu().double(), gamma.double() * invstd_e.double(), rtol=1e-6, atol=0)
    assert torch.count_nonzero(c3_e[c:]).item() == 0


# ---------------------------------------------------------------------------------------------------------------------------
# the fused MLP: sync int32[3] zero on entry, zero again on exit ([2] included: no barrier timed out); ws of goalnet_mlp_bwd_ws_bytes(n)
# ---------------------------------------------------------------------------------------------------------------------------
MLP_WIDTHS = (512, 512, 256, 128)


def _host_ptrs(ts):
    return (ctypes.c_void_p * len(ts))(*[None if t is None else t.data_ptr() for t in ts])


@pytest.mark.parametrize("n,k0,use_masks", MLP_ROWS)
def test_fused_mlp_guarded(n, k0, use_masks):
    """inputs, fp64 autograd oracle and tolerances of test_fused_mlp_forward_and_backward_vs_fp64 (tests/test_gpu_small.py)"""
    lib = _lib.load()
    g = torch.Generator().manual_seed(100 + n)
    dims = [k0] + list(MLP_WIDTHS) + [1]
    wsd = [((torch.rand(dims[l + 1], dims[l], generator=g, dtype=torch.float64) - 0.5) * 2 / dims[l] ** 0.5) for l in range(5)]
    bsd = [((torch.rand(dims[l + 1], generator=g, dtype=torch.float64) - 0.5) * 0.2) for l in range(5)]
    wide = torch.rand(n, k0 + 64, generator=g, dtype=torch.float64) - 0.3
    masks = [((torch.rand(n, w, generator=g) >= 0.2).double() * 1.25) if use_masks else None for w in MLP_WIDTHS]
    labels = torch.randint(1, 6, (n,), generator=g).double()
    wd = [w.clone().requires_grad_(True) for w in wsd]
    bd = [b.clone().requires_grad_(True) for b in bsd]
    x0 = wide[:, 32:32 + k0].clone().requires_grad_(True)
    x, hs = x0, []
    for l in range(4):
        x = F.relu(F.linear(x, wd[l], bd[l]))
        if masks[l] is not None:
            x = x * masks[l]
        hs.append(x)
    z = F.linear(x, wd[4], bd[4]).view(-1)
    out = 4 * torch.sigmoid(z) + 1
    d = out.view(n, 1) - labels.view(1, n)
    loss = (d * d).mean()
    loss.backward()
    # ---- device: cat is a column slice of a wider guarded buffer, so the columns beside it are NaN
    bands = Bands()
    ld = k0 + 64
    cat = bands.place_rows(wide[:, 32:32 + k0].float(), ld, "cat")
    wg, bg = [bands.place(w.float(), f"w{l}") for l, w in enumerate(wsd)], [bands.place(b.float(), f"b{l}") for l, b in enumerate(bsd)]
    mg = [None if m is None else bands.place(m.float(), f"mask{l}") for l, m in enumerate(masks)]
    hg = [bands.guarded((n, w), F32, name=f"h{l + 1}") for l, w in enumerate(MLP_WIDTHS)]
    mult = [bands.guarded((n, w), F32, name=f"mult{l + 1}") for l, w in enumerate(MLP_WIDTHS)]
    logit, og = bands.guarded(n, F32, name="logit"), bands.guarded(n, F32, name="out")
    lossg, dout = bands.guarded(1, F32, name="loss"), bands.guarded(n, F32, name="dout")
    lab = bands.place(labels.float(), "labels")
    sync = bands.guarded(3, torch.int32, fill=0, name="sync")
    ldm = (ctypes.c_int64 * 4)(*[0 if m is None else w for m, w in zip(mg, MLP_WIDTHS)])
    _twice(lambda: _ok(lib.goalnet_mlp_fwd(ptr(cat), ld, k0, _host_ptrs(wg), _host_ptrs(bg), _host_ptrs(mg), ldm, _host_ptrs(hg), _host_ptrs(mult),
                                           ptr(logit), ptr(og), ptr(lab), ptr(lossg), ptr(dout), n, ptr(sync), _s()), "mlp_fwd"),
           hg + mult + [logit, og, lossg, dout], sync, "mlp_fwd", bands)
    for l in range(4):
        close(f"mlp.h{l + 1}", hg[l], hs[l], rtol=3e-6)
        want_mult = (hs[l] != 0).double() * (masks[l] if masks[l] is not None else 1.0)
        assert ((mult[l].cpu().double() - want_mult).abs() > 1e-6).sum().item() <= 2, f"saved multipliers of layer {l}"
    close("mlp.logit", logit, z, rtol=3e-6)
    close("mlp.out", og, out, rtol=3e-6)
    close("mlp.loss", lossg, loss.view(1), rtol=3e-6, atol=2e-7)
    close("mlp.dout", dout, (2.0 / n) * (out.detach() - labels.mean()), rtol=3e-6, atol=2e-7)
    # ---- backward
    mcat = bands.place_rows(torch.ones(n, k0), ld, "mcat")
    dws = [bands.guarded(tuple(w.shape), F32, name=f"dw{l}") for l, w in enumerate(wsd)]
    dbs = [bands.guarded(tuple(b.shape), F32, name=f"db{l}") for l, b in enumerate(bsd)]
    dcat = bands.guarded((n, k0), F32, name="dcat")
    db5 = bands.guarded(512, F32, name="db5")
    nbytes = lib.goalnet_mlp_bwd_ws_bytes(n)
    wsb = _ws(bands, nbytes)
    _twice(lambda: _ok(lib.goalnet_mlp_bwd(ptr(dout), ptr(og), _host_ptrs([cat] + hg), ld, _host_ptrs([mcat] + mult), ld, _host_ptrs(wg), _host_ptrs(dws),
                                           _host_ptrs(dbs), ptr(dcat), k0, ptr(db5), k0 - 512, n, k0, ptr(wsb), nbytes, ptr(sync), _s()), "mlp_bwd"),
           dws + dbs + [dcat, db5], sync, "mlp_bwd", bands)
    for l in range(5):
        close(f"mlp.dw{l}", dws[l], wd[l].grad, rtol=1e-5)
        close(f"mlp.db{l}", dbs[l], bd[l].grad, rtol=1e-5, atol=1e-9)
    close("mlp.dcat", dcat, x0.grad, rtol=1e-5)
    close("mlp.db5 (column sums of dcat[:, voff:])", db5, x0.grad[:, k0 - 512:].sum(0), rtol=1e-5, atol=1e-9)


# ---------------------------------------------------------------------------------------------------------------------------
# AudBl conv1d: the optional frame-slice workspace (>= 512 frames), the many-frame kernels without it, the one-launch form
# ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n,bins", CONV1D)
def test_audbl_conv1d_guarded(n, bins):
    """the two layers of test_audbl_conv1d (tests/test_gpu_ops.py), its oracle and tolerances; n < 64 goes through
    goalnet_conv1d_bwd_small (ReLU backward folded in), as test_conv1d_backward_in_one_launch_equals_the_multi_launch_form"""
    lib = _lib.load()
    x = rnd(n, 30, bins, seed=35, lo=-50, hi=50)
    w1, b1 = rnd(64, 30, 3, seed=36, lo=-0.1, hi=0.1), rnd(64, seed=37)
    w2, b2 = rnd(128, 64, 3, seed=38, lo=-0.07, hi=0.07), rnd(128, seed=39)
    w1d, b1d, w2d, b2d = (t.double().requires_grad_(True) for t in (w1, b1, w2, b2))
    a1 = F.relu(F.conv1d(x.double(), w1d, b1d, stride=2, padding=1))
    a2 = F.relu(F.conv1d(a1, w2d, b2d, stride=2, padding=1))
    G = rnd(*a2.shape, seed=40).double()
    (a2 * G).sum().backward()
    l1, l2 = a1.shape[2], a2.shape[2]
    bands = Bands()
    xg, w1g, b1g, w2g, b2g = (bands.place(t, nm) for t, nm in ((x, "x"), (w1, "w1"), (b1, "b1"), (w2, "w2"), (b2, "b2")))
    g1, g2 = bands.guarded((n, 64, l1), F32, name="a1"), bands.guarded((n, 128, l2), F32, name="a2")
    _ok(lib.goalnet_conv1d_fwd(ptr(xg), ptr(w1g), ptr(b1g), 1, ptr(g1), n, 30, bins, 64, 2, 1, _s()), "conv1d_fwd")
    _ok(lib.goalnet_conv1d_fwd(ptr(g1), ptr(w2g), ptr(b2g), 1, ptr(g2), n, 64, l1, 128, 2, 1, _s()), "conv1d_fwd")
    close("audbl.conv1", g1, a1, rtol=3e-6); close("audbl.conv2", g2, a2, rtol=3e-6)
    Gg = bands.place(G.float(), "G")
    da1 = bands.guarded((n, 64, l1), F32, name="da1")
    dw2, db2 = bands.guarded((128, 64, 3), F32, name="dw2"), bands.guarded(128, F32, name="db2")
    dw1, db1 = bands.guarded((64, 30, 3), F32, name="dw1"), bands.guarded(64, F32, name="db1")
    if n < 64:
        _ok(lib.goalnet_conv1d_bwd_small(ptr(g1), ptr(Gg), ptr(g2), ptr(w2g), ptr(da1), ptr(dw2), ptr(db2), n, 64, l1, 128, 2, 1, _s()), "conv1d_bwd_small")
        _ok(lib.goalnet_conv1d_bwd_small(ptr(xg), ptr(da1), ptr(g1), ptr(w1g), 0, ptr(dw1), ptr(db1), n, 30, bins, 64, 2, 1, _s()), "conv1d_bwd_small")
    else:
        dz2 = bands.guarded((n, 128, l2), F32, name="dz2")
        _ok(lib.goalnet_relu_bwd(ptr(Gg), ptr(g2), ptr(dz2), dz2.numel(), _s()), "relu_bwd")
        nb2, nb1 = lib.goalnet_conv1d_bwd_ws_bytes(n, 64, 128), lib.goalnet_conv1d_bwd_ws_bytes(n, 30, 64)
        assert (nb2 > 0) == (n >= 512) and (nb1 > 0) == (n >= 512)
        ws2, ws1 = _ws(bands, nb2), _ws(bands, nb1)
        _ok(lib.goalnet_conv1d_bwd(ptr(g1), ptr(dz2), ptr(w2g), ptr(da1), ptr(dw2), ptr(db2), n, 64, l1, 128, 2, 1, ptr(ws2), nb2, _s()), "conv1d_bwd")
        _ok(lib.goalnet_relu_bwd(ptr(da1), ptr(g1), ptr(da1), da1.numel(), _s()), "relu_bwd")
        _ok(lib.goalnet_conv1d_bwd(ptr(xg), ptr(da1), ptr(w1g), 0, ptr(dw1), ptr(db1), n, 30, bins, 64, 2, 1, ptr(ws1), nb1, _s()), "conv1d_bwd")
    close("audbl.dw2", dw2, w2d.grad, rtol=1e-5); close("audbl.db2", db2, b2d.grad, rtol=1e-5)
    close("audbl.dw1", dw1, w1d.grad, rtol=1e-5); close("audbl.db1", db1, b1d.grad, rtol=1e-5)
    bands.assert_bands_intact()


# ---------------------------------------------------------------------------------------------------------------------------
# head (fusion.12 + Sigmoid + 4y + 1) and the broadcast MSE
# ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [1, 10, 300])
def test_head_and_mse_guarded(n):
    """test_head_and_mse (tests/test_gpu_ops.py) with every buffer guarded and h, mult, dh on a leading dimension above K"""
    lib = _lib.load()
    h, w, b = rnd(n, 128, seed=41), rnd(128, seed=42, lo=-0.1, hi=0.1), rnd(1, seed=43)
    lab = torch.from_numpy(synth.make_labels(n))            # the labels of test_head_and_mse: its tolerance is worked out for them
    mult = (torch.rand(n, 128, generator=torch.Generator().manual_seed(44)) >= 0.2).float() * 1.25
    hd, wd, bd = h.double().requires_grad_(True), w.double().requires_grad_(True), b.double().requires_grad_(True)
    z = hd @ wd + bd
    out = 4 * torch.sigmoid(z) + 1
    loss = avm_ref.mse_bcast(out.view(n, 1), lab.double())
    loss.backward()
    bands = Bands()
    hg, wg, bg, labg = bands.place_rows(h, 132, "h"), bands.place(w, "w"), bands.place(b, "b"), bands.place(lab, "labels")
    mg = bands.place_rows(mult, 136, "mult")
    logit, og = bands.guarded(n, F32, name="logit"), bands.guarded(n, F32, name="out")
    _ok(lib.goalnet_head_fwd(ptr(hg), 132, ptr(wg), ptr(bg), ptr(logit), ptr(og), n, 128, _s()), "head_fwd")
    close("head.logit", logit, z, rtol=2e-6, atol=2e-7); close("head.out", og, out, rtol=1e-6)
    lg, dpred = bands.guarded(1, F32, name="loss"), bands.guarded(n, F32, name="dpred")
    _ok(lib.goalnet_mse_bcast(ptr(og), ptr(labg), n, ptr(lg), ptr(dpred), _s()), "mse_bcast")
    close("mse_bcast.loss", lg, loss.detach().view(1), rtol=2e-6)
    dh = bands.guarded_rows(n, 128, 140, F32, name="dh")
    dw, db = bands.guarded(128, F32, name="dw"), bands.guarded(1, F32, name="db")
    _ok(lib.goalnet_head_bwd(ptr(dpred), ptr(og), ptr(hg), 132, ptr(wg), ptr(mg), 136, ptr(dh), 140, ptr(dw), ptr(db), n, 128, _s()), "head_bwd")
    close("head.dh", dh, hd.grad * mult.double(), rtol=5e-6)
    close("head.dw", dw, wd.grad, rtol=5e-6); close("head.db", db, bd.grad.view(1), rtol=5e-6)
    bands.assert_bands_intact()


# ---------------------------------------------------------------------------------------------------------------------------
# conv1 (3 -> 64, k3 s3 p3): forward and weight gradient, ws of goalnet_conv1_wgrad_ws_bytes
# ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n,h,w", CONV1)
def test_conv1_guarded(n, h, w):
    """inputs, oracle and tolerances of test_conv1_fwd_and_wgrad (tests/test_gpu_ops.py)"""
    lib = _lib.load()
    x = rnd(n, 3, h, w, seed=3, lo=0, hi=1)
    wt = rnd(64, 3, 3, 3, seed=4, lo=-0.2, hi=0.2)       # OIHW
    b = rnd(64, seed=5, lo=-0.2, hi=0.2)
    wd, bd = wt.double().requires_grad_(True), b.double().requires_grad_(True)
    out = F.conv2d(x.double(), wd, bd, stride=3, padding=3)
    ho, wo = out.shape[2], out.shape[3]
    dy = rnd(n, ho, wo, 64, seed=6)
    out.backward(nchw(dy).double())
    bands = Bands()
    xg, wg, bg = bands.place(x, "x"), bands.place(wt.permute(0, 2, 3, 1).contiguous(), "w"), bands.place(b, "bias")
    y = bands.guarded((n, ho, wo, 64), F32, name="y")
    _ok(lib.goalnet_conv1_fwd(ptr(xg), ptr(wg), ptr(bg), ptr(y), n, h, w, _s()), "conv1_fwd")
    close("conv1_fwd", y, nhwc(F.relu(out.detach())))
    dyg = bands.place(dy, "dy")
    dw, db = bands.guarded((64, 3, 3, 3), F32, name="dw"), bands.guarded(64, F32, name="db")
    nbytes = lib.goalnet_conv1_wgrad_ws_bytes(n, h, w)
    ws = _ws(bands, nbytes)
    _ok(lib.goalnet_conv1_wgrad(ptr(xg), ptr(dyg), ptr(dw), ptr(db), ptr(ws), nbytes, n, h, w, _s()), "conv1_wgrad")
    close("conv1_wgrad.dw", dw, wd.grad.permute(0, 2, 3, 1), rtol=2e-5)
    close("conv1_wgrad.db", db, bd.grad, rtol=2e-5)
    bands.assert_bands_intact()


# ---------------------------------------------------------------------------------------------------------------------------
# zero-padded 16-bit layouts: the whole total_elems buffer is the payload (its guard pixels are zero by contract), bands outside
# ---------------------------------------------------------------------------------------------------------------------------
H16 = {"bf16": torch.bfloat16, "fp16": torch.float16}


def _padded(lib, bands, n, h, w, c, dtype, name):
    """(whole buffer, view at padded pixel 0) of goalnet_bf16_padded_layout, zeroed, between bands"""
    tot, off = ctypes.c_int64(), ctypes.c_int64()
    _ok(lib.goalnet_bf16_padded_layout(n, h, w, c, ctypes.byref(tot), ctypes.byref(off)), "bf16_padded_layout")
    buf = bands.guarded(tot.value, dtype, fill=0, name=name)
    return buf, buf[off.value:]


def _interior(view, n, h, w, c):
    return view[: n * (h + 2) * (w + 2) * c].view(n, h + 2, w + 2, c)[:, 1:-1, 1:-1, :]


def _only_interior_written(buf, view, n, h, w, c, what):
    """borders and guard pixels keep their zeros: the buffer's non-zero count is the interior's"""
    assert torch.count_nonzero(buf.float()).item() == torch.count_nonzero(_interior(view, n, h, w, c).float()).item(), \
        f"{what}: a border or guard pixel of the padded layout was written"


def _to_padded(lib, bands, x, dtype, name):
    n, h, w, c = x.shape
    buf, view = _padded(lib, bands, n, h, w, c, dtype, name)
    xg = bands.place(x, name + ".f32")
    _ok(lib.goalnet_to_bf16_padded(ptr(xg), 0, 0, ptr(view), n, h, w, c, int(dtype == torch.float16), _s()), "to_bf16_padded")
    assert bits_equal(_interior(view, n, h, w, c).cpu(), x.to(dtype)), f"{name}: the padded copy is not the rounded tensor"
    _only_interior_written(buf, view, n, h, w, c, name)
    return view


# ---------------------------------------------------------------------------------------------------------------------------
# the large pool / BatchNorm kernels: slice-major argmax store, fp64 partial rows, fused backward (fp32 and 16-bit operands)
# ---------------------------------------------------------------------------------------------------------------------------
def _pool_case(n, hc, wc, c):
    y = F.relu(rnd(n, hc, wc, c, seed=16))                 # many exact zeros: ties
    pd, pidx = F.max_pool2d(nchw(y.double()), 3, 1, 0, return_indices=True)
    hp, wp = hc - 2, wc - 2
    tap = ((pidx // wc - torch.arange(hp).view(1, 1, hp, 1)) * 3 + (pidx % wc - torch.arange(wp).view(1, 1, 1, wp))).to(torch.uint8)
    return y, nhwc(pd), nhwc(tap)


def _bnpool_bwd_fp64(dz, p, tap, coef3, n, hc, wc, c):
    """dp = a dz + b p + c per channel, routed to the argmax tap of each 3 x 3 window, gated by the ReLU mask read off p (p > 0)"""
    a, b, k = (coef3[i * c:(i + 1) * c].double() for i in range(3))
    dp = (a * dz.double() + b * p.double() + k) * (p > 0)
    dy = torch.zeros(n, hc, wc, c, dtype=torch.float64)
    for t in range(9):
        dy[:, t // 3:t // 3 + hc - 2, t % 3:t % 3 + wc - 2, :] += dp * (tap == t)
    return dy


@pytest.mark.parametrize("kind", ["f32", "bf16", "fp16"])
@pytest.mark.parametrize("n,hc,wc,c,nparts", POOL)
def test_pool_bnstats_and_bnpool_bwd_guarded(n, hc, wc, c, nparts, kind):
    """pool_bnstats_fwd / _p16 then bnpool_bwd / bnpool_bwd_bf16p_t. Max-pool and argmax bit-exact against ATen (the 16-bit p is
    the maximum rounded once); the fp64 partial rows against the sums of the stored values (1e-12, as
    test_bf16_pooled_activation_variants_match_the_fp32_kernels_on_the_stored_values); dy against the fp64 restatement above to
    1e-5 and the bias-gradient rows to the cancellation bound of test_pool_bn_forward_and_backward; the padded 16-bit dy is the
    fp32 dy rounded once."""
    from cvml_goalnet_amd import ops
    lib = _lib.load()
    dt = H16.get(kind, F32)
    f16 = int(kind == "fp16")
    hp, wp = hc - 2, wc - 2
    y, pool, tap = _pool_case(n, hc, wc, c)
    bands = Bands()
    yg = bands.place(y, "y")
    p = bands.guarded((n, hp, wp, c), dt, name="p")
    idx = bands.guarded(n * hp * wp * c, torch.uint8, name="idx")
    partials = bands.guarded((nparts, 2, c), torch.float64, name="partials")
    if kind == "f32":
        _ok(lib.goalnet_pool_bnstats_fwd(ptr(yg), ptr(p), ptr(idx), ptr(partials), nparts, n, hc, wc, c, _s()), "pool_bnstats_fwd")
    else:
        _ok(lib.goalnet_pool_bnstats_fwd_p16(ptr(yg), 0, ptr(p), ptr(idx), ptr(partials), nparts, n, hc, wc, c, f16, _s()), "pool_bnstats_fwd_p16")
    stored = pool.float().to(dt)
    assert bits_equal(p.cpu(), stored), "pooled values"
    assert torch.equal(ops.idx_to_nhwc(idx, n, hp, wp, c).cpu(), tap), "argmax positions differ from ATen's"
    tot = partials.sum(0).cpu()
    sd = stored.double()
    assert torch.allclose(tot[0], sd.sum((0, 1, 2)), rtol=1e-12, atol=1e-9) and torch.allclose(tot[1], (sd ** 2).sum((0, 1, 2)), rtol=1e-12, atol=1e-9)
    bands.assert_bands_intact()
    # ---- backward
    dz = rnd(n, hp, wp, c, seed=21).to(dt)
    coef3 = torch.cat([rnd(c, seed=22, lo=0.5, hi=1.5), rnd(c, seed=23, lo=-0.2, hi=0.2), rnd(c, seed=24, lo=-0.1, hi=0.1)])
    dzg, cg = bands.place(dz, "dz"), bands.place(coef3, "coef3")
    dy = bands.guarded((n, hc, wc, c), F32, name="dy")
    dparts = bands.guarded((nparts, c), torch.float64, name="dbias_partials")
    if kind == "f32":
        _ok(lib.goalnet_bnpool_bwd(ptr(dzg), ptr(p), ptr(idx), ptr(cg), ptr(dy), ptr(dparts), nparts, n, hc, wc, c, _s()), "bnpool_bwd")
    else:
        buf, dyp = _padded(lib, bands, n, hc, wc, c, dt, "dy_pad")
        _ok(lib.goalnet_bnpool_bwd_bf16p_t(ptr(dzg), 1, ptr(p), 1, ptr(idx), ptr(cg), ptr(dy), ptr(dyp), ptr(dparts), nparts, n, hc, wc, c, f16, _s()),
            "bnpool_bwd_bf16p_t")
        assert bits_equal(_interior(dyp, n, hc, wc, c).cpu(), dy.cpu().to(dt)), "the padded 16-bit dy is not the fp32 dy rounded once"
        _only_interior_written(buf, dyp, n, hc, wc, c, "bnpool_bwd_bf16p_t")
    want = _bnpool_bwd_fp64(dz, stored, tap, coef3, n, hc, wc, c)
    close("bn+pool+relu bwd", dy, want, rtol=1e-5)
    close("dbias partial rows", dparts.sum(0), want.sum((0, 1, 2)), rtol=0.0, atol=3e-6 * want.abs().max().item() * (n * hc * wc) ** 0.5)
    bands.assert_bands_intact()


@pytest.mark.parametrize("kind", ["f32", "bf16", "fp16"])
@pytest.mark.parametrize("n,hc,wc,c,nparts", POOL)
def test_pool_bn_eval_fwd_guarded(n, hc, wc, c, nparts, kind):
    """eval mode: p and idx as the train-mode kernels store them, st = (running_mean, invstd, scale, shift) to 1e-6 as
    test_pool_bn_eval_fwd_equals_pool_bnstats_fwd (tests/test_gpu_eval.py), the running buffers read only"""
    from cvml_goalnet_amd import ops
    lib = _lib.load()
    dt = H16.get(kind, F32)
    hp, wp = hc - 2, wc - 2
    y, pool, tap = _pool_case(n, hc, wc, c)
    gamma, beta = rnd(c, seed=17, lo=-1.0, hi=1.0), rnd(c, seed=18)
    rm, rv = rnd(c, seed=19, lo=-1.5, hi=1.5), rnd(c, seed=20, lo=0.25, hi=4.0)
    bands = Bands()
    yg, gg, bg, rmg, rvg = (bands.place(t, nm) for t, nm in ((y, "y"), (gamma, "gamma"), (beta, "beta"), (rm, "running_mean"), (rv, "running_var")))
    p = bands.guarded((n, hp, wp, c), dt, name="p")
    idx = bands.guarded(n * hp * wp * c, torch.uint8, name="idx")
    st = bands.guarded((4, c), F32, name="st")
    _ok(lib.goalnet_pool_bn_eval_fwd(ptr(yg), 0, ptr(p), int(kind != "f32"), ptr(idx), ptr(gg), ptr(bg), ptr(rmg), ptr(rvg), 1e-5, ptr(st), nparts,
                                     n, hc, wc, c, int(kind == "fp16"), _s()), "pool_bn_eval_fwd")
    assert bits_equal(p.cpu(), pool.float().to(dt)), "pooled values"
    assert torch.equal(ops.idx_to_nhwc(idx, n, hp, wp, c).cpu(), tap), "argmax positions differ from ATen's"
    assert bits_equal(rmg.cpu(), rm) and bits_equal(rvg.cpu(), rv), "eval mode wrote the running statistics"
    inv = 1.0 / torch.sqrt(rv.double() + 1e-5)
    want = torch.stack([rm.double(), inv, gamma.double() * inv, beta.double() - rm.double() * gamma.double() * inv])
    assert (st.cpu().double() - want).abs().max().item() <= 1e-6 * max(1.0, want.abs().max().item())
    bands.assert_bands_intact()


# ---------------------------------------------------------------------------------------------------------------------------
# the 16-bit engine: both GOALNET_BF16_TILE values, both formats. Products of two 8- or 11-bit significands are exact in fp32 and
# the accumulation is fp32, so against fp64 on the SAME rounded operands the tolerances are those of tests/test_gpu_ops.py
# ---------------------------------------------------------------------------------------------------------------------------
TILES_FORMATS = [(t, f) for t in ("128", "256") for f in ("bf16", "fp16")]


@pytest.mark.parametrize("tile,fmt", TILES_FORMATS)
@pytest.mark.parametrize("n,h,w,cin,cout,bias,relu", BF16_CONV)
def test_conv3x3_fwd_bf16p_guarded(n, h, w, cin, cout, bias, relu, tile, fmt, monkeypatch):
    monkeypatch.setenv("GOALNET_BF16_TILE", tile)
    lib = _lib.load()
    dt, f16 = H16[fmt], int(fmt == "fp16")
    x = rnd(n, h, w, cin, seed=63)
    wt = rnd(cout, 3, 3, cin, seed=64, lo=-0.05, hi=0.05).to(dt)
    b = rnd(cout, seed=65) if bias else None
    ref = F.conv2d(nchw(x.to(dt).double()), wt.double().permute(0, 3, 1, 2), None if b is None else b.double(), padding=1)
    ref = nhwc(F.relu(ref) if relu else ref)
    bands = Bands()
    xp = _to_padded(lib, bands, x, dt, "x_pad")
    wg = bands.place(wt, "w")
    bg = None if b is None else bands.place(b, "bias")
    y = bands.guarded((n, h, w, cout), F32, name="y")
    nbytes = lib.goalnet_conv3x3_fwd_bf16p_ws_bytes(n, h, w, cin, cout)
    ws = _ws(bands, nbytes)
    _ok(lib.goalnet_conv3x3_fwd_bf16p(ptr(xp), ptr(wg), ptr(bg), int(relu), ptr(y), n, h, w, cin, cout, ptr(ws), nbytes, f16, _s()), "conv3x3_fwd_bf16p")
    close(f"conv3x3_fwd_bf16p[{n}x{h}x{w}x{cin}->{cout}] {tile} {fmt}", y, ref, rtol=5e-6)
    bands.assert_bands_intact()


@pytest.mark.parametrize("fmt", ["bf16", "fp16"])
@pytest.mark.parametrize("bias_relu", [False, True])
def test_conv3x3_fwd_bf16p_o16_guarded(bias_relu, fmt, monkeypatch):
    """the 16-bit-output form (256 x 256 tile only) stores the fp32 accumulator rounded once: bit-identical to the fp32-output form
    rounded to nearest even, ragged rows and columns included (test_bf16_gradient_outputs_equal_the_fp32_outputs_rounded_once)"""
    monkeypatch.setenv("GOALNET_BF16_TILE", "256")
    lib = _lib.load()
    dt, f16 = H16[fmt], int(fmt == "fp16")
    n, h, w, cin, cout = O16_CONV
    assert lib.goalnet_conv3x3_fwd_bf16p_o16_ok(n, h, w, cin, cout)
    x = rnd(n, h, w, cin, seed=63)
    wt = rnd(cout, 3, 3, cin, seed=64, lo=-0.05, hi=0.05).to(dt)
    b = rnd(cout, seed=65) if bias_relu else None
    ref = F.conv2d(nchw(x.to(dt).double()), wt.double().permute(0, 3, 1, 2), None if b is None else b.double(), padding=1)
    ref = nhwc(F.relu(ref) if bias_relu else ref)
    bands = Bands()
    xp, wg = _to_padded(lib, bands, x, dt, "x_pad"), bands.place(wt, "w")
    bg = None if b is None else bands.place(b, "bias")
    y32, y16 = bands.guarded((n, h, w, cout), F32, name="y32"), bands.guarded((n, h, w, cout), dt, name="y16")
    nbytes = lib.goalnet_conv3x3_fwd_bf16p_ws_bytes(n, h, w, cin, cout)
    ws = _ws(bands, nbytes)
    _ok(lib.goalnet_conv3x3_fwd_bf16p(ptr(xp), ptr(wg), ptr(bg), int(bias_relu), ptr(y32), n, h, w, cin, cout, ptr(ws), nbytes, f16, _s()), "conv3x3_fwd_bf16p")
    _ok(lib.goalnet_conv3x3_fwd_bf16p_o16(ptr(xp), ptr(wg), ptr(bg), int(bias_relu), ptr(y16), n, h, w, cin, cout, f16, _s()), "conv3x3_fwd_bf16p_o16")
    close("conv3x3_fwd_bf16p (256)", y32, ref, rtol=5e-6)
    assert bits_equal(y16.cpu(), y32.cpu().to(dt)), "the 16-bit output is not the fp32 output rounded once"
    bands.assert_bands_intact()


@pytest.mark.parametrize("tile,fmt", TILES_FORMATS)
@pytest.mark.parametrize("n,h,w,cin,cout", BF16_WGRAD)
def test_conv3x3_wgrad_bf16_guarded(n, h, w, cin, cout, tile, fmt, monkeypatch):
    monkeypatch.setenv("GOALNET_BF16_TILE", tile)
    lib = _lib.load()
    dt, f16 = H16[fmt], int(fmt == "fp16")
    x, dy = rnd(n, h, w, cin, seed=66), rnd(n, h, w, cout, seed=67)
    ref = torch.nn.grad.conv2d_weight(nchw(x.to(dt).double()), (cout, cin, 3, 3), nchw(dy.to(dt).double()), padding=1)
    bands = Bands()
    xp, dyp = _to_padded(lib, bands, x, dt, "x_pad"), _to_padded(lib, bands, dy, dt, "dy_pad")
    dw = bands.guarded((cout, 3, 3, cin), F32, name="dw")
    nbytes = lib.goalnet_conv3x3_wgrad_bf16_ws_bytes(n, h, w, cin, cout)
    ws = _ws(bands, nbytes)
    _ok(lib.goalnet_conv3x3_wgrad_bf16(ptr(xp), ptr(dyp), ptr(dw), ptr(ws), nbytes, n, h, w, cin, cout, f16, _s()), "conv3x3_wgrad_bf16")
    close(f"conv3x3_wgrad_bf16[{n}x{h}x{w}x{cin}->{cout}] {tile} {fmt}", dw, ref.permute(0, 2, 3, 1), rtol=5e-6)
    bands.assert_bands_intact()


@pytest.mark.parametrize("tile,fmt", TILES_FORMATS)
@pytest.mark.parametrize("m,k,j", BF16_LINEAR_FWD)
def test_linear_fwd_bf16_guarded(m, k, j, tile, fmt, monkeypatch):
    monkeypatch.setenv("GOALNET_BF16_TILE", tile)
    lib = _lib.load()
    dt, f16 = H16[fmt], int(fmt == "fp16")
    x, w, b = rnd(m, k, seed=56).to(dt), rnd(j, k, seed=57, lo=-0.05, hi=0.05).to(dt), rnd(j, seed=58)
    dm = (torch.rand(m, j, generator=torch.Generator().manual_seed(59)) >= 0.2).float() * 1.25
    pre = x.double() @ w.double().t() + b.double()
    ref = F.relu(pre) * dm.double()
    bands = Bands()
    xg, wg, bg, dmg = bands.place_rows(x, k + 8, "x"), bands.place(w, "w"), bands.place(b, "bias"), bands.place_rows(dm, j + 4, "dropmask")
    y, mult = bands.guarded_rows(m, j, j + 4, F32, name="y"), bands.guarded_rows(m, j, j + 8, F32, name="mult_out")
    nbytes = lib.goalnet_linear_fwd_bf16_ws_bytes(m, k, j)
    ws = _ws(bands, nbytes)
    _ok(lib.goalnet_linear_fwd_bf16(ptr(xg), k + 8, ptr(wg), ptr(bg), 1, ptr(dmg), j + 4, ptr(y), j + 4, ptr(mult), j + 8, m, k, j, ptr(ws), nbytes, f16, _s()),
        "linear_fwd_bf16")
    close(f"linear_fwd_bf16[{m}x{k}->{j}] {tile} {fmt}", y, ref, rtol=3e-6)
    saved_mult_check(f"linear_fwd_bf16[{m}x{k}->{j}] {tile} {fmt}", mult, pre, dm, 3e-6)
    bands.assert_bands_intact()


@pytest.mark.parametrize("tile,fmt", TILES_FORMATS)
@pytest.mark.parametrize("m,k,j,use_mult", BF16_LINEAR_BWD)
def test_linear_bwd_bf16_guarded(m, k, j, use_mult, tile, fmt, monkeypatch):
    monkeypatch.setenv("GOALNET_BF16_TILE", tile)
    lib = _lib.load()
    dt, f16 = H16[fmt], int(fmt == "fp16")
    dy, w, x = rnd(m, j, seed=68).to(dt), rnd(j, k, seed=69, lo=-0.05, hi=0.05).to(dt), rnd(m, k, seed=70).to(dt)
    mult = (torch.rand(m, k, generator=torch.Generator().manual_seed(71)) >= 0.5).float() * 1.25 if use_mult else None
    ref = dy.double() @ w.double()
    if use_mult:
        ref = ref * mult.double()
    bands = Bands()
    dyg, wg, xg = bands.place_rows(dy, j + 8, "dy"), bands.place(w, "w"), bands.place_rows(x, k + 8, "x")
    mg = None if mult is None else bands.place_rows(mult, k + 4, "mult")
    dx = bands.guarded_rows(m, k, k + 4, F32, name="dx")
    _ok(lib.goalnet_linear_bwd_dx_bf16(ptr(dyg), j + 8, ptr(wg), ptr(mg), k + 4, ptr(dx), k + 4, m, k, j, f16, _s()), "linear_bwd_dx_bf16")
    close(f"linear_bwd_dx_bf16[{m}x{j}->{k}] {tile} {fmt}", dx, ref, rtol=3e-6)
    dw = bands.guarded((j, k), F32, name="dw")
    _ok(lib.goalnet_linear_bwd_dw_bf16(ptr(dyg), j + 8, ptr(xg), k + 8, ptr(dw), m, k, j, f16, _s()), "linear_bwd_dw_bf16")
    close(f"linear_bwd_dw_bf16[{m}: {j}x{k}] {tile} {fmt}", dw, dy.double().t() @ x.double(), rtol=3e-6)
    bands.assert_bands_intact()


@pytest.mark.parametrize("fmt", ["bf16", "fp16"])
def test_linear_bwd_dx_bf16_o16_guarded(fmt, monkeypatch):
    """dx stored in 16 bits (256 x 256 tile only): the fp32-output form rounded once, on ragged rows and columns"""
    monkeypatch.setenv("GOALNET_BF16_TILE", "256")
    lib = _lib.load()
    dt, f16 = H16[fmt], int(fmt == "fp16")
    m, k, j = O16_LINEAR
    assert lib.goalnet_linear_bwd_dx_bf16_o16_ok(m, k, j)
    dy, w = rnd(m, j, seed=68, lo=-0.5, hi=0.5).to(dt), rnd(j, k, seed=69, lo=-0.5, hi=0.5).to(dt)
    bands = Bands()
    dyg, wg = bands.place(dy, "dy"), bands.place(w, "w")
    dx32, dx16 = bands.guarded_rows(m, k, k + 4, F32, name="dx32"), bands.guarded_rows(m, k, k + 8, dt, name="dx16")
    _ok(lib.goalnet_linear_bwd_dx_bf16(ptr(dyg), j, ptr(wg), 0, 0, ptr(dx32), k + 4, m, k, j, f16, _s()), "linear_bwd_dx_bf16")
    _ok(lib.goalnet_linear_bwd_dx_bf16_o16(ptr(dyg), j, ptr(wg), ptr(dx16), k + 8, m, k, j, f16, _s()), "linear_bwd_dx_bf16_o16")
    close("linear_bwd_dx_bf16 (256)", dx32, dy.double() @ w.double(), rtol=3e-6)
    assert bits_equal(dx16.cpu(), dx32.cpu().to(dt)), "the 16-bit dx is not the fp32 dx rounded once"
    bands.assert_bands_intact()


# ---------------------------------------------------------------------------------------------------------------------------
# the split engine (bf16 triples / scaled fp16 pairs): split_padded, split_rows, conv3x3_fwd_split, conv3x3_wgrad_split, linear_fwd_split
# ---------------------------------------------------------------------------------------------------------------------------
def _amax(lib, bands, x, ld, rows, c, scale=None, shift=None, bnc=0, name="amax"):
    word = bands.guarded(1, torch.int32, fill=0, name=name)
    _ok(lib.goalnet_absmax(ptr(x), ld, ptr(scale), ptr(shift), bnc, rows, c, ptr(word), _s()), "absmax")
    return word


def _oscale(lib, bands, a, b, name):
    o = bands.guarded(1, torch.int32, name=name)
    _ok(lib.goalnet_split_scales(ptr(a), ptr(b), ptr(o), _s()), "split_scales")
    return o


def _parts_are(got2d, want_f32, parts, scale, c, what):
    """the parts lie side by side and are torch's own roundings of the value, bit for bit (test_split_is_exact_...)"""
    for k, part in enumerate(_split_host(want_f32, parts, scale)):
        assert bits_equal(got2d[..., k * c:(k + 1) * c].cpu().contiguous(), part.contiguous()), f"{what}: part {k} differs from torch's rounding"


@pytest.mark.parametrize("parts", [3, 2])
def test_conv3x3_split_guarded(parts):
    """inputs, fp64 oracle on the UNROUNDED operands and the 6e-6 bound of
    test_conv3x3_split_forward_data_gradient_and_weight_gradient_vs_fp64 (tests/test_gpu_ops.py)"""
    lib = _lib.load()
    n, h, w, cin, cout, bias, relu = SPLIT_CONV
    dt = torch.bfloat16 if parts == 3 else torch.float16
    x = torch.relu(rnd(n, h, w, cin, seed=310) * 2.0)
    sc, sh = rnd(cin, seed=311, lo=0.5, hi=1.5), rnd(cin, seed=312, lo=-0.5, hi=0.5)
    wt = rnd(cout, 3, 3, cin, seed=313) * 0.05
    b = rnd(cout, seed=314)
    dy = rnd(n, h, w, cout, seed=315) * (10.0 ** (-7 + 4 * rnd(cout, seed=316, lo=0.0, hi=1.0)))
    bands = Bands()
    xg, scg, shg, wg, bg, dyg = (bands.place(t, nm) for t, nm in ((x, "x"), (sc, "scale"), (sh, "shift"), (wt, "w"), (b, "bias"), (dy, "dy")))
    ax = aw = ady = oxw = oyx = None
    if parts == 2:
        ax = _amax(lib, bands, xg, cin, n * h * w, cin, scg, shg, cin, "amax_x")
        aw = _amax(lib, bands, wg, cin, cout * 9, cin, name="amax_w")
        ady = _amax(lib, bands, dyg, cout, n * h * w, cout, name="amax_dy")
        oxw, oyx = _oscale(lib, bands, ax, aw, "oscale_xw"), _oscale(lib, bands, ady, ax, "oscale_dyx")
    bufx, xps = _padded(lib, bands, n, h, w, parts * cin, dt, "x_pads")
    _ok(lib.goalnet_split_padded(parts, ptr(xg), ptr(scg), ptr(shg), ptr(ax), ptr(xps), n, h, w, cin, _s()), "split_padded")
    xa = (x.double() * sc.double() + sh.double()).float()                 # the correctly rounded fma
    _parts_are(_interior(xps, n, h, w, parts * cin), xa, parts, 1.0 if parts == 3 else _scale_of(ax), cin, "split_padded")
    _only_interior_written(bufx, xps, n, h, w, parts * cin, "split_padded")
    wsp = bands.guarded((cout * 9, parts * cin), dt, name="w_parts")
    _ok(lib.goalnet_split_rows(parts, ptr(wg), cin, 0, 0, 0, ptr(aw), ptr(wsp), cout * 9, cin, _s()), "split_rows")
    _parts_are(wsp, wt.view(cout * 9, cin), parts, 1.0 if parts == 3 else _scale_of(aw), cin, "split_rows")
    y = bands.guarded((n, h, w, cout), F32, name="y")
    _ok(lib.goalnet_conv3x3_fwd_split(parts, ptr(xps), ptr(wsp), ptr(bg), int(relu), ptr(y), n, h, w, cin, cout, ptr(oxw), _s()), "conv3x3_fwd_split")
    xh = nchw(x.double() * sc.double() + sh.double())
    ref = F.conv2d(xh, nchw(wt.double()), b.double(), padding=1)
    close(f"conv3x3_fwd_split[{parts}] vs fp64", y, nhwc(F.relu(ref)), rtol=6e-6)
    bufdy, dyps = _padded(lib, bands, n, h, w, parts * cout, dt, "dy_pads")
    _ok(lib.goalnet_split_padded(parts, ptr(dyg), 0, 0, ptr(ady), ptr(dyps), n, h, w, cout, _s()), "split_padded")
    _only_interior_written(bufdy, dyps, n, h, w, parts * cout, "split_padded(dy)")
    dw = bands.guarded((cout, 3, 3, cin), F32, name="dw")
    nbytes = lib.goalnet_conv3x3_wgrad_split_ws_bytes(parts, n, h, w, cin, cout)
    ws = _ws(bands, nbytes)
    _ok(lib.goalnet_conv3x3_wgrad_split(parts, ptr(xps), ptr(dyps), ptr(dw), ptr(ws), nbytes, n, h, w, cin, cout, ptr(oyx), _s()), "conv3x3_wgrad_split")
    refdw = torch.nn.grad.conv2d_weight(xh, (cout, cin, 3, 3), nchw(dy.double()), padding=1).permute(0, 2, 3, 1)
    close(f"conv3x3_wgrad_split[{parts}] vs fp64", dw, refdw, rtol=6e-6)
    bands.assert_bands_intact()


_SPLIT_LINEAR_CASE = []


def _split_linear_case():
    """the operands and the fp64 result, computed once for both values of `parts`"""
    if not _SPLIT_LINEAR_CASE:
        m, k, j, bnc = SPLIT_LINEAR
        x, w, b = rnd(m, k, seed=320), rnd(j, k, seed=323) * 0.02, rnd(j, seed=324)
        sc, sh = rnd(bnc, seed=321, lo=0.5, hi=1.5), rnd(bnc, seed=322, lo=-0.5, hi=0.5)
        mask = (rnd(m, j, seed=326) > 0).float() * 2.0
        xh = x.double() * sc.double().repeat(k // bnc) + sh.double().repeat(k // bnc)
        pre = xh @ w.double().t() + b.double()
        _SPLIT_LINEAR_CASE.append((x, w, b, sc, sh, mask, F.relu(pre) * mask.double(), pre))
    return _SPLIT_LINEAR_CASE[0]


@pytest.mark.parametrize("parts", [3, 2])
def test_linear_fwd_split_guarded(parts):
    """linear5's forward on split operands at the shape of test_linear5_on_split_operands_forward_dx_dw_vs_fp64 (ragged in M and K), 6e-6"""
    lib = _lib.load()
    m, k, j, bnc = SPLIT_LINEAR
    assert lib.goalnet_linear_split_ok(parts, m, k, j)
    dt = torch.bfloat16 if parts == 3 else torch.float16
    x, w, b, sc, sh, mask, ref, pre = _split_linear_case()
    bands = Bands()
    xg, wg, bg, scg, shg, mg = (bands.place(t, nm) for t, nm in ((x, "x"), (w, "w"), (b, "bias"), (sc, "scale"), (sh, "shift"), (mask, "dropmask")))
    ax = aw = osc = None
    if parts == 2:
        ax, aw = _amax(lib, bands, xg, k, m, k, scg, shg, bnc, "amax_x"), _amax(lib, bands, wg, k, j, k, name="amax_w")
        osc = _oscale(lib, bands, ax, aw, "oscale")
    xs, wsp = bands.guarded((m, parts * k), dt, name="x_parts"), bands.guarded((j, parts * k), dt, name="w_parts")
    _ok(lib.goalnet_split_rows(parts, ptr(xg), k, ptr(scg), ptr(shg), bnc, ptr(ax), ptr(xs), m, k, _s()), "split_rows")
    _ok(lib.goalnet_split_rows(parts, ptr(wg), k, 0, 0, 0, ptr(aw), ptr(wsp), j, k, _s()), "split_rows")
    y, mult = bands.guarded_rows(m, j, j + 4, F32, name="y"), bands.guarded_rows(m, j, j + 8, F32, name="mult_out")
    nbytes = lib.goalnet_linear_fwd_split_ws_bytes(parts, m, k, j)
    ws = _ws(bands, nbytes)
    _ok(lib.goalnet_linear_fwd_split(parts, ptr(xs), ptr(wsp), ptr(bg), 1, ptr(mg), j, ptr(y), j + 4, ptr(mult), j + 8, m, k, j, ptr(ws), nbytes, ptr(osc), _s()),
        "linear_fwd_split")
    close(f"linear_fwd_split[{parts}] vs fp64", y, ref, rtol=6e-6)
    saved_mult_check(f"linear_fwd_split[{parts}]", mult, pre, mask, 6e-6)
    bands.assert_bands_intact()


# ---------------------------------------------------------------------------------------------------------------------------
# the classifier head (extension): scores = 4 softmax(h w^T + b) + 1, cross entropy, backward
# ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [1, 10, 515])
def test_cls_head_guarded(n):
    """inputs, fp64 autograd oracle and bounds of test_classifier_head_kernels_vs_torch_fp64 (tests/test_gpu_classifier.py); h, mult
    and dh on leading dimensions above K"""
    lib = _lib.load()
    C, k = 5, 128
    g = torch.Generator().manual_seed(3 + n)
    h = torch.rand(n, k, generator=g) * 2 - 0.5
    w = (torch.rand(C, k, generator=g) - 0.5) * 0.4
    b = torch.rand(C, generator=g) - 0.5
    mult = (torch.rand(n, k, generator=g) >= 0.2).float() * 1.25
    lab = torch.randint(1, C + 1, (n,), generator=g).float()
    hd, wd, bd = h.double().requires_grad_(True), w.double().requires_grad_(True), b.double().requires_grad_(True)
    z = F.linear(hd, wd, bd)
    s = 4 * torch.softmax(z, dim=1) + 1
    loss = F.cross_entropy(s, (lab - 1).long())
    loss.backward()
    bands = Bands()
    hg, wg, bg, mg, labg = bands.place_rows(h, k + 4, "h"), bands.place(w, "w"), bands.place(b, "b"), bands.place_rows(mult, k + 8, "mult"), bands.place(lab, "labels")
    logits, scores = bands.guarded((n, C), F32, name="logits"), bands.guarded((n, C), F32, name="scores")
    _ok(lib.goalnet_cls_head_fwd(ptr(hg), k + 4, ptr(wg), ptr(bg), ptr(logits), ptr(scores), n, k, C, _s()), "cls_head_fwd")
    assert (logits.cpu().double() - z.detach()).abs().max().item() < 2e-6
    assert (scores.cpu().double() - s.detach()).abs().max().item() < 2e-6
    lg, ds = bands.guarded(1, F32, name="loss"), bands.guarded((n, C), F32, name="dscores")
    _ok(lib.goalnet_cross_entropy(ptr(scores), ptr(labg), ptr(lg), ptr(ds), n, C, _s()), "cross_entropy")
    assert abs(lg.item() - loss.item()) < 2e-6 * max(1.0, abs(loss.item()))
    dh = bands.guarded_rows(n, k, k + 12, F32, name="dh")
    dw, db = bands.guarded((C, k), F32, name="dw"), bands.guarded(C, F32, name="db")
    _ok(lib.goalnet_cls_head_bwd(ptr(ds), ptr(scores), ptr(hg), k + 4, ptr(wg), ptr(mg), k + 8, ptr(dh), k + 12, ptr(dw), ptr(db), n, k, C, _s()), "cls_head_bwd")
    for name, got, want in (("dh", dh, hd.grad * mult.double()), ("dw", dw, wd.grad), ("db", db, bd.grad)):
        assert (got.cpu().double() - want).abs().max().item() <= 5e-6 * max(want.abs().max().item(), 1e-30), name
    classes = bands.guarded(n, F32, name="classes")
    _ok(lib.goalnet_argmax_plus1(ptr(scores), ptr(classes), n, C, _s()), "argmax_plus1")
    assert torch.equal(classes.cpu(), (torch.argmax(scores.cpu(), dim=1) + 1).float())
    bands.assert_bands_intact()
