"""Case builders for the tests that call the fp32 GEMM entry points through the raw C ABI with guarded buffers (tests/_abi_guard.py):
tests/test_gpu_abi_contract.py and tests/test_gpu_split_classes.py. A case is the seeded fp32 inputs of tests/test_gpu_ops.py's test of the
same kernel and its fp64 torch CPU reference; a call places the inputs between NaN bands, hands every output and workspace out as a guarded
view and returns the output with a closure that repeats the launch."""
import torch
import torch.nn.functional as F

from _abi_guard import ptr
from cvml_goalnet_amd import _lib
from test_gpu_ops import nchw, nhwc, rnd

F32 = torch.float32


def _s():
    return torch.cuda.current_stream().cuda_stream


def _ok(rc, what):
    _lib.check(rc, what)


def _ws(bands, nbytes, nan=False):
    """a guarded workspace of exactly nbytes bytes (None when the entry point asks for none). nan: float32 quiet NaNs instead of the 0xA5
    byte pattern, which reads as -2.9e-16 and would vanish in a sum: a split-K slab that nobody wrote then turns the output to NaN"""
    if not nbytes:
        return None
    if nan:
        assert nbytes % 4 == 0
        return bands.guarded(nbytes // 4, F32, name="ws")
    return bands.guarded(nbytes, torch.uint8, name="ws")


def _tiles128(rows, cols):
    """the header: one ticket counter per 128 x 128 output tile"""
    return ((rows + 127) // 128) * ((cols + 127) // 128)


def _counters_clean(ctr, what):
    assert not ctr.any().item(), f"{what}: {int((ctr != 0).sum())} ticket counters left non-zero"


# ---------------------------------------------------------------------------------------------------------------------------
# conv3x3_fwd
# ---------------------------------------------------------------------------------------------------------------------------
def _conv_fwd_case(n, h, w, cin, cout, affine, bias, relu):
    x = rnd(n, h, w, cin, seed=7)
    sc = rnd(cin, seed=8, lo=0.5, hi=1.5) if affine else None
    sh = rnd(cin, seed=9, lo=-0.5, hi=0.5) if affine else None
    wt = rnd(cout, 3, 3, cin, seed=10, lo=-0.05, hi=0.05)
    b = rnd(cout, seed=11) if bias else None
    xn = x.double() * sc.double() + sh.double() if affine else x.double()
    ref = F.conv2d(nchw(xn), wt.double().permute(0, 3, 1, 2), None if b is None else b.double(), padding=1)
    return x, sc, sh, wt, b, nhwc(F.relu(ref) if relu else ref)


def _conv_fwd_call(lib, bands, case, dims, relu, mode, nan_ws=False):
    """mode: 'null' (ws = NULL: no split), 'ws' (split-K slabs + reduce launch), 'ctr' (slabs + ticket counters: fused reduce)"""
    n, h, w, cin, cout = dims
    x, sc, sh, wt, b, _ = case
    xg, wg = bands.place(x, "x"), bands.place(wt, "w")
    scg, shg, bg = (None if t is None else bands.place(t, nm) for t, nm in ((sc, "scale"), (sh, "shift"), (b, "bias")))
    y = bands.guarded((n, h, w, cout), F32, name="y")
    nbytes = lib.goalnet_conv3x3_fwd_ws_bytes(*dims) if mode != "null" else 0
    ws = _ws(bands, nbytes, nan_ws)
    nctr = _tiles128(n * h * w, cout)
    ctr = bands.guarded(nctr, torch.int32, fill=0, name="tile_ctr") if mode == "ctr" else None

    def call():
        _ok(lib.goalnet_conv3x3_fwd(ptr(xg), ptr(scg), ptr(shg), ptr(wg), ptr(bg), int(relu), ptr(y), n, h, w, cin, cout, ptr(ws), nbytes,
                                    ptr(ctr), nctr if ctr is not None else 0, _s()), "conv3x3_fwd")
    call()
    return y, ctr, call


# ---------------------------------------------------------------------------------------------------------------------------
# conv3x3_wgrad
# ---------------------------------------------------------------------------------------------------------------------------
def _conv_wgrad_case(n, h, w, cin, cout, affine):
    x = rnd(n, h, w, cin, seed=12)
    sc = rnd(cin, seed=13, lo=0.5, hi=1.5) if affine else None
    sh = rnd(cin, seed=14, lo=-0.5, hi=0.5) if affine else None
    dy = rnd(n, h, w, cout, seed=15)
    xn = x.double() * sc.double() + sh.double() if affine else x.double()
    ref = torch.nn.grad.conv2d_weight(nchw(xn), (cout, cin, 3, 3), nchw(dy.double()), padding=1).permute(0, 2, 3, 1)
    return x, sc, sh, dy, ref


def _conv_wgrad_call(lib, bands, case, dims, mode, nan_ws=False):
    """mode: 'ws' (the caller's code table, slabs + reduce launch), 'ctr' (the same with ticket counters lent), 'nocodes' (the code table
    built inside the workspace). GOALNET_WGRAD_PATH is read per call: the caller sets it."""
    n, h, w, cin, cout = dims
    x, sc, sh, dy, _ = case
    nbytes = lib.goalnet_conv3x3_wgrad_ws_bytes(n, h, w, cin, cout)
    xg, dyg = bands.place(x, "x"), bands.place(dy, "dy")
    scg, shg = (None if t is None else bands.place(t, nm) for t, nm in ((sc, "scale"), (sh, "shift")))
    dw = bands.guarded((cout, 3, 3, cin), F32, name="dw")
    ws = _ws(bands, nbytes, nan_ws)
    codes = None
    if mode != "nocodes":
        codes = bands.guarded(lib.goalnet_conv3x3_wgrad_codes_bytes(n, h, w), torch.uint8, name="codes")
        _ok(lib.goalnet_conv3x3_wgrad_codes(ptr(codes), n, h, w, _s()), "conv3x3_wgrad_codes")
    nctr = _tiles128(cout, 9 * cin)
    ctr = bands.guarded(nctr, torch.int32, fill=0, name="tile_ctr") if mode == "ctr" else None

    def call():
        _ok(lib.goalnet_conv3x3_wgrad(ptr(xg), ptr(scg), ptr(shg), ptr(dyg), ptr(dw), ptr(ws), nbytes, ptr(codes), ptr(ctr),
                                      nctr if ctr is not None else 0, n, h, w, cin, cout, _s()), "conv3x3_wgrad")
    call()
    return dw, ctr, call


# ---------------------------------------------------------------------------------------------------------------------------
# linear_fwd
# ---------------------------------------------------------------------------------------------------------------------------
def _linear_fwd_case(m, k, j, affine, mask):
    """inputs, the fp64 pre-activation and the fp64 result relu(pre) * mask"""
    x = rnd(m, k, seed=22)
    w = rnd(j, k, seed=23, lo=-0.05, hi=0.05)
    b = rnd(j, seed=24)
    sc = rnd(512, seed=25, lo=0.5, hi=1.5) if affine else None
    sh = rnd(512, seed=26, lo=-0.5, hi=0.5) if affine else None
    dm = (torch.rand(m, j, generator=torch.Generator().manual_seed(27)) >= 0.2).float() * 1.25 if mask else None
    xd = x.double()
    if affine:
        ch = torch.arange(k) % 512
        xd = xd * sc.double()[ch] + sh.double()[ch]
    pre = xd @ w.double().t() + b.double()
    ref = F.relu(pre) * (dm.double() if mask else 1.0)
    return x, w, b, sc, sh, dm, pre, ref


def _linear_fwd_call(lib, bands, case, dims, ldextra, nan_ws=False):
    """y and mult_out as (m, j) views of row stride j + ldextra: the gaps between the rows are bands too"""
    m, k, j = dims
    x, w, b, sc, sh, dm, _, _ = case
    xg, wg, bg = bands.place(x, "x"), bands.place(w, "w"), bands.place(b, "bias")
    scg, shg, dmg = (None if t is None else bands.place(t, nm) for t, nm in ((sc, "scale"), (sh, "shift"), (dm, "dropmask")))
    ld = j + ldextra
    y = bands.guarded_rows(m, j, ld, F32, name="y")
    mult = bands.guarded_rows(m, j, ld, F32, name="mult_out")
    nbytes = lib.goalnet_linear_fwd_ws_bytes(m, k, j)
    ws = _ws(bands, nbytes, nan_ws)

    def call():
        _ok(lib.goalnet_linear_fwd(ptr(xg), k, ptr(scg), ptr(shg), 512 if sc is not None else 0, ptr(wg), ptr(bg), 1, ptr(dmg), j, ptr(y), ld,
                                   ptr(mult), ld, m, k, j, ptr(ws), nbytes, _s()), "linear_fwd")
    call()
    return y, mult, call

