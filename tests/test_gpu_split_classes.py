"""GPU: the fp32 GEMM engine at every split-K and tile-order class against fp64 (tests/_split_classes.py has the classes and the tables,
tests/test_split_classes_host.py holds the tables against the dispatch rules on the CPU).

Every row calls its entry point through the raw C ABI with the inputs between NaN bands, the output in a guarded view and a workspace of
exactly *_ws_bytes float32 NaNs: a (tile, split) slab that no block wrote turns the output to NaN, one written twice is harmless only if both
blocks computed the same, and a slab summed twice or a tile computed from the wrong K range misses the tolerance. Reference and tolerance are
those of test_conv3x3_fwd, test_conv3x3_wgrad and test_linear_fwd (tests/test_gpu_ops.py): fp64 torch CPU on the same fp32 inputs,
`close` at 5e-6 (convolutions) and 3e-6 (linear forward) of max |reference|. Every split row runs twice and must repeat its bits (the
slabs are summed in a fixed order); with ticket counters the fused reduction must give the bits of the two-launch form and leave the
counters zero; all bands stay intact."""
import pytest
import torch

import _split_classes as S
from _abi_cases import (_conv_fwd_call, _conv_fwd_case, _conv_wgrad_call, _conv_wgrad_case, _counters_clean, _linear_fwd_call,
                        _linear_fwd_case)
from _abi_guard import Bands, bits_equal
from cvml_goalnet_amd import _lib
from test_gpu_ops import close

pytestmark = pytest.mark.gpu

NAN = float("nan")


def _repeats(call, outs, bands, what):
    """a second launch on the same buffers gives the same bits"""
    first = [o.clone() for o in outs]
    for o in outs:
        o.fill_(NAN)
    call()
    for o, f in zip(outs, first):
        assert bits_equal(o, f), f"{what}: the second call differs from the first"
    bands.assert_bands_intact()


@pytest.mark.parametrize("n,h,w,cin,cout,affine,bias,relu", S.CONV_FWD_ROWS)
def test_conv3x3_fwd_at_every_split_class(n, h, w, cin, cout, affine, bias, relu):
    lib = _lib.load()
    dims = (n, h, w, cin, cout)
    tiles, nsplit = S.conv_fwd_plan(*dims)
    assert lib.goalnet_conv3x3_fwd_ws_bytes(*dims) == (4 * nsplit * n * h * w * cout if nsplit > 1 else 0)
    cls = "/".join(S.order_class(tiles, nsplit))
    case = _conv_fwd_case(n, h, w, cin, cout, affine, bias, relu)
    modes = ("null", "ws", "ctr") if (n, h, w, cin, cout, affine, bias, relu) == S.CONV_FWD_CTR else ("null", "ws")
    got = {}
    for mode in modes:                  # "null": the unsplit launch, held to the same tolerance and not compared with the split one
        bands = Bands()
        y, ctr, call = _conv_fwd_call(lib, bands, case, dims, relu, mode, nan_ws=True)
        what = f"conv3x3_fwd[{n}x{h}x{w}x{cin}->{cout}] {tiles} tiles x {nsplit if mode != 'null' else 1} splits ({cls if mode != 'null' else 'one'}) {mode}"
        close(what, y, case[5], rtol=5e-6)
        bands.assert_bands_intact()
        got[mode] = y.clone()
        if ctr is not None:
            _counters_clean(ctr, what)
        if mode != "null":
            _repeats(call, [y], bands, what)
        if ctr is not None:
            _counters_clean(ctr, what + ", second call")
    if "ctr" in got:
        assert bits_equal(got["ws"], got["ctr"]), "fused split-K reduction differs from the two-launch form"


def _wgrad_run(lib, case, dims, path, mode, monkeypatch, what):
    """one guarded call under GOALNET_WGRAD_PATH = path (None: unset), checked against fp64, repeated once; returns a copy of dW"""
    if path is None:
        monkeypatch.delenv("GOALNET_WGRAD_PATH", raising=False)
    else:
        monkeypatch.setenv("GOALNET_WGRAD_PATH", path)
    bands = Bands()
    dw, ctr, call = _conv_wgrad_call(lib, bands, case, dims, mode, nan_ws=True)
    close(what, dw, case[4], rtol=5e-6)
    bands.assert_bands_intact()
    out = dw.clone()
    if ctr is not None:
        _counters_clean(ctr, what)
    _repeats(call, [dw], bands, what)
    if ctr is not None:
        _counters_clean(ctr, what + ", second call")
    return out


@pytest.mark.parametrize("n,h,w,cin,cout,affine", S.WGRAD_ROWS)
def test_conv3x3_wgrad_at_every_split_class(n, h, w, cin, cout, affine, monkeypatch):
    lib = _lib.load()
    dims = (n, h, w, cin, cout)
    tiles, nsplit = S.wgrad_plan(*dims)
    assert lib.goalnet_conv3x3_wgrad_ws_bytes(*dims) == S.wgrad_ws_fixed_bytes(n, h, w, cout) + 4 * nsplit * cout * 9 * cin
    name = f"conv3x3_wgrad[{n}x{h}x{w}x{cin}->{cout}] {tiles} tiles x {nsplit} splits ({'/'.join(S.order_class(tiles, nsplit))}, {S.reduce_of('wgrad', dims)} reduce)"
    case = _conv_wgrad_case(n, h, w, cin, cout, affine)
    got = {path: _wgrad_run(lib, case, dims, path, "nocodes", monkeypatch, f"{name} {path or 'unforced'}") for path in ("select", "correct", None)}
    assert bits_equal(got[None], got[S.wgrad_path(n, h, w)]), "the unforced call is not the path the threshold names"
    if (n, h, w, cin, cout, affine) in S.WGRAD_CTR:
        fused = _wgrad_run(lib, case, dims, "select", "ctr", monkeypatch, f"{name} select, ticket counters")
        assert bits_equal(fused, got["select"]), "with ticket counters the weight gradient differs from the two-launch form"


@pytest.mark.parametrize("n,h,w,cin,cout,affine", S.WGRAD_THRESHOLD)
def test_conv3x3_wgrad_takes_the_path_its_threshold_names(n, h, w, cin, cout, affine, monkeypatch):
    """N max(H, W) = 4 096 | 4 100 with no switch set: the in-loop select up to 4 096, the border-sum correction above. The unforced result
    is the forced one of that path bit for bit, and the two paths differ in bits on these rows, so the equality tells them apart."""
    lib = _lib.load()
    dims = (n, h, w, cin, cout)
    tiles, nsplit = S.wgrad_plan(*dims)
    want = S.wgrad_path(n, h, w)
    name = f"conv3x3_wgrad[{n}x{h}x{w}x{cin}->{cout}] N max(H, W) = {n * max(h, w)} ({want}), {nsplit} splits, {S.reduce_of('wgrad', dims)} reduce"
    case = _conv_wgrad_case(n, h, w, cin, cout, affine)
    got = {path: _wgrad_run(lib, case, dims, path, "nocodes", monkeypatch, f"{name} {path or 'unforced'}") for path in (None, "select", "correct")}
    assert not bits_equal(got["select"], got["correct"]), "both paths give the same bits here: the row cannot tell them apart"
    assert bits_equal(got[None], got[want]), f"the unforced call did not take the {want} path"


@pytest.mark.parametrize("m,k,j,affine,mask,ldextra", S.LINEAR_ROWS)
def test_linear_fwd_at_every_split_class(m, k, j, affine, mask, ldextra):
    lib = _lib.load()
    tiles, nsplit = S.linear_plan(m, k, j)
    assert lib.goalnet_linear_fwd_ws_bytes(m, k, j) == (4 * nsplit * m * j if nsplit > 1 else 0)
    case = _linear_fwd_case(m, k, j, affine, mask)
    dm, pre, ref = case[5:]
    bands = Bands()
    y, mult, call = _linear_fwd_call(lib, bands, case, (m, k, j), ldextra, nan_ws=True)
    what = f"linear_fwd[{m}x{k}->{j}] {tiles} tiles x {nsplit} splits ({'/'.join(S.order_class(tiles, nsplit))})"
    close(what, y, ref, rtol=3e-6)
    # mult = (pre > 0) * mask; pre-activations within fp32 noise of 0 may legitimately differ
    want_mult = (pre > 0).double() * (dm.double() if mask else 1.0)
    safe = pre.abs() > 1e-4
    assert torch.equal(mult.cpu().double()[safe], want_mult[safe])
    bands.assert_bands_intact()
    _repeats(call, [y, mult], bands, what)
