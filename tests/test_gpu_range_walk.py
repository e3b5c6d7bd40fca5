"""GPU: every arena pass on a range LARGER than its per-range block cap, where a block of the range strides by nb * blockDim.x over
its share (csrc/ranges.h: block_share, for_share), through the raw C ABI between guard bands (tests/_abi_guard.py).

One layout serves all entry points: range 0 begins at 64 and holds 8 388 608 + 4 * 300 + 3 elements (the cap of the update, average,
swap and accumulate passes is 8 192 blocks x 256 threads x 4 elements = 8 388 608: 300 float4s for a second trip, a tail of 3), range 1
holds 7 elements further on, a gap lies between them and behind them. The sum of squares caps a range at 1 024 blocks = 1 048 576
elements and runs on the first 1 048 576 + 4 * 300 + 3 elements of range 0.

What is asserted: the three update launches give goalnet_adam_step's bits, run range by range; the accumulate pass the two torch
operations' bits; the exchange is exact and its own inverse; the average's copy is exact and its averaging step the correctly rounded
fmaf(w, p - e, e) (to within the fp64 restatement's own rounding, see _fma_bound); the sum of squares is within n * 2^-53 (relative) of
torch's fp64 sum and repeats its bits. Everything outside the ranges keeps its bits, and so do the bands."""
import ctypes

import pytest
import torch

pytestmark = pytest.mark.gpu

if not torch.cuda.is_available():
    pytest.skip("no GPU", allow_module_level=True)

from _abi_guard import Bands, bits_equal, ptr          # noqa: E402
from cvml_goalnet_amd import _lib                       # noqa: E402

DEV = "cuda:0"
CAP = 8192 * 256 * 4
BIG = CAP + 4 * 300 + 3
RANGES = [(64, BIG), (64 + BIG + 61, 7)]                # 64 + BIG + 61 = 8 389 936, a multiple of 4: a gap of 61 elements
TOTAL = RANGES[1][0] + 7 + 29
SS_CAP = 1024 * 256 * 4
SS_RANGES = [(64, SS_CAP + 4 * 300 + 3), RANGES[1]]
HYPER = (1e-3, 0.9, 0.999, 1e-8)
GS = 0.5
STEPS = 3
assert all(b % 4 == 0 for b, _ in RANGES) and RANGES[0][0] + BIG < RANGES[1][0] and RANGES[1][0] + 7 < TOTAL


def _stream():
    return torch.cuda.current_stream().cuda_stream


def _arr(struct, ranges, *rest):
    return (struct * len(ranges))(*[struct(b, c, 0, *rest) for b, c in ranges])


def _inside(ranges=RANGES):
    m = torch.zeros(TOTAL, dtype=torch.bool, device=DEV)
    for b, c in ranges:
        m[b:b + c] = True
    return m


@pytest.fixture(scope="module")
def data():
    g = torch.Generator(device=DEV).manual_seed(77)
    return {"p": torch.randn(TOTAL, device=DEV, generator=g), "g": torch.randn(TOTAL, device=DEV, generator=g) * 3,
            "m": torch.randn(TOTAL, device=DEV, generator=g) * 0.1, "v": torch.rand(TOTAL, device=DEV, generator=g) * 0.01}


@pytest.fixture(scope="module")
def adam_want(data):
    """three steps of goalnet_adam_step (host count) on each range, on a private copy: computed once, never written again"""
    lib = _lib.load()
    t = {k: v.clone() for k, v in data.items()}
    for step in range(1, STEPS + 1):
        for b, c in RANGES:
            p, g, m, v = (t[x][b:b + c] for x in "pgmv")
            assert p.data_ptr() % 16 == 0
            assert lib.goalnet_adam_step(ptr(p), ptr(g), ptr(m), ptr(v), c, *HYPER, step, GS, _stream()) == 0, lib.goalnet_last_error()
    torch.cuda.synchronize()
    assert not bits_equal(t["p"], data["p"]) and bits_equal(t["g"], data["g"])
    return t


def _three_steps(data, adam_want, launch):
    lib = _lib.load()
    bands = Bands(DEV)
    t = {k: bands.place(v, k) for k, v in data.items()}
    step = torch.zeros(1, dtype=torch.int64, device=DEV)
    for _ in range(STEPS):
        assert launch(lib, t, step) == 0, lib.goalnet_last_error()
        step += 1
    bands.assert_bands_intact()
    for k in "pgmv":
        assert bits_equal(t[k], adam_want[k]), k          # outside the ranges too: `adam_want` holds the untouched input there


def test_adam_step_dev_ranges_beyond_the_cap(data, adam_want):
    arr = _arr(_lib.AdamRange, RANGES)
    _three_steps(data, adam_want, lambda lib, t, step: lib.goalnet_adam_step_dev_ranges(
        ptr(t["p"]), ptr(t["g"]), ptr(t["m"]), ptr(t["v"]), arr, len(RANGES), *HYPER, ptr(step), GS, None, 0, 0, 0, None, _stream()))


def _opts_off():
    return _lib.OptimOpts(*HYPER, 0.0, 0.0, 0.0, 0.0, 0, 0, 0, 0, 0)


def test_optim_step_dev_ranges_with_every_option_off_beyond_the_cap(data, adam_want):
    arr, opts = _arr(_lib.OptimRange, RANGES, 0, 0), _opts_off()
    _three_steps(data, adam_want, lambda lib, t, step: lib.goalnet_optim_step_dev_ranges(
        ptr(t["p"]), ptr(t["g"]), ptr(t["m"]), ptr(t["v"]), arr, len(RANGES), ctypes.byref(opts), ptr(step), GS, None, None, 0, 0, 0, None,
        _stream()))


def test_group_step_dev_ranges_with_one_plain_group_beyond_the_cap(data, adam_want):
    arr, opts = _arr(_lib.GroupRange, RANGES, 0, 0), _opts_off()
    table = (_lib.GroupHyper * 1)(_lib.GroupHyper(*HYPER, 0.0, 0, 0))
    _three_steps(data, adam_want, lambda lib, t, step: lib.goalnet_group_step_dev_ranges(
        ptr(t["p"]), ptr(t["g"]), ptr(t["m"]), ptr(t["v"]), None, arr, len(RANGES), table, 1, ctypes.byref(opts), ptr(step), GS, None, None,
        0, 0, 0, None, _stream()))


def test_grad_accum_first_then_later_beyond_the_cap(data):
    lib = _lib.load()
    c = ctypes.c_float(1.0 / 3.0).value
    arr, inside = _arr(_lib.AdamRange, RANGES), _inside()
    old = data["m"].clone()
    old[RANGES[0][0]] = float("nan")                     # the first call does not read the accumulator
    bands = Bands(DEV)
    acc, g1, g2 = bands.place(old, "acc"), bands.place(data["g"], "g1"), bands.place(data["p"], "g2")
    assert lib.goalnet_grad_accum_dev_ranges(ptr(acc), ptr(g1), arr, len(RANGES), c, 1, _stream()) == 0, lib.goalnet_last_error()
    want1 = torch.where(inside, data["g"] * c, old)
    assert bits_equal(acc, want1), "first"
    assert lib.goalnet_grad_accum_dev_ranges(ptr(acc), ptr(g2), arr, len(RANGES), c, 0, _stream()) == 0, lib.goalnet_last_error()
    t = data["p"] * c
    assert bits_equal(acc, torch.where(inside, want1 + t, old)), "later"
    assert bits_equal(g1, data["g"]) and bits_equal(g2, data["p"]), "the gradients are read only"
    bands.assert_bands_intact()


def test_swap_ranges_beyond_the_cap(data):
    lib = _lib.load()
    arr, inside = _arr(_lib.AdamRange, RANGES), _inside()
    bands = Bands(DEV)
    a, b = bands.place(data["p"], "a"), bands.place(data["g"], "b")
    assert lib.goalnet_swap_ranges(ptr(a), ptr(b), arr, len(RANGES), _stream()) == 0, lib.goalnet_last_error()
    assert bits_equal(a, torch.where(inside, data["g"], data["p"])) and bits_equal(b, torch.where(inside, data["p"], data["g"]))
    assert lib.goalnet_swap_ranges(ptr(a), ptr(b), arr, len(RANGES), _stream()) == 0, lib.goalnet_last_error()
    assert bits_equal(a, data["p"]) and bits_equal(b, data["g"]), "twice is the identity"
    bands.assert_bands_intact()


def _fma_bound(r):
    """fmaf rounds the exact w d + e once: the fp32 result r is within half an fp32 ulp of it (2^(exp - 25) with |r| = m 2^exp,
    1/2 <= m < 1). The fp64 restatement w d + e (the product of two fp32 values is exact there) rounds the same exact value to within
    2^-53 |x| <= 2^-52 |r|. Their distance is at most the sum."""
    exp = torch.frexp(r).exponent.clamp(min=-125)
    return torch.ldexp(torch.ones_like(r, dtype=torch.float64), exp - 25) + 2.0 ** -52 * r.abs().double()


def test_ema_copy_and_average_beyond_the_cap(data):
    lib = _lib.load()
    arr, inside = _arr(_lib.AdamRange, RANGES), _inside()
    bands = Bands(DEV)
    p, e = bands.place(data["p"], "p"), bands.place(data["g"], "e")
    step = torch.zeros(1, dtype=torch.int64, device=DEV)

    copy = _lib.EmaOpts(0.9, 1, 5, 0, 0)                  # t = 1 <= start_step: the average tracks the weights
    assert lib.goalnet_ema_update_dev_ranges(ptr(p), ptr(e), arr, len(RANGES), ctypes.byref(copy), ptr(step), 1, None, _stream()) == 0
    assert bits_equal(e, torch.where(inside, data["p"], data["g"])), "copy"

    e.copy_(data["g"])
    avg = _lib.EmaOpts(0.9, 1, 0, 0, 0)                   # t = 1, the first averaging update: w = (float)(1 - 0.9)
    assert lib.goalnet_ema_update_dev_ranges(ptr(p), ptr(e), arr, len(RANGES), ctypes.byref(avg), ptr(step), 1, None, _stream()) == 0
    w = ctypes.c_float(1.0 - 0.9).value
    d = data["p"] - data["g"]                             # p - e, rounded to fp32 as the kernel's operand is
    x = w * d.double() + data["g"].double()
    err, bound = (e.double() - x).abs()[inside], _fma_bound(e)[inside]
    exact = int((e[inside] == x.float()[inside]).sum())
    print(f"ema average: worst |e - x| / bound = {float((err / bound).max()):.3f}; {exact} of {int(inside.sum())} equal (float)x")
    assert bool((err <= bound).all())
    assert bits_equal(e[~inside], data["g"][~inside]) and bits_equal(p, data["p"])
    bands.assert_bands_intact()


def test_grad_sumsq_beyond_its_cap(data):
    lib = _lib.load()
    arr = _arr(_lib.OptimRange, SS_RANGES, 0, 0)
    nbytes = lib.goalnet_grad_sumsq_ws_bytes(arr, len(SS_RANGES))
    assert nbytes == 8 * (1024 + 1)                       # the long range at its cap, one block for the 7 elements
    bands = Bands(DEV)
    g = bands.place(data["g"], "g")
    ws, out = bands.guarded(nbytes // 8, torch.float64, name="ws"), bands.guarded(2, torch.float64, name="out")
    for k in range(2):
        rc = lib.goalnet_grad_sumsq(ptr(g), arr, len(SS_RANGES), ptr(out[k:]), ptr(ws), nbytes, _stream())
        assert rc == 0, lib.goalnet_last_error()
    n = sum(c for _, c in SS_RANGES)
    want = sum(float((data["g"][b:b + c].double() ** 2).sum()) for b, c in SS_RANGES)
    rel = abs(float(out[0]) - want) / want
    print(f"grad_sumsq over {n} elements: relative error {rel:.3e}, bound {n * 2.0 ** -53:.3e}")
    assert rel <= n * 2.0 ** -53
    assert bits_equal(out[0], out[1]), "a second call gives the same bits"
    assert bits_equal(g, data["g"])
    bands.assert_bands_intact()
