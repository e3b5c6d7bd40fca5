"""GPU: goalnet_grad_accum_dev_ranges (include/goalnet_accum.h) through the raw C ABI, between guard bands
(tests/_abi_guard.py). Every case is two calls on the same device data — first = 1, then first = 0, with c = (float)(1 / 3) — and the
accumulator is compared BIT FOR BIT with the two torch operations the header names, on the same device tensors: t = g * c; acc + t.
Everything outside the ranges — the gaps between two ranges, the slack behind the last — keeps the bits it had.

Shapes: the smallest at which each path of the kernel can go wrong. A range of 1 or 3 elements is tail only; 4 is one 16-byte access and
no tail; 5 is both; 1 023 leaves the last wave of a block partly idle and has a tail of 3. Three ranges with gaps: the block-to-range
search, one range shorter than a block. The last case is long enough for the per-range block cap (8 192 blocks of 256 threads x 4
elements) to be reached, so that a block's grid-stride loop takes a second trip, plus a tail of 3."""
import ctypes

import pytest
import torch

pytestmark = pytest.mark.gpu

if not torch.cuda.is_available():
    pytest.skip("no GPU", allow_module_level=True)

from _abi_guard import Bands, bits_equal, ptr          # noqa: E402
from cvml_goalnet_amd import _lib, ops                  # noqa: E402

DEV = "cuda:0"
C = ctypes.c_float(1.0 / 3.0).value                     # (float)(1.0 / 3)
CAP_ELEMS = 8192 * 256 * 4                              # what the blocks of one range cover in one trip of their loops

CASES = [
    ("one-1", 16, [(0, 1)]),
    ("one-3", 16, [(4, 3)]),
    ("one-4", 16, [(8, 4)]),
    ("one-5", 16, [(4, 5)]),
    ("one-1023", 1100, [(64, 1023)]),
    ("three-with-gaps", 4096, [(0, 70), (128, 2050), (2304, 1500)]),
    ("second-trip-tail-3", CAP_ELEMS + 1024 + 3 + 64, [(64, CAP_ELEMS + 1024 + 3)]),
]


def _call(acc, g, ranges, first):
    arr = (_lib.AdamRange * len(ranges))(*[_lib.AdamRange(b, n, 0) for b, n in ranges])
    rc = _lib.load().goalnet_grad_accum_dev_ranges(ptr(acc), ptr(g), arr, len(ranges), C, first, torch.cuda.current_stream().cuda_stream)
    assert rc == 0, _lib.load().goalnet_last_error()


@pytest.mark.parametrize("what,numel,ranges", CASES, ids=[c[0] for c in CASES])
def test_two_calls_equal_the_two_torch_ops_bit_for_bit(what, numel, ranges):
    gen = torch.Generator(device=DEV).manual_seed(1234 + numel)
    g1 = torch.randn(numel, device=DEV, generator=gen) * torch.exp(4.0 * torch.randn(numel, device=DEV, generator=gen))
    g2 = torch.randn(numel, device=DEV, generator=gen) * torch.exp(4.0 * torch.randn(numel, device=DEV, generator=gen))
    old = torch.randn(numel, device=DEV, generator=gen)              # what a previous window left in the accumulator
    for b, n in ranges:                                              # a NaN there must not survive first = 1: acc is not read
        old[b] = float("nan")
    bands = Bands(DEV)
    acc = bands.place(old, "acc")
    ga, gb = bands.place(g1, "g1"), bands.place(g2, "g2")
    inside = torch.zeros(numel, dtype=torch.bool, device=DEV)
    for b, n in ranges:
        inside[b:b + n] = True

    _call(acc, ga, ranges, 1)
    torch.cuda.synchronize()
    want1 = torch.where(inside, g1 * C, old)
    assert bits_equal(acc, want1), f"{what}: first call"
    _call(acc, gb, ranges, 0)
    torch.cuda.synchronize()
    t = g2 * C
    want2 = torch.where(inside, want1 + t, old)
    assert bits_equal(acc, want2), f"{what}: second call"
    assert bits_equal(ga, g1) and bits_equal(gb, g2), "the gradients are read only"
    bands.assert_bands_intact()
    # the restatement is not the fused multiply-add: somewhere in a range of any length the two differ (1-element ranges: not asserted)
    if inside.sum().item() >= 1023:
        fused = torch.where(inside, torch.addcmul(want1.double(), g2.double(), torch.tensor(float(C), dtype=torch.float64, device=DEV)).float(), old)
        assert not bits_equal(fused, want2), "the data cannot tell a contracted multiply-add from two rounded operations"


def test_ops_wrapper_checks_and_runs():
    g = torch.arange(64, dtype=torch.float32, device=DEV)
    acc = torch.full((64,), 7.0, device=DEV)
    ops.grad_accum_dev_ranges(acc, g, [(0, 10), (32, 6, 0)], 0.5, True)
    ops.grad_accum_dev_ranges(acc, g, [(0, 10), (32, 6, 0)], 0.5, False)
    torch.cuda.synchronize()
    want = torch.full((64,), 7.0, device=DEV)
    want[0:10] = g[0:10]
    want[32:38] = g[32:38]
    assert bits_equal(acc, want)
    with pytest.raises(Exception, match="leaves the arena"):
        ops.grad_accum_dev_ranges(acc, g, [(60, 8)], 0.5, True)
    with pytest.raises(Exception):
        ops.grad_accum_dev_ranges(acc, g[:32], [(0, 8)], 0.5, True)
    assert bits_equal(acc, want)
