"""GPU: goalnet_adam_step_dev_ranges through the raw C ABI, in guard-banded buffers (tests/_abi_guard.py). Element for element the result
is that of goalnet_adam_step_dev applied to each range with step_bias = 1 - skipped; gaps between the ranges and the bands are untouched."""
import pytest
import torch

pytestmark = pytest.mark.gpu

if not torch.cuda.is_available():
    pytest.skip("no GPU", allow_module_level=True)

from _abi_guard import Bands, bits_equal, ptr                      # noqa: E402
from cvml_goalnet_amd import _lib                                  # noqa: E402

DEV = "cuda:0"
N = 10000
HYPER = (1e-3, 0.9, 0.999, 1e-8)
STEP0 = 40                                     # completed steps on the device counter; every `skipped` below is smaller
GS = 0.5


def _ranges(count):
    if count == 1:
        return [(8, 9992, 3)]                                        # ends at the buffer's end
    if count == 3:
        return [(0, 4, 0), (64, 1001, 7), (9000, 1000, 40)]         # a 4-element range, an odd length, one ending at the end (t = 1)
    out, b = [], 0
    for r in range(32):                                              # 32 ranges of assorted lengths with gaps of 4 .. 28 elements
        c = 4 if r == 5 else 37 + 17 * r
        out.append((b, c, r))
        b += (c + 3) // 4 * 4 + 4 * (1 + r % 7)
    out[-1] = (out[-1][0], N - out[-1][0], 31)
    assert out[-1][1] > 0
    return out


@pytest.fixture(scope="module")
def data():
    g = torch.Generator().manual_seed(5)
    return {"p": torch.randn(N, generator=g), "g": torch.randn(N, generator=g) * 3, "m": torch.randn(N, generator=g) * 0.1,
            "v": torch.rand(N, generator=g) * 0.01}


def _place(data):
    bands = Bands(DEV)
    return bands, {k: bands.place(t, k) for k, t in data.items()}


def _expected(data, ranges, lib):
    """goalnet_adam_step_dev on each range with step_bias = 1 - skipped, on a private copy"""
    t = {k: v.to(DEV).clone() for k, v in data.items()}
    step = torch.tensor([STEP0], dtype=torch.int64, device=DEV)
    for b, c, k in ranges:
        p, g, m, v = (t[x][b:b + c] for x in "pgmv")
        assert p.data_ptr() % 16 == 0
        assert lib.goalnet_adam_step_dev(ptr(p), ptr(g), ptr(m), ptr(v), c, *HYPER, ptr(step), 1 - k, GS, None) == 0
    torch.cuda.synchronize()
    return t


def _call(lib, t, ranges, step, shadow=None, sh_begin=0, f16=0, bad=None):
    arr = (_lib.AdamRange * len(ranges))(*[_lib.AdamRange(*r) for r in ranges])
    return lib.goalnet_adam_step_dev_ranges(ptr(t["p"]), ptr(t["g"]), ptr(t["m"]), ptr(t["v"]), arr, len(ranges), *HYPER, ptr(step), GS,
                                            ptr(shadow), sh_begin, 0 if shadow is None else shadow.numel(), f16, ptr(bad), None)


@pytest.mark.parametrize("count", [1, 3, 32])
def test_ranges_equal_the_single_range_kernel_and_touch_nothing_else(data, count):
    lib = _lib.load()
    ranges = _ranges(count)
    want = _expected(data, ranges, lib)
    bands, t = _place(data)
    step = torch.tensor([STEP0], dtype=torch.int64, device=DEV)
    assert _call(lib, t, ranges, step) == 0, lib.goalnet_last_error()
    bands.assert_bands_intact()
    for k in "pgmv":
        assert bits_equal(t[k], want[k]), k             # the gaps too: `want` holds the untouched input there
    assert int(step) == STEP0
    touched = torch.zeros(N, dtype=torch.bool)
    for b, c, _ in ranges:
        touched[b:b + c] = True
    assert not torch.equal(t["p"].cpu(), data["p"]) and torch.equal(t["p"].cpu()[~touched], data["p"][~touched])


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16])
def test_shadow_slice_and_guard(data, dtype):
    lib = _lib.load()
    ranges = _ranges(3)
    want = _expected(data, ranges, lib)
    sh_begin, sh_count = 200, 400                        # inside the second range
    step = torch.tensor([STEP0], dtype=torch.int64, device=DEV)
    f16 = int(dtype == torch.float16)

    # a stamped step (bad_step == *step + 1, whatever the ranges' own counts are) leaves everything untouched
    bands, t = _place(data)
    shadow = bands.guarded(sh_count, dtype, name="shadow")
    pristine = shadow.clone()
    bad = torch.tensor([STEP0 + 1], dtype=torch.int64, device=DEV)
    assert _call(lib, t, ranges, step, shadow, sh_begin, f16, bad) == 0, lib.goalnet_last_error()
    bands.assert_bands_intact()
    assert all(bits_equal(t[k].cpu(), data[k]) for k in "pgmv") and bits_equal(shadow, pristine)

    # another step's stamp does not: the update runs and the shadow holds the cast of the new parameters
    bad.fill_(STEP0 + 1 - 7)                             # the second range's own t: the guard must not compare against it
    assert _call(lib, t, ranges, step, shadow, sh_begin, f16, bad) == 0, lib.goalnet_last_error()
    bands.assert_bands_intact()
    for k in "pgmv":
        assert bits_equal(t[k], want[k]), k
    assert bits_equal(shadow, t["p"][sh_begin:sh_begin + sh_count].to(dtype))
