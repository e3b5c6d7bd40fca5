"""GPU: the Adam / overflow-guard entry points of include/goalnet_hip.h, called through the raw C ABI.

What the header promises besides values: the five doors to the one Adam kernel give the same bits; the shadow variant writes
the 16-bit copy of exactly one slice; the guard stamps on inf / nan only, skips the stamped step completely and lets the retry
run under the same count. Every buffer the kernels may write sits between guard bands (tests/_abi_guard.py)."""
import math

import pytest
import torch

from _abi_guard import Bands, bits_equal, ptr
from cvml_goalnet_amd import _lib

pytestmark = pytest.mark.gpu

LR, B1, B2, EPS = 1e-3, 0.9, 0.999, 1e-8
FLT_MAX = 3.4028234663852886e38


def _s():
    return torch.cuda.current_stream().cuda_stream


def _ok(rc, what):
    _lib.check(rc, what)


def _i64(*vals):
    return torch.tensor(list(vals), dtype=torch.int64, device="cuda")


def _state(n, seed):
    gen = torch.Generator().manual_seed(seed)
    p = torch.randn(n, generator=gen)
    m = torch.randn(n, generator=gen) * 0.01
    v = torch.rand(n, generator=gen) * 1e-4
    gs = [torch.randn(n, generator=gen) * (0.1 ** k) for k in range(3)]
    return p, m, v, gs


def _adam_host(lib, p, g, m, v, step, gs=0.5):
    _ok(lib.goalnet_adam_step(ptr(p), ptr(g), ptr(m), ptr(v), p.numel(), LR, B1, B2, EPS, step, gs, _s()), "adam_step")


# ---------------------------------------------------------------------------------------------------------------------------
# 1. one kernel, five doors
# ---------------------------------------------------------------------------------------------------------------------------
DOORS = ["dev", "blocks1", "blocks7", "blocks128", "shadow", "guarded", "guarded_shadow"]


# a shadowed slice is a positive multiple of 4 elements: none fits into n = 3, so the shadow doors start at n = 4
@pytest.mark.parametrize("n,door", [(n, d) for n in (3, 4, 1003, 100003, (1 << 20) + 8) for d in DOORS if n >= 4 or "shadow" not in d])
def test_every_door_gives_the_bits_of_adam_step(n, door):
    """three steps with grad_scale 0.5: p, m, v of each device-step door == those of goalnet_adam_step, bit for bit. n = 3 leaves
    the float4 body empty (one block, tail lanes only); a shadow slice needs four elements, so the shadow doors start at n = 4."""
    lib = _lib.load()
    p0, m0, v0, gs = _state(n, 1234 + n)
    ref = [t.cuda() for t in (p0, m0, v0)]
    for k, g in enumerate(gs):
        _adam_host(lib, ref[0], g.cuda(), ref[1], ref[2], k + 1)

    bands = Bands()
    p, m, v = bands.place(p0, "p"), bands.place(m0, "m"), bands.place(v0, "v")
    step, bad = _i64(0), _i64(0)
    n4 = n & ~3
    shadow = bands.guarded(n4, torch.bfloat16, name="shadow") if "shadow" in door else None
    for k, g in enumerate(gs):
        gd = bands.place(g, f"g{k}")
        step.fill_(k)                              # the counter holds the completed steps; bias 1 makes the 1-based count
        head = (ptr(p), ptr(gd), ptr(m), ptr(v), n, LR, B1, B2, EPS, ptr(step), 1, 0.5)
        if door == "dev":
            rc = lib.goalnet_adam_step_dev(*head, _s())
        elif door.startswith("blocks"):
            rc = lib.goalnet_adam_step_dev_blocks(*head, int(door[6:]), _s())
        elif door == "shadow":
            rc = lib.goalnet_adam_step_dev_shadow(*head, ptr(shadow), 0, n4, 0, _s())
        elif door == "guarded":
            rc = lib.goalnet_adam_step_dev_guarded(*head, 0, 0, 0, 0, ptr(bad), _s())
        else:
            rc = lib.goalnet_adam_step_dev_guarded(*head, ptr(shadow), 0, n4, 0, ptr(bad), _s())
        _ok(rc, door)
    bands.assert_bands_intact()
    for name, got, want in zip("pmv", (p, m, v), ref):
        assert bits_equal(got, want), f"{door}, n = {n}: {name} differs from goalnet_adam_step in {(got != want).sum().item()} elements"
    if shadow is not None:
        assert bits_equal(shadow, p[:n4].to(torch.bfloat16))


# ---------------------------------------------------------------------------------------------------------------------------
# 2. shadow slice
# ---------------------------------------------------------------------------------------------------------------------------
def _slices(n):
    n4 = n & ~3
    return [(0, 4), (4, n4 - 4), (n4 - 4, 4), (0, n4)]


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16], ids=["bf16", "fp16"])
@pytest.mark.parametrize("n", [1003, 4096])
@pytest.mark.parametrize("which", range(4))
def test_shadow_is_the_rounded_slice_and_nothing_else(n, which, dtype):
    """shadow == p_new[begin : begin + count].to(dtype) (round to nearest even) and every byte around it is untouched. p, g, m, v
    are views at a non-zero 16-byte-aligned offset of larger arenas (as AVM._adam_piece passes them); the arenas outside the views
    keep their bits."""
    lib = _lib.load()
    begin, count = _slices(n)[which]
    off = 68                                       # floats: 272 bytes, a multiple of 16
    gen = torch.Generator().manual_seed(99 + n + which)
    arenas = [torch.randn(n + 2 * off, generator=gen).cuda() for _ in range(4)]
    arenas[3].abs_().mul_(1e-3)                    # v >= 0
    if dtype is torch.float16:
        arenas[0].mul_(100.0)                      # some magnitudes with few fp16 bits behind the point, some subnormal
        arenas[0][off:off + 8] = torch.tensor([6.1e-5, -6.0e-8, 65504.0, -65519.0, 1e-9, 0.0, -0.0, 2049.0])
    before = [a.clone() for a in arenas]
    p, g, m, v = (a[off:off + n] for a in arenas)
    assert all(t.data_ptr() % 16 == 0 for t in (p, g, m, v))
    bands = Bands()
    shadow = bands.guarded(count, dtype, name="shadow")
    step = _i64(4)
    _ok(lib.goalnet_adam_step_dev_shadow(ptr(p), ptr(g), ptr(m), ptr(v), n, LR, B1, B2, EPS, ptr(step), 1, 1.0, ptr(shadow), begin, count,
                                         int(dtype is torch.float16), _s()), "adam_step_dev_shadow")
    bands.assert_bands_intact()
    assert bits_equal(shadow, p[begin:begin + count].to(dtype))
    want = [b.clone() for b in before]
    _adam_host(lib, want[0][off:off + n], want[1][off:off + n], want[2][off:off + n], want[3][off:off + n], 5, gs=1.0)
    for name, a, b, w in zip("pgmv", arenas, before, want):
        assert bits_equal(a[:off], b[:off]) and bits_equal(a[off + n:], b[off + n:]), f"arena of {name} touched outside the view"
        assert bits_equal(a, w), f"{name}: the shadowed step differs from goalnet_adam_step"


# ---------------------------------------------------------------------------------------------------------------------------
# 3. guard
# ---------------------------------------------------------------------------------------------------------------------------
GRID_SPAN = 1024 * 256                             # threads of the check's largest grid: beyond it the grid-stride loop runs
WHERE = {"first": (1000, 0), "last": (1000, 999), "last_ragged": (1003, 1002), "past_grid": (GRID_SPAN + 5003, GRID_SPAN + 4999)}


def _check(lib, g, step, bad, skipped, bias=1):
    _ok(lib.goalnet_grad_finite_check(ptr(g), g.numel(), ptr(step), bias, ptr(bad), ptr(skipped), _s()), "grad_finite_check")


@pytest.mark.parametrize("value", [math.inf, -math.inf, math.nan], ids=["+inf", "-inf", "nan"])
@pytest.mark.parametrize("where", list(WHERE))
@pytest.mark.parametrize("many", [False, True], ids=["one", "many"])
def test_finite_check_stamps_once_per_step(where, value, many):
    """a non-finite gradient stamps bad_step = step + bias and adds exactly 1 to skipped, however many elements (and waves) see it;
    a second check in the same step adds nothing, a later step adds again; skipped = NULL is accepted"""
    lib = _lib.load()
    n, pos = WHERE[where]
    bands = Bands()
    host = torch.randn(n, generator=torch.Generator().manual_seed(n + pos))
    host[pos] = value
    if many:
        host[pos % 7::7] = value                   # every block of the grid sees some
    g = bands.place(host, "g")
    state = bands.guarded(3, torch.int64, fill=torch.tensor([7, 0, 5]), name="step|bad|skipped")
    step, bad, skipped = state[0:1], state[1:2], state[2:3]
    _check(lib, g, step, bad, skipped)
    assert state.tolist() == [7, 8, 6]
    _check(lib, g, step, bad, skipped)
    assert state.tolist() == [7, 8, 6], "a second check in the same step must not count again"
    step.fill_(8)
    _check(lib, g, step, bad, skipped)
    assert state.tolist() == [8, 9, 7], "a later step must count again"
    step.fill_(11)
    _check(lib, g, step, bad, None, bias=3)
    assert state.tolist() == [11, 14, 7]
    bands.assert_bands_intact()


@pytest.mark.parametrize("n", [4, 1003, GRID_SPAN + 5003])
def test_finite_check_leaves_finite_gradients_alone(n):
    """the header: the guard fires on "an inf / nan". FLT_MAX, -FLT_MAX, the subnormals and signed zeros are finite."""
    lib = _lib.load()
    bands = Bands()
    host = torch.randn(n, generator=torch.Generator().manual_seed(n)) * 1e30
    host[0], host[n - 1], host[n // 2], host[1], host[2] = FLT_MAX, -FLT_MAX, 1e-45, 3.0e38, -0.0
    assert torch.isfinite(host).all()
    g = bands.place(host, "g")
    state = bands.guarded(3, torch.int64, fill=torch.tensor([7, 0, 5]), name="step|bad|skipped")
    _check(lib, g, state[0:1], state[1:2], state[2:3])
    assert state.tolist() == [7, 0, 5], "a finite gradient was stamped as overflow"
    bands.assert_bands_intact()


@pytest.mark.parametrize("tick", ["counters_add4_guarded", "rows_scatter_tick"])
@pytest.mark.parametrize("with_shadow", [False, True], ids=["plain", "shadow"])
def test_stamped_step_is_skipped_and_retried_under_the_same_count(tick, with_shadow):
    lib = _lib.load()
    n = 1003
    p0, m0, v0, gs = _state(n, 77)
    bands = Bands()
    p, m, v = bands.place(p0, "p"), bands.place(m0, "m"), bands.place(v0, "v")
    n4 = n & ~3
    shadow = bands.guarded(n4, torch.float16, fill=1.5, name="shadow") if with_shadow else None
    counters = bands.guarded(4, torch.int64, fill=torch.tensor([7, 3, 20, 2]), name="counters")
    flags = bands.guarded(2, torch.int64, fill=0, name="bad|skipped")
    bad, skipped = flags[0:1], flags[1:2]
    table = bands.guarded((8, 4), torch.float32, fill=-1.0, name="table")
    block = torch.arange(8, dtype=torch.float32, device="cuda").view(2, 4)

    def guarded_step(g):
        _check(lib, g, counters[0:1], bad, skipped)
        _ok(lib.goalnet_adam_step_dev_guarded(ptr(p), ptr(g), ptr(m), ptr(v), n, LR, B1, B2, EPS, ptr(counters), 1, 0.5, ptr(shadow), 0,
                                              n4 if with_shadow else 0, 1, ptr(bad), _s()), "adam_step_dev_guarded")
        if tick == "counters_add4_guarded":
            _ok(lib.goalnet_counters_add4_guarded(ptr(counters), 1, 1, 10, 1, ptr(bad), _s()), tick)
        else:
            seg = (_lib.RowCopy * 1)(_lib.RowCopy(ptr(block), ptr(table), 16, 2, 0, ptr(counters[3:4]), 0))   # rows [c3, c3 + 2) of the table
            _ok(lib.goalnet_rows_scatter_tick(seg, 1, ptr(counters), 1, 1, 10, 1, ptr(bad), _s()), tick)

    overflowed = gs[0].clone()
    overflowed[n - 1] = math.inf
    guarded_step(bands.place(overflowed, "g_inf"))
    for name, got, want in zip("pmv", (p, m, v), (p0, m0, v0)):
        assert bits_equal(got.cpu(), want), f"{name} moved in a stamped step"
    if with_shadow:
        assert bits_equal(shadow.cpu(), torch.full((n4,), 1.5, dtype=torch.float16)), "the shadow was written in a stamped step"
    assert counters.tolist() == [7, 4, 30, 3], "a stamped step holds counter 0 and advances counters 1..3"
    assert flags.tolist() == [0, 1], "the stamp is cleared by the step's last launch; the skip is counted once"

    guarded_step(bands.place(gs[1], "g_ok"))       # the retry: same count (8), judged on its own gradients
    assert counters.tolist() == [8, 5, 40, 4] and flags.tolist() == [0, 1]
    ref = [t.cuda() for t in (p0, m0, v0)]
    _adam_host(lib, ref[0], gs[1].cuda(), ref[1], ref[2], 8)
    for name, got, want in zip("pmv", (p, m, v), ref):
        assert bits_equal(got, want), f"{name}: the retry differs from an unguarded step at the same count"
    if with_shadow:
        assert bits_equal(shadow, p[:n4].to(torch.float16))
    if tick == "rows_scatter_tick":
        want = torch.full((8, 4), -1.0)
        want[2:4] = block.cpu()                    # first tick: cursor 2 (read before the counters move)
        want[3:5] = block.cpu()                    # second tick: cursor 3
        assert bits_equal(table.cpu(), want)
    bands.assert_bands_intact()


# ---------------------------------------------------------------------------------------------------------------------------
# 4. long horizon against fp64
# ---------------------------------------------------------------------------------------------------------------------------
N_LONG, STEPS, MARKS = 4099, 300, (1, 10, 100, 300)


def long_gradient(t):
    """step t's gradient (1-based): seeded normal values whose scale drifts over three decades, elements 0..99 exactly zero at
    every step, 100..199 one constant each, and a tenth of the rest exactly zero at random steps"""
    gen = torch.Generator().manual_seed(5000 + t)
    g = torch.randn(N_LONG, generator=gen) * (10.0 ** (-3.0 * t / STEPS))
    g[torch.rand(N_LONG, generator=gen) < 0.1] = 0.0
    g[:100] = 0.0
    g[100:200] = torch.linspace(-2.0, 2.0, 100)
    return g


def long_start():
    return torch.randn(N_LONG, generator=torch.Generator().manual_seed(4099))


def adam_fp64(p, g, m, v, t):
    """torch.optim.Adam's _single_tensor_adam (defaults: no weight decay, no amsgrad) in double, operation by operation"""
    m += (g - m) * (1.0 - B1)                      # exp_avg.lerp_(grad, 1 - beta1)
    v *= B2
    v += (1.0 - B2) * g * g                        # exp_avg_sq.mul_(beta2).addcmul_(grad, grad, value = 1 - beta2)
    step_size = LR / (1.0 - B1 ** t)
    denom = v.sqrt() / math.sqrt(1.0 - B2 ** t) + EPS
    p -= step_size * (m / denom)                   # param.addcdiv_(exp_avg, denom, value = -step_size)


def update_direction(m, v, t):
    """m / (sqrt(v) / sqrt(1 - b2^t) + eps) in double from a state in any precision: the bias-correction-sensitive quantity"""
    m, v = m.double(), v.double()
    return m / (v.sqrt() / math.sqrt(1.0 - B2 ** t) + EPS)


def fp64_marks():
    p = long_start().double()
    m, v = torch.zeros_like(p), torch.zeros_like(p)
    out = {}
    for t in range(1, STEPS + 1):
        adam_fp64(p, long_gradient(t).double(), m, v, t)
        if t in MARKS:
            out[t] = (p.clone(), update_direction(m, v, t))
    return out


def torch_fp32_marks():
    """torch.optim.Adam itself, fp32 on the CPU, single-tensor path: the reference's own arithmetic"""
    p = long_start().clone().requires_grad_(True)
    opt = torch.optim.Adam([p], lr=LR, betas=(B1, B2), eps=EPS, foreach=False)
    out = {}
    for t in range(1, STEPS + 1):
        p.grad = long_gradient(t)
        opt.step()
        if t in MARKS:
            st = opt.state[p]
            out[t] = (p.detach().clone(), update_direction(st["exp_avg"], st["exp_avg_sq"], t))
    return out


def distances(marks, ref):
    return {t: tuple((a.double() - b).abs().max().item() for a, b in zip(marks[t], ref[t])) for t in MARKS}


def test_three_hundred_steps_stay_within_twice_torch_fp32_of_fp64():
    """300 steps of goalnet_adam_step_dev on 4 099 parameters (counter-driven, so the fp64 bias corrections run to t = 300) against
    the fp64 restatement above, at steps 1, 10, 100 and 300: max |p - p64| and max |u - u64| with u = m / (sqrt(v) / sqrt(1 - b2^t) +
    eps).

    Bound = FACTOR x the distance of torch.optim.Adam (fp32, CPU, foreach = False) from the same fp64 run, computed in this test
    from the same gradients. FACTOR = 2: the kernel's operation order is torch's, and only the contraction of v * b2 + (omb2 * g) * g
    (and of the two other multiply-adds) into fused operations may differ. torch's distances, measured on the CPU (x86-64, torch
    2.10; they do not involve the code under test):

        step      max |p - p64|     max |u - u64|
           1      7.248e-08         8.722e-09
          10      7.247e-07         1.285e-07
         100      7.247e-06         1.018e-06
         300      2.174e-05         3.510e-06
    """
    FACTOR = 2.0
    lib = _lib.load()
    ref = fp64_marks()
    allowed = distances(torch_fp32_marks(), ref)
    bands = Bands()
    p = bands.place(long_start(), "p")
    m, v = bands.guarded(N_LONG, torch.float32, fill=0.0, name="m"), bands.guarded(N_LONG, torch.float32, fill=0.0, name="v")
    step = _i64(0)
    got = {}
    for t in range(1, STEPS + 1):
        g = long_gradient(t).cuda()
        _ok(lib.goalnet_adam_step_dev(ptr(p), ptr(g), ptr(m), ptr(v), N_LONG, LR, B1, B2, EPS, ptr(step), 1, 1.0, _s()), "adam_step_dev")
        _ok(lib.goalnet_counter_add(ptr(step), 1, _s()), "counter_add")
        if t in MARKS:
            got[t] = (p.cpu(), update_direction(m.cpu(), v.cpu(), t))
    bands.assert_bands_intact()
    mine = distances(got, ref)
    for t in MARKS:
        print(f"step {t:3d}: |p - p64| kernel {mine[t][0]:.3e} torch-fp32 {allowed[t][0]:.3e}; |u - u64| kernel {mine[t][1]:.3e} "
              f"torch-fp32 {allowed[t][1]:.3e}")
    for t in MARKS:
        assert mine[t][0] <= FACTOR * allowed[t][0], f"step {t}: p is {mine[t][0]:.3e} from fp64, torch's fp32 Adam {allowed[t][0]:.3e}"
        assert mine[t][1] <= FACTOR * allowed[t][1], f"step {t}: m / denom is {mine[t][1]:.3e} from fp64, torch's fp32 Adam {allowed[t][1]:.3e}"
