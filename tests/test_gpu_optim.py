"""GPU: the kernels of include/goalnet_optim.h (csrc/optim.hip) in guard-banded buffers (tests/_abi_guard.py):
options off equals goalnet_adam_step_dev_ranges bit for bit; the gradient's sum of squares against numpy fp64; three steps of weight
decay and clipping against torch's own optimizers on the CPU; the schedule against its closed form; the guard."""
import math

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

if not torch.cuda.is_available():
    pytest.skip("no GPU", allow_module_level=True)

from _abi_guard import Bands, bits_equal                           # noqa: E402
from cvml_goalnet_amd import ops                                   # noqa: E402
from cvml_goalnet_amd.optim import OptimOptions                    # noqa: E402

DEV = "cuda:0"
HYPER = (1e-3, 0.9, 0.999, 1e-8)
I64 = torch.int64


def rnd(*shape, seed=0, lo=-1.0, hi=1.0):
    g = torch.Generator().manual_seed(seed)
    return (torch.rand(*shape, generator=g, dtype=torch.float64) * (hi - lo) + lo).float()


def _arenas(n, seed):
    return {"p": rnd(n, seed=seed), "g": rnd(n, seed=seed + 1), "m": rnd(n, seed=seed + 2), "v": rnd(n, seed=seed + 3, lo=0.0)}


def _place(data):
    bands = Bands(DEV)
    return bands, {k: bands.place(t, k) for k, t in data.items()}


# ---- 1. options off: goalnet_adam_step_dev_ranges' bits ------------------------------------------------------------------------------------
# a count of 4k + 3 (the tail), a range of 69 blocks that sat two steps out, a range under a 16-bit copy
OFF_RANGES = [(0, 4 * 257 + 3, 0), (2048, 70000, 2), (72064, 8192, 0)]
OFF_N = 72064 + 8192
STEP0 = 40


@pytest.mark.parametrize("stamped", [False, True], ids=["unstamped", "stamped"])
@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16], ids=["bf16", "fp16"])
def test_options_off_is_adam_step_dev_ranges_bit_for_bit(dtype, stamped):
    data = _arenas(OFF_N, 100)
    sh_begin, sh_count = 72064 + 64, 4096
    step = torch.tensor([STEP0], dtype=I64, device=DEV)
    bad = torch.tensor([STEP0 + 1 if stamped else STEP0 - 1], dtype=I64, device=DEV)       # STEP0 - 1: the second range's own count

    want = {k: v.to(DEV).clone() for k, v in data.items()}
    want_sh = torch.zeros(sh_count, dtype=dtype, device=DEV)
    ops.adam_step_dev_ranges(want["p"], want["g"], want["m"], want["v"], OFF_RANGES, *HYPER, step, 0.5, shadow=want_sh, shadow_begin=sh_begin,
                             bad_step=bad)

    # the decay flags are set: without weight_decay they switch nothing on
    for opt in (OptimOptions(), OptimOptions(decoupled=True, no_decay=("bias",), min_lr=1e-5, gamma=0.5)):
        bands, t = _place(data)
        shadow = bands.guarded(sh_count, dtype, fill=0.0, name="shadow")
        ranges = [(b, c, k, r != 1) for r, (b, c, k) in enumerate(OFF_RANGES)]
        ops.optim_step_dev_ranges(t["p"], t["g"], t["m"], t["v"], ranges, *HYPER, opt, step, 0.5, shadow=shadow, shadow_begin=sh_begin, bad_step=bad)
        bands.assert_bands_intact()
        for k in "pgmv":
            assert bits_equal(t[k], want[k]), k
        assert bits_equal(shadow, want_sh)
        assert int(step) == STEP0
        if stamped:
            assert all(bits_equal(t[k].cpu(), data[k]) for k in "pgmv") and not shadow.any()
        else:
            assert not torch.equal(t["p"].cpu(), data["p"]) and bits_equal(shadow, t["p"][sh_begin:sh_begin + sh_count].to(dtype))


def test_undecayed_unclipped_range_under_options_keeps_adams_bits():
    """weight decay on ONE range: the other range runs the plain loop at the same (constant) rate"""
    data = _arenas(4096 + 1031, 120)
    step = torch.tensor([3], dtype=I64, device=DEV)
    want = {k: v.to(DEV).clone() for k, v in data.items()}
    ops.adam_step_dev_ranges(want["p"], want["g"], want["m"], want["v"], [(4096, 1031, 0)], *HYPER, step)
    bands, t = _place(data)
    ops.optim_step_dev_ranges(t["p"], t["g"], t["m"], t["v"], [(0, 4096, 0, True), (4096, 1031, 0, False)], *HYPER,
                              OptimOptions(weight_decay=0.01, decoupled=True), step)
    bands.assert_bands_intact()
    for k in "pmv":
        assert bits_equal(t[k][4096:], want[k][4096:]), k
    assert not bits_equal(t["p"][:4096].cpu(), data["p"][:4096]) and bits_equal(t["g"].cpu(), data["g"])


# ---- 2. the sum of squares -------------------------------------------------------------------------------------------------------------------
SS_SIZES = [1, 3, 4, 1027, 262149]


@pytest.fixture(scope="module")
def ss_case():
    """one arena holding the five ranges with gaps of NaN between them (a read outside a range poisons the sum), magnitudes over 2^+-20"""
    ranges, b = [], 0
    for c in SS_SIZES:
        ranges.append((b, c, 0, False))
        b += (c + 3) // 4 * 4 + 8
    n = b
    g = torch.full((n,), float("nan"))
    gen = torch.Generator().manual_seed(7)
    for b, c, _, _ in ranges:
        x = rnd(c, seed=200 + c)
        k = torch.randint(-20, 21, (c,), generator=gen)
        g[b:b + c] = torch.ldexp(x, k)
    sq = g.double().numpy() ** 2                                     # exact: 24-bit significands
    return g, ranges, [math.fsum(sq[b:b + c]) for b, c, _, _ in ranges]


def test_grad_sumsq_against_fp64(ss_case):
    g, ranges, want = ss_case
    bands = Bands(DEV)
    gd = bands.place(g, "g")
    out = bands.guarded(6, torch.float64, name="sumsq")
    for i, r in enumerate(ranges):
        ops.grad_sumsq(gd, [r], out=out[i:i + 1])
    ops.grad_sumsq(gd, ranges, out=out[5:6])
    bands.assert_bands_intact()
    got = out.cpu().tolist()
    for (b, c, _, _), x, w in zip(ranges, got[:5], want):
        rel = abs(x - w) / w
        print(f"[sumsq] n = {c}: {x!r} vs {w!r}, rel = {rel:.3e}, bound = {c * 2.0 ** -53:.3e}")
        assert rel <= c * 2.0 ** -53, (c, x, w)
    n, w = sum(SS_SIZES), math.fsum(want)
    print(f"[sumsq] all five ranges: rel = {abs(got[5] - w) / w:.3e}, bound = {n * 2.0 ** -53:.3e}")
    assert abs(got[5] - w) / w <= n * 2.0 ** -53


def test_grad_sumsq_repeats_its_bits_eager_and_replayed(ss_case):
    g, ranges, _ = ss_case
    gd = g.to(DEV)
    a, b, c = (torch.zeros(1, dtype=torch.float64, device=DEV) for _ in range(3))
    ops.grad_sumsq(gd, ranges, out=a)
    ops.grad_sumsq(gd, ranges, out=b)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        ops.grad_sumsq(gd, ranges, out=c)
    graph.replay()
    graph.replay()
    torch.cuda.synchronize()
    assert math.isfinite(a.item()) and a.item() > 0
    assert bits_equal(a, b) and bits_equal(a, c)


# ---- 3. three steps against torch on the CPU ---------------------------------------------------------------------------------------------
# (begin, count, decay): a tail, a one-block range without decay, a 20-block range, a 4-element range without decay
T_RANGES = [(0, 1031, True), (1032, 903, False), (2048, 20003, True), (22052, 4, False)]
T_N = 22056
SCALES = (1.0, 3.0, 0.2)             # one max_norm = step 1's norm: the coefficient is ~1, 1/3 and 1 — Adam is invariant under a CONSTANT one
COSINE = dict(schedule="cosine", warmup_steps=2, total_steps=5, min_lr=1e-5)


@pytest.fixture(scope="module")
def t_case():
    p0 = rnd(T_N, seed=300)
    grads = [rnd(T_N, seed=301 + t) * s for t, s in enumerate(SCALES)]
    norm1 = math.sqrt(math.fsum(np.concatenate([grads[0][b:b + c].double().numpy() ** 2 for b, c, _ in T_RANGES])))
    return p0, grads, norm1


def _torch_three_steps(p0, grads, opt, max_norm):
    prm = [torch.nn.Parameter(p0[b:b + c].clone()) for b, c, _ in T_RANGES]
    groups = [{"params": [q for q, r in zip(prm, T_RANGES) if r[2]], "weight_decay": opt.weight_decay},
              {"params": [q for q, r in zip(prm, T_RANGES) if not r[2]], "weight_decay": 0.0}]
    ref = (torch.optim.AdamW if opt.decoupled else torch.optim.Adam)(groups, lr=HYPER[0], betas=HYPER[1:3], eps=HYPER[3], foreach=False)
    out = []
    for t, g in enumerate(grads):
        for grp in ref.param_groups:
            grp["lr"] = opt.lr_at(HYPER[0], t)                       # step t + 1 runs at the rate after t ticks
        for q, (b, c, _) in zip(prm, T_RANGES):
            q.grad = g[b:b + c].clone()
        if max_norm is not None:
            torch.nn.utils.clip_grad_norm_(prm, max_norm)
        ref.step()
        full = p0.clone()
        for q, (b, c, _) in zip(prm, T_RANGES):
            full[b:b + c] = q.detach()
        out.append(full)
    return out


@pytest.mark.parametrize("decoupled,clip,scaled,sched", [
    (False, False, False, {}), (False, True, False, {}), (True, False, False, {}), (True, True, False, {}),
    (False, True, True, {}), (True, True, True, {}), (True, True, False, COSINE)],
    ids=["adam-wd", "adam-wd-clip", "adamw", "adamw-clip", "adam-wd-clip-lossscale", "adamw-clip-lossscale", "adamw-clip-cosine"])
def test_three_steps_match_torch(t_case, decoupled, clip, scaled, sched):
    p0, grads, norm1 = t_case
    opt = OptimOptions(weight_decay=0.01, decoupled=decoupled, max_grad_norm=norm1 if clip else None, **sched)
    want = _torch_three_steps(p0, grads, opt, opt.max_grad_norm)
    bands, t = _place({"p": p0, "m": torch.zeros(T_N), "v": torch.zeros(T_N)})
    g = bands.guarded(T_N, torch.float32, name="g")
    step = torch.zeros(1, dtype=I64, device=DEV)
    ranges = [(b, c, 0, d) for b, c, d in T_RANGES]
    gs = 1.0 / 1024 if scaled else 1.0                              # the fp16 route: the arena holds loss_scale x gradient
    worst, coefs = 0.0, []
    for ti, gr in enumerate(grads, start=1):
        g.copy_(gr * 1024 if scaled else gr)
        ss = ops.grad_sumsq(g, ranges) if clip else None
        ops.optim_step_dev_ranges(t["p"], g, t["m"], t["v"], ranges, *HYPER, opt, step, gs, sumsq=ss)
        ops.counter_add(step, 1)
        bands.assert_bands_intact()
        if clip:
            coefs.append(min(1.0, norm1 / (gs * math.sqrt(ss.item()) + 1e-6)))
        ref = want[ti - 1]
        bound = 2e-7 + ti * 2.0 ** -23 * ref.abs()
        ratio = ((t["p"].cpu() - ref).abs() / bound).max().item()
        worst = max(worst, ratio)
        print(f"[optim] step {ti}: worst |p - p_ref| / bound = {ratio:.3f}")
        assert ratio <= 1.0, f"step {ti}: {ratio:.3f} x the bound"
    print(f"[optim] decoupled={decoupled} clip={clip} scaled={scaled} sched={bool(sched)}: worst ratio {worst:.3f}, coefficients {coefs}")
    untouched = torch.ones(T_N, dtype=torch.bool)
    for b, c, _ in T_RANGES:
        untouched[b:b + c] = False
    assert torch.equal(t["p"].cpu()[untouched], p0[untouched]) and not t["m"].cpu()[untouched].any()
    if clip:
        assert coefs[0] > 0.99 and abs(coefs[1] - 1 / 3) < 1e-3 and coefs[2] == 1.0, coefs
    # the options are not decoration: against the same three steps without them the parameters differ by far more than the bound
    plain = _torch_three_steps(p0, grads, OptimOptions(**sched), None)[-1]
    assert ((want[-1] - plain).abs() / (2e-7 + 3 * 2.0 ** -23 * plain.abs())).max() > 10
    if clip:
        unclipped = _torch_three_steps(p0, grads, OptimOptions(weight_decay=0.01, decoupled=decoupled, **sched), None)[-1]
        assert ((want[-1] - unclipped).abs() / (2e-7 + 3 * 2.0 ** -23 * unclipped.abs())).max() > 10, "a missing clip would pass"


# ---- 4. the schedule on the device --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kw,total", [
    (dict(schedule="cosine", total_steps=12, min_lr=1e-5), 12), (dict(schedule="cosine", warmup_steps=3, total_steps=12, min_lr=0.0), 12),
    (dict(schedule="step", step_period=3, gamma=0.5), 12), (dict(schedule="step", warmup_steps=2, step_period=4, gamma=0.1), 12),
    (dict(warmup_steps=4), 6), (dict(), 2)], ids=["cosine", "warmup-cosine", "step", "warmup-step", "warmup-constant", "constant"])
def test_device_schedule_against_the_closed_form(kw, total):
    opt, lr = OptimOptions(**kw), 3e-3
    steps = torch.arange(total + 4, dtype=I64, device=DEV)
    bands = Bands(DEV)
    out = bands.guarded(total + 4, torch.float64, name="lr")
    for e in range(total + 4):
        ops.optim_lr(lr, opt, steps[e], out=out[e:e + 1])
    bands.assert_bands_intact()
    got = out.cpu().tolist()
    for e, x in enumerate(got):
        w = opt.lr_at(lr, e)
        assert abs(x - w) <= 8 * 2.0 ** -52 * lr, (e, x, w)
    assert len(set(got)) > 1 or not kw


# ---- 5. the guard under clipping ------------------------------------------------------------------------------------------------------------
def test_stamped_step_with_clipping_touches_nothing():
    data = _arenas(T_N, 400)
    data["g"][5] = float("inf")                                      # what a stamped step looks like: the norm is not a number either
    bands, t = _place(data)
    shadow = bands.guarded(1024, torch.bfloat16, fill=0.0, name="shadow")
    step = torch.tensor([9], dtype=I64, device=DEV)
    bad = torch.tensor([10], dtype=I64, device=DEV)
    ranges = [(b, c, 0, d) for b, c, d in T_RANGES]
    opt = OptimOptions(weight_decay=0.01, decoupled=True, max_grad_norm=1.0, warmup_steps=3)
    ss = ops.grad_sumsq(t["g"], ranges)
    ops.optim_step_dev_ranges(t["p"], t["g"], t["m"], t["v"], ranges, *HYPER, opt, step, 1.0, sumsq=ss, shadow=shadow, shadow_begin=2048, bad_step=bad)
    bands.assert_bands_intact()
    assert not math.isfinite(ss.item())
    assert all(bits_equal(t[k].cpu(), data[k]) for k in "pgmv") and not shadow.any()
    bad.fill_(9)                                                     # another step's stamp: the update runs
    data["g"][5] = 0.5
    t["g"].copy_(data["g"])
    ss = ops.grad_sumsq(t["g"], ranges)
    ops.optim_step_dev_ranges(t["p"], t["g"], t["m"], t["v"], ranges, *HYPER, opt, step, 1.0, sumsq=ss, shadow=shadow, shadow_begin=2048, bad_step=bad)
    bands.assert_bands_intact()
    assert not bits_equal(t["p"].cpu(), data["p"]) and bits_equal(shadow, t["p"][2048:2048 + 1024].to(torch.bfloat16))
