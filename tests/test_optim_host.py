"""CPU: optimizer options on the fused step (include/goalnet_optim.h) — what holds without a GPU: the fourth header
against its ctypes table and the built library, the untouched first ABI, the argument refusals of the new entry points (every one
returns before any launch; pointers are small fake integers, as in tests/test_abi.py), OptimOptions, the path decision and the
closed-form schedule against torch's schedulers."""
import ctypes
import os
import re

import pytest
import torch

from cvml_goalnet_amd import GoalnetError, _lib
from cvml_goalnet_amd.avm import _Spec, optim_ranges, optim_step_path, trainable_ranges
from cvml_goalnet_amd.optim import OptimOptions

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
E_NULL, E_SHAPE, E_ALIGN, E_WORKSPACE, E_VALUE = -1, -2, -3, -4, -5
A, A2, A3, A4, A5, A6, A7 = 4096, 8192, 12288, 16384, 20480, 24576, 28672     # fake, 16-byte aligned "device addresses": never dereferenced


def _header(name="goalnet_optim.h"):
    return open(os.path.join(ROOT, "include", name)).read()


def _declared():
    text = re.sub(r"/\*.*?\*/", "", _header(), flags=re.S)
    return sorted(set(re.findall(r"\b(goalnet_[a-z0-9_]+)\s*\(", text)))


def test_optim_header_and_binding_agree():
    assert _declared() == sorted(_lib.OPTIM_PROTOTYPES)
    if not os.path.exists(_lib.LIB_PATH):
        import __graft_entry__ as g
        g.build()
    lib = ctypes.CDLL(_lib.LIB_PATH)
    for name in _declared():
        assert hasattr(lib, name), f"{name} missing from libgoalnet_hip.so"
    loaded = _lib.load()
    for name, (res, args) in _lib.OPTIM_PROTOTYPES.items():
        fn = getattr(loaded, name)
        assert fn.restype is res and list(fn.argtypes) == args, f"{name} was not bound by _lib.load()"


def test_the_other_three_headers_are_untouched_by_these_names():
    assert _lib.ABI_VERSION == 7 and _lib.load().goalnet_abi_version() == 7
    assert "#define GOALNET_ABI_VERSION 7" in _header("goalnet_hip.h")
    for table in (_lib.PROTOTYPES, _lib.LOSS_PROTOTYPES, _lib.EPOCH_PROTOTYPES):
        assert set(_lib.OPTIM_PROTOTYPES).isdisjoint(table)
    for other in ("goalnet_hip.h", "goalnet_loss.h", "goalnet_epoch.h"):
        text = _header(other)
        for name in (*_lib.OPTIM_PROTOTYPES, "goalnet_optim_range", "goalnet_optim_opts"):
            assert name not in text, f"{name} belongs to include/goalnet_optim.h, not {other}"


def test_structs_and_codes_match_the_header():
    h = _header()
    codes = {m.group(1).lower(): int(m.group(2)) for m in re.finditer(r"#define GOALNET_SCHED_([A-Z]+) (\d+)", h)}
    assert codes == _lib.SCHEDULES
    assert ctypes.sizeof(_lib.OptimRange) == 32 and ctypes.sizeof(_lib.OptimOpts) == 8 * 8 + 3 * 8 + 2 * 4
    rng = re.search(r"typedef struct \{([^}]*)\} goalnet_optim_range;", h).group(1)
    assert re.findall(r"\b([a-z_0-9]+)\s*[,;]", rng) == [f for f, _ in _lib.OptimRange._fields_]
    opts = re.sub(r"/\*.*?\*/", "", re.search(r"typedef struct \{([^}]*)\} goalnet_optim_opts;", h, flags=re.S).group(1), flags=re.S)
    assert re.findall(r"\b([a-z_0-9]+)\s*[,;]", opts) == [f for f, _ in _lib.OptimOpts._fields_]


# ---- argument refusals: every one before any launch ------------------------------------------------------------------------------------
def _ranges(rs):
    return (_lib.OptimRange * len(rs))(*[_lib.OptimRange(*r) for r in rs])


def _opts(lr=1e-3, wd=0.0, max_norm=0.0, min_lr=0.0, gamma=0.1, warmup=0, total=0, period=0, decoupled=0, schedule=0):
    return _lib.OptimOpts(lr, 0.9, 0.999, 1e-8, wd, max_norm, min_lr, gamma, warmup, total, period, decoupled, schedule)


GOOD = [(0, 100, 0, 1, 0), (128, 7, 2, 0, 0)]


# goalnet_optim_step_dev_ranges(p, g, m, v, ranges, count, opts, step, grad_scale, sumsq, shadow, sh_begin, sh_count, f16, bad_step, stream)
def _step(p=A, g=A2, m=A3, v=A4, ranges=GOOD, count=None, opts=None, no_opts=False, step=A5, sumsq=None, shadow=None, sh_begin=0, sh_count=0):
    o = None if no_opts else ctypes.byref(opts if opts is not None else _opts())
    arr = None if ranges is None else _ranges(ranges)
    return [p, g, m, v, arr, (len(ranges) if ranges else 1) if count is None else count, o, step, 1.0, sumsq, shadow, sh_begin, sh_count, 0, None,
            None]


MANY = [(64 * r, 8, 0, 0, 0) for r in range(33)]
STEP_REFUSALS = [
    ("null step counter", _step(step=None), E_NULL),
    ("null arena", _step(m=None), E_NULL),
    ("null ranges", _step(ranges=None), E_NULL),
    ("null options", _step(no_opts=True), E_NULL),
    ("weight_decay < 0", _step(opts=_opts(wd=-0.01)), E_VALUE),
    ("weight_decay = NaN", _step(opts=_opts(wd=float("nan"))), E_VALUE),
    ("unsorted ranges", _step(ranges=[GOOD[1], GOOD[0]]), E_SHAPE),
    ("overlapping ranges", _step(ranges=[(0, 100, 0, 1, 0), (96, 8, 0, 0, 0)]), E_SHAPE),
    ("empty range", _step(ranges=[(0, 0, 0, 0, 0)]), E_SHAPE),
    ("negative skipped", _step(ranges=[(0, 8, -1, 0, 0)]), E_SHAPE),
    ("range begins off a multiple of 4", _step(ranges=[(2, 8, 0, 0, 0)]), E_ALIGN),
    ("count = 0", _step(count=0), E_SHAPE),
    ("count = 33", _step(ranges=MANY), E_SHAPE),
    ("misaligned arena", _step(g=A2 + 4), E_ALIGN),
    ("max_norm > 0 without sumsq", _step(opts=_opts(max_norm=1.0)), E_NULL),
    ("sumsq without max_norm > 0", _step(sumsq=A6), E_VALUE),
    ("misaligned sumsq", _step(opts=_opts(max_norm=1.0), sumsq=A6 + 4), E_ALIGN),
    ("cosine with total = warmup", _step(opts=_opts(schedule=1, warmup=5, total=5)), E_VALUE),
    ("cosine with total < warmup", _step(opts=_opts(schedule=1, warmup=5, total=3)), E_VALUE),
    ("step with period = 0", _step(opts=_opts(schedule=2, period=0)), E_VALUE),
    ("step with gamma = 0", _step(opts=_opts(schedule=2, period=3, gamma=0.0)), E_VALUE),
    ("unknown schedule", _step(opts=_opts(schedule=3)), E_VALUE),
    ("negative warmup", _step(opts=_opts(warmup=-1)), E_VALUE),
    ("negative min_lr", _step(opts=_opts(min_lr=-1e-5)), E_VALUE),
    ("shadow off a multiple of 4", _step(shadow=A7, sh_begin=2, sh_count=8), E_SHAPE),
    ("misaligned shadow", _step(shadow=A7 + 4, sh_begin=0, sh_count=8), E_ALIGN),
]


def _refused(name, args, code, what):
    lib = _lib.load()
    rc = getattr(lib, name)(*args)
    msg = lib.goalnet_last_error()
    assert rc == code, f"{name}, {what}: rc = {rc}, expected {code} ({msg!r})"
    assert rc < 0 and msg, f"{name}, {what}: no error message"


@pytest.mark.parametrize("what,args,code", STEP_REFUSALS, ids=[r[0] for r in STEP_REFUSALS])
def test_optim_step_refusals(what, args, code):
    _refused("goalnet_optim_step_dev_ranges", args, code, what)


# goalnet_grad_sumsq(g, ranges, count, sumsq, ws, ws_bytes, stream)
def _ss(g=A, ranges=GOOD, count=None, sumsq=A2, ws=A3, ws_bytes=1 << 20):
    return [g, None if ranges is None else _ranges(ranges), (len(ranges) if ranges else 1) if count is None else count, sumsq, ws, ws_bytes, None]


SUMSQ_REFUSALS = [
    ("null gradient", _ss(g=None), E_NULL),
    ("null result", _ss(sumsq=None), E_NULL),
    ("null workspace", _ss(ws=None), E_NULL),
    ("null ranges", _ss(ranges=None), E_NULL),
    ("count = 33", _ss(ranges=MANY), E_SHAPE),
    ("unsorted ranges", _ss(ranges=[GOOD[1], GOOD[0]]), E_SHAPE),
    ("range begins off a multiple of 4", _ss(ranges=[(6, 8, 0, 0, 0)]), E_ALIGN),
    ("misaligned arena", _ss(g=A + 8), E_ALIGN),
    ("misaligned workspace", _ss(ws=A3 + 4), E_ALIGN),
    ("workspace one byte short", _ss(ws_bytes=15), E_WORKSPACE),
]


@pytest.mark.parametrize("what,args,code", SUMSQ_REFUSALS, ids=[r[0] for r in SUMSQ_REFUSALS])
def test_grad_sumsq_refusals(what, args, code):
    _refused("goalnet_grad_sumsq", args, code, what)


def test_grad_sumsq_workspace_size():
    lib = _lib.load()
    assert lib.goalnet_grad_sumsq_ws_bytes(_ranges(GOOD), 2) == 16                          # one block per small range
    big = [(0, 4 * 256 * 5 + 3, 0, 0, 0), (8192, 1 << 24, 0, 0, 0)]
    assert lib.goalnet_grad_sumsq_ws_bytes(_ranges(big), 2) == 8 * (5 + 1024)               # 256 float4 per block, at most 1024 blocks a range
    assert lib.goalnet_grad_sumsq_ws_bytes(_ranges(MANY), 33) == 0
    assert lib.goalnet_grad_sumsq_ws_bytes(_ranges([GOOD[1], GOOD[0]]), 2) == 0
    assert lib.goalnet_grad_sumsq_ws_bytes(None, 1) == 0


def test_optim_lr_refusals():
    _refused("goalnet_optim_lr", [ctypes.byref(_opts()), None, A2, None], E_NULL, "null step counter")
    _refused("goalnet_optim_lr", [ctypes.byref(_opts()), A, None, None], E_NULL, "null result")
    _refused("goalnet_optim_lr", [None, A, A2, None], E_NULL, "null options")
    _refused("goalnet_optim_lr", [ctypes.byref(_opts(schedule=1, warmup=2, total=2)), A, A2, None], E_VALUE, "cosine with total = warmup")


# ---- OptimOptions ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kw", [
    dict(weight_decay=-0.1), dict(weight_decay=float("inf")), dict(weight_decay="0.1"), dict(max_grad_norm=0.0), dict(max_grad_norm=-1.0),
    dict(max_grad_norm=float("nan")), dict(schedule="linear"), dict(warmup_steps=-1), dict(warmup_steps=1.5), dict(min_lr=-1e-4),
    dict(schedule="cosine"), dict(schedule="cosine", total_steps=5, warmup_steps=5), dict(schedule="cosine", total_steps=4, warmup_steps=5),
    dict(schedule="step"), dict(schedule="step", step_period=0), dict(schedule="step", step_period=3, gamma=0.0), dict(no_decay="bias"),
    dict(no_decay=("bias", "")), dict(total_steps=-1), dict(step_period=0),
], ids=lambda kw: ",".join(f"{k}={v}" for k, v in kw.items()))
def test_options_validate_in_the_constructor(kw):
    with pytest.raises(ValueError):
        OptimOptions(**kw)


def test_options_trivial_signature_and_decays():
    assert OptimOptions().trivial and OptimOptions().signature() == ()
    assert OptimOptions(decoupled=True, no_decay=("bias",), gamma=0.5, min_lr=1e-5).trivial, "nothing is switched on by these alone"
    on = [OptimOptions(weight_decay=0.01), OptimOptions(max_grad_norm=1.0), OptimOptions(schedule="cosine", total_steps=5),
          OptimOptions(schedule="step", step_period=2), OptimOptions(warmup_steps=1)]
    assert not any(o.trivial for o in on)
    sigs = {o.signature() for o in on} | {OptimOptions(weight_decay=0.01, decoupled=True).signature(),
                                           OptimOptions(weight_decay=0.01, no_decay=("bias",)).signature()}
    assert len(sigs) == 7 and () not in sigs, "options that bake different launch arguments have different signatures"
    assert OptimOptions(weight_decay=0.01, no_decay=["bias"]).signature() == OptimOptions(weight_decay=0.01, no_decay=("bias",)).signature()
    hash(on[0].signature())
    with pytest.raises(Exception):
        on[0].weight_decay = 0.1                                                             # frozen
    o = OptimOptions(weight_decay=0.01, no_decay=("bias", "bnorm"))
    assert o.decays("visbl.conv2.weight") and not o.decays("visbl.conv2.bias") and not o.decays("visbl.bnorm1.weight")
    assert not OptimOptions(no_decay=()).decays("visbl.conv2.weight"), "no decay without weight_decay"


# ---- the path decision and the ranges ---------------------------------------------------------------------------------------------------
def _specs():
    out, off = [], 0
    for name, n in (("a.weight", 100), ("a.bias", 10), ("bnorm.weight", 10), ("bnorm.bias", 10), ("b.weight", 64), ("c.weight", 130), ("c.bias", 3)):
        s = _Spec(name, "plain", (n,), n)
        s.offset = off
        off += (n + 63) // 64 * 64
        out.append(s)
    return out


def test_path_decision():
    assert optim_step_path(None, sharded=False) is False and optim_step_path(None, sharded=True) is False
    assert optim_step_path(OptimOptions(), sharded=False) is False, "trivial options: today's plan"
    assert optim_step_path(OptimOptions(), sharded=True) is False, "and today's plan shards as it did"
    assert optim_step_path(OptimOptions(max_grad_norm=1.0), sharded=False) is True
    for o in (OptimOptions(weight_decay=0.01), OptimOptions(max_grad_norm=1.0), OptimOptions(warmup_steps=3)):
        with pytest.raises(GoalnetError, match="shard_linear5"):
            optim_step_path(o, sharded=True)


def test_ranges_split_where_the_decay_flag_changes():
    specs = _specs()
    plain = [(b, c, k, False) for b, c, k in trainable_ranges(specs, frozenset(), {})]
    assert optim_ranges(specs, frozenset(), {}, OptimOptions(max_grad_norm=1.0)) == plain == [(0, 579, 0, False)]
    assert optim_ranges(specs, frozenset(), {}, OptimOptions(weight_decay=0.01)) == [(0, 579, 0, True)]
    o = OptimOptions(weight_decay=0.01, no_decay=("bias", "bnorm"))
    assert optim_ranges(specs, frozenset(), {}, o) == [(0, 100, 0, True), (128, 138, 0, False), (320, 194, 0, True), (576, 3, 0, False)]
    # frozen tensors and sat-out counts split as trainable_ranges splits them
    got = optim_ranges(specs, frozenset({"b.weight"}), {"c.weight": 2, "c.bias": 2}, o)
    assert got == [(0, 100, 0, True), (128, 138, 0, False), (384, 130, 2, True), (576, 3, 2, False)]
    assert [(b, c, k) for b, c, k, _ in optim_ranges(specs, frozenset({"b.weight"}), {"c.weight": 2, "c.bias": 2}, OptimOptions(warmup_steps=1))] \
        == trainable_ranges(specs, frozenset({"b.weight"}), {"c.weight": 2, "c.bias": 2})
    assert all(b % 4 == 0 for b, _, _, _ in got)


# ---- the schedule's closed form ---------------------------------------------------------------------------------------------------------
def _torch_rates(make, base, steps):
    p = torch.nn.Parameter(torch.zeros(1))
    opt = torch.optim.SGD([p], lr=base)
    sched = make(opt)
    out = []
    for _ in range(steps):
        out.append(opt.param_groups[0]["lr"])           # the rate step e + 1 runs at, after e ticks
        opt.step()
        sched.step()
    return out


def test_lr_at_matches_cosine_annealing():
    base, T, eta = 3e-3, 17, 1e-5
    o = OptimOptions(schedule="cosine", total_steps=T, min_lr=eta)
    want = _torch_rates(lambda opt: torch.optim.lr_scheduler.CosineAnnealingLR(opt, T_max=T, eta_min=eta), base, T + 1)
    for e, w in enumerate(want):
        assert abs(o.lr_at(base, e) - w) <= 1e-12 * w, (e, o.lr_at(base, e), w)
    assert o.lr_at(base, T + 5) == o.lr_at(base, T) and abs(o.lr_at(base, T) - eta) <= 1e-12 * eta, "held at min_lr past total_steps"


def test_lr_at_matches_step_lr():
    base = 2e-3
    o = OptimOptions(schedule="step", step_period=4, gamma=0.3)
    want = _torch_rates(lambda opt: torch.optim.lr_scheduler.StepLR(opt, step_size=4, gamma=0.3), base, 14)
    for e, w in enumerate(want):
        assert abs(o.lr_at(base, e) - w) <= 1e-12 * w, (e, o.lr_at(base, e), w)


def test_lr_at_warmup_by_hand():
    base = 1e-3
    o = OptimOptions(schedule="cosine", warmup_steps=4, total_steps=8, min_lr=1e-4)
    assert [o.lr_at(base, e) for e in range(4)] == [base * 1.0 / 4.0, base * 2.0 / 4.0, base * 3.0 / 4.0, base * 4.0 / 4.0]
    assert o.lr_at(base, 4) == base, "the first step after warm-up runs at the full rate: cos(0) = 1"
    assert abs(o.lr_at(base, 6) - (1e-4 + (base - 1e-4) * 0.5)) <= 1e-18, "half way down the cosine: cos(pi / 2)"
    assert abs(o.lr_at(base, 8) - 1e-4) <= 1e-18 and o.lr_at(base, 11) == o.lr_at(base, 8)
    c = OptimOptions(warmup_steps=2)
    assert [c.lr_at(base, e) for e in range(4)] == [base / 2.0, base, base, base]
    s = OptimOptions(schedule="step", warmup_steps=2, step_period=3, gamma=0.5)
    assert [s.lr_at(base, e) for e in range(9)] == [base / 2.0, base, base, base, base, base * 0.5, base * 0.5, base * 0.5, base * 0.25]
    assert OptimOptions().lr_at(base, 123) == base


def test_python_surface_refuses_before_any_launch():
    from cvml_goalnet_amd import optim as O
    prm = [torch.nn.Parameter(torch.zeros(1))]
    with pytest.raises(ValueError):
        O.Adam(prm, weight_decay=-1.0)
    with pytest.raises(ValueError):
        O.Adam(prm, weight_decay=0.1, options=OptimOptions(weight_decay=0.1))
    with pytest.raises(ValueError):
        O.Adam(prm, options=OptimOptions(weight_decay=0.1, decoupled=True))
    with pytest.raises(ValueError):
        O.Adam(prm, options="cosine")
    assert O.AdamW(prm).options == OptimOptions(weight_decay=0.01, decoupled=True), "torch.optim.AdamW's default decay"
    assert O.Adam(prm).options.trivial and O.Adam(prm, weight_decay=0.02).options.decoupled is False
    from cvml_goalnet_amd.loop import VideoTrainer
    with pytest.raises(ValueError):
        VideoTrainer(object(), optim={"weight_decay": 0.1})
