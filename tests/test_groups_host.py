"""CPU: parameter groups and AMSGrad on the fused step (include/goalnet_groups.h) — what holds without a GPU: the
seventh header against its ctypes table and the built library, the untouched six older headers, the argument refusals of the entry
points (every one returns before any launch; pointers are small fake integers, as in tests/test_optim_host.py), ParamGroup and
OptimOptions, the signature that saved trainer states compare, the cut of the real spec list into group ranges, and the drop-in
optimizer's construction-time and step-time refusals."""
import ctypes
import os
import re

import pytest
import torch

from cvml_goalnet_amd import AVM, GoalnetError, OptimOptions, ParamGroup, _lib
from cvml_goalnet_amd import optim as O
from cvml_goalnet_amd.avm import _Spec, group_ranges, optim_ranges

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
E_NULL, E_SHAPE, E_ALIGN, E_VALUE = -1, -2, -3, -5
A, A2, A3, A4, A5, A6, A7, A8 = 4096, 8192, 12288, 16384, 20480, 24576, 28672, 32768     # fake "device addresses": never dereferenced
OLDER_HEADERS = ("goalnet_hip.h", "goalnet_loss.h", "goalnet_epoch.h", "goalnet_optim.h", "goalnet_ema.h", "goalnet_accum.h")
HW3, L2 = 81, 8                                   # 40 x 40 frames, 30 bins
NAN, INF = float("nan"), float("inf")


def _header(name="goalnet_groups.h"):
    return open(os.path.join(ROOT, "include", name)).read()


def _declared():
    text = re.sub(r"/\*.*?\*/", "", _header(), flags=re.S)
    return sorted(set(re.findall(r"\b(goalnet_[a-z0-9_]+)\s*\(", text)))


def test_groups_header_and_binding_agree():
    assert _declared() == sorted(_lib.GROUPS_PROTOTYPES) == ["goalnet_group_lr", "goalnet_group_step_dev_ranges"]
    if not os.path.exists(_lib.LIB_PATH):
        import __graft_entry__ as g
        g.build()
    lib = ctypes.CDLL(_lib.LIB_PATH)
    for name in _declared():
        assert hasattr(lib, name), f"{name} missing from libgoalnet_hip.so"
    loaded = _lib.load()
    for name, (res, args) in _lib.GROUPS_PROTOTYPES.items():
        fn = getattr(loaded, name)
        assert fn.restype is res and list(fn.argtypes) == args, f"{name} was not bound by _lib.load()"


def test_structs_match_the_header():
    h = _header()
    assert int(re.search(r"#define GOALNET_GROUPS_MAX (\d+)", h).group(1)) == _lib.GROUPS_MAX == 8 == O.GROUPS_MAX + 1
    assert ctypes.sizeof(_lib.GroupHyper) == 5 * 8 + 2 * 4 and ctypes.sizeof(_lib.GroupRange) == 32
    hyper = re.search(r"typedef struct \{([^}]*)\} goalnet_group_hyper;", h).group(1)
    assert re.findall(r"\b([a-z_0-9]+)\s*[,;]", hyper) == [f for f, _ in _lib.GroupHyper._fields_]
    rng = re.search(r"typedef struct \{([^}]*)\} goalnet_group_range;", h).group(1)
    assert re.findall(r"\b([a-z_0-9]+)\s*[,;]", rng) == [f for f, _ in _lib.GroupRange._fields_]


def test_the_six_older_headers_are_untouched_by_these_names():
    assert _lib.ABI_VERSION == 7 and _lib.load().goalnet_abi_version() == 7
    assert "#define GOALNET_ABI_VERSION 7" in _header("goalnet_hip.h")
    for table in (_lib.PROTOTYPES, _lib.LOSS_PROTOTYPES, _lib.EPOCH_PROTOTYPES, _lib.OPTIM_PROTOTYPES, _lib.EMA_PROTOTYPES, _lib.ACCUM_PROTOTYPES):
        assert set(_lib.GROUPS_PROTOTYPES).isdisjoint(table)
    for other in OLDER_HEADERS:
        text = _header(other)
        for name in (*_lib.GROUPS_PROTOTYPES, "goalnet_group_hyper", "goalnet_group_range", "GOALNET_GROUPS_MAX"):
            assert name not in text, f"{name} belongs to include/goalnet_groups.h, not {other}"


def test_the_build_depends_on_the_header():
    assert '"goalnet_groups.h"' in open(os.path.join(ROOT, "__graft_entry__.py")).read()


# ---- argument refusals: every one before any launch ------------------------------------------------------------------------------------
def _ranges(rs):
    return (_lib.GroupRange * len(rs))(*[_lib.GroupRange(*r) for r in rs])


def _hyper(lr=1e-3, b1=0.9, b2=0.999, eps=1e-8, wd=0.0, ams=0):
    return (lr, b1, b2, eps, wd, ams, 0)


def _table(rows):
    return (_lib.GroupHyper * len(rows))(*[_lib.GroupHyper(*r) for r in rows])


def _opts(wd=0.0, max_norm=0.0, min_lr=0.0, gamma=0.1, warmup=0, total=0, period=0, decoupled=0, schedule=0):
    return _lib.OptimOpts(1e-3, 0.9, 0.999, 1e-8, wd, max_norm, min_lr, gamma, warmup, total, period, decoupled, schedule)


GOOD = [(0, 100, 0, 1, 0), (128, 7, 2, 0, 1)]             # (begin, count, skipped, decay, group)
TWO = [_hyper(), _hyper(lr=1e-2, b1=0.8, b2=0.5)]
MANY = [(64 * r, 8, 0, 0, 0) for r in range(33)]


# goalnet_group_step_dev_ranges(p, g, m, v, vmax, ranges, count, groups, ngroups, opts, step, grad_scale, sumsq, shadow, sh_begin, sh_count,
#                               f16, bad_step, stream)
def _step(p=A, g=A2, m=A3, v=A4, vmax=None, ranges=GOOD, count=None, groups=TWO, ngroups=None, opts=None, no_opts=False, step=A5, sumsq=None,
          shadow=None, sh_begin=0, sh_count=0):
    o = None if no_opts else ctypes.byref(opts if opts is not None else _opts())
    arr = None if ranges is None else _ranges(ranges)
    tab = None if groups is None else _table(groups)
    return [p, g, m, v, vmax, arr, (len(ranges) if ranges else 1) if count is None else count, tab,
            (len(groups) if groups else 1) if ngroups is None else ngroups, o, step, 1.0, sumsq, shadow, sh_begin, sh_count, 0, None, None]


STEP_REFUSALS = [
    # what the issue lists for the groups
    ("ngroups = 0", _step(ngroups=0), E_SHAPE),
    ("ngroups = 9", _step(groups=[_hyper()] * 9), E_SHAPE),
    ("a range's group beyond the table", _step(ranges=[(0, 100, 0, 1, 2)]), E_SHAPE),
    ("a range's group below 0", _step(ranges=[(0, 100, 0, 1, -1)]), E_SHAPE),
    ("lr < 0", _step(groups=[_hyper(), _hyper(lr=-1e-3)]), E_VALUE),
    ("lr = NaN", _step(groups=[_hyper(lr=NAN)], ranges=GOOD[:1]), E_VALUE),
    ("lr = inf", _step(groups=[_hyper(), _hyper(lr=INF)]), E_VALUE),
    ("beta1 = 1", _step(groups=[_hyper(b1=1.0), _hyper()]), E_VALUE),
    ("beta1 < 0", _step(groups=[_hyper(b1=-0.1), _hyper()]), E_VALUE),
    ("beta2 = 1", _step(groups=[_hyper(), _hyper(b2=1.0)]), E_VALUE),
    ("beta2 = NaN", _step(groups=[_hyper(), _hyper(b2=NAN)]), E_VALUE),
    ("eps < 0", _step(groups=[_hyper(), _hyper(eps=-1e-8)]), E_VALUE),
    ("eps = inf", _step(groups=[_hyper(), _hyper(eps=INF)]), E_VALUE),
    ("weight_decay < 0", _step(groups=[_hyper(wd=-0.01), _hyper()]), E_VALUE),
    ("weight_decay = NaN", _step(groups=[_hyper(wd=NAN), _hyper()]), E_VALUE),
    ("an unreferenced group is checked too", _step(groups=TWO + [_hyper(lr=-1.0)]), E_VALUE),
    ("amsgrad without vmax", _step(groups=[_hyper(), _hyper(ams=1)]), E_VALUE),
    ("null group table", _step(groups=None), E_NULL),
    ("misaligned vmax", _step(groups=[_hyper(), _hyper(ams=1)], vmax=A8 + 4), E_ALIGN),
    # everything goalnet_optim_step_dev_ranges refuses
    ("null step counter", _step(step=None), E_NULL),
    ("null arena", _step(m=None), E_NULL),
    ("null ranges", _step(ranges=None), E_NULL),
    ("null options", _step(no_opts=True), E_NULL),
    ("options' weight_decay < 0", _step(opts=_opts(wd=-0.01)), E_VALUE),
    ("options' weight_decay = NaN", _step(opts=_opts(wd=NAN)), E_VALUE),
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
    assert rc == code, f"{what}: rc = {rc}, expected {code} ({msg!r})"
    assert rc < 0 and msg, f"{what}: no error message"


@pytest.mark.parametrize("what,args,code", STEP_REFUSALS, ids=[r[0] for r in STEP_REFUSALS])
def test_group_step_refusals(what, args, code):
    _refused("goalnet_group_step_dev_ranges", args, code, what)


# goalnet_group_lr(opts, groups, g, step, lr_out, stream)
def _lr(opts=None, no_opts=False, groups=TWO, g=1, step=A5, out=A6):
    return [None if no_opts else ctypes.byref(opts if opts is not None else _opts()), None if groups is None else _table(groups), g, step, out, None]


LR_REFUSALS = [
    ("null step counter", _lr(step=None), E_NULL),
    ("null result", _lr(out=None), E_NULL),
    ("null table", _lr(groups=None), E_NULL),
    ("null options", _lr(no_opts=True), E_NULL),
    ("group below 0", _lr(g=-1), E_SHAPE),
    ("group = 8", _lr(g=8), E_SHAPE),
    ("the group's lr < 0", _lr(groups=[_hyper(), _hyper(lr=-1.0)]), E_VALUE),
    ("the group's lr = NaN", _lr(groups=[_hyper(), _hyper(lr=NAN)]), E_VALUE),
    ("unknown schedule", _lr(opts=_opts(schedule=7)), E_VALUE),
    ("cosine with total = warmup", _lr(opts=_opts(schedule=1, warmup=2, total=2)), E_VALUE),
]


@pytest.mark.parametrize("what,args,code", LR_REFUSALS, ids=[r[0] for r in LR_REFUSALS])
def test_group_lr_refusals(what, args, code):
    _refused("goalnet_group_lr", args, code, what)


# ---- ParamGroup and OptimOptions ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kw", [
    dict(match="visbl."), dict(match=()), dict(match=("visbl.", "")), dict(match=(3,)),
    dict(match=("a",), lr=-1e-3), dict(match=("a",), lr=NAN), dict(match=("a",), lr=True), dict(match=("a",), lr="1e-3"),
    dict(match=("a",), betas=(0.9,)), dict(match=("a",), betas=(0.9, 1.0)), dict(match=("a",), betas=(-0.1, 0.5)), dict(match=("a",), betas=0.9),
    dict(match=("a",), eps=-1e-8), dict(match=("a",), eps=INF), dict(match=("a",), weight_decay=-0.1), dict(match=("a",), weight_decay=NAN),
    dict(match=("a",), amsgrad="yes")], ids=repr)
def test_param_group_validation(kw):
    with pytest.raises(ValueError):
        ParamGroup(**kw)


def test_param_group_is_frozen_and_normalised():
    g = ParamGroup(["visbl.", "audbl."], lr=1, betas=[0.8, 0.5], amsgrad=1)
    assert g.match == ("visbl.", "audbl.") and g.lr == 1.0 and isinstance(g.lr, float) and g.betas == (0.8, 0.5) and g.amsgrad is True
    with pytest.raises(Exception):
        g.lr = 2.0
    assert ParamGroup(("a",)).signature() == (("a",), None, None, None, None, None)
    hash(g.signature())


def test_optim_options_groups_validation_and_trivial():
    g = ParamGroup(("visbl.",), lr=1e-4)
    for bad in (g, (("visbl.",),), [{"params": []}]):
        with pytest.raises(ValueError):
            OptimOptions(groups=bad)
    with pytest.raises(ValueError, match="7"):
        OptimOptions(groups=(g,) * 8)
    with pytest.raises(ValueError):
        OptimOptions(amsgrad="no")
    assert OptimOptions(groups=(g,) * 7).groups == (g,) * 7 and OptimOptions(groups=[g]).groups == (g,)
    assert OptimOptions().trivial and OptimOptions().signature() == () and not OptimOptions().grouped
    assert not OptimOptions(groups=(g,)).trivial and not OptimOptions(amsgrad=True).trivial
    assert OptimOptions(groups=(g,)).grouped and OptimOptions(amsgrad=True).grouped and not OptimOptions(weight_decay=0.1).grouped


def test_signature_is_todays_without_groups_and_distinct_with_them():
    assert OptimOptions(weight_decay=0.01).signature() == (0.01, False, (), None, "constant", 0, None, 0.0, None, 0.1)
    a, b = ParamGroup(("visbl.",), lr=1e-4), ParamGroup(("fusion.12",), betas=(0.8, 0.5), amsgrad=True)
    sets = [(), (a,), (b,), (a, b), (b, a), (ParamGroup(("visbl.",), lr=2e-4),), (ParamGroup(("visbl.",), lr=1e-4, weight_decay=0.0),)]
    sigs = [OptimOptions(weight_decay=0.01, groups=s, amsgrad=f).signature() for s in sets for f in (False, True)]
    assert len({hash(s) for s in sigs}) == len(set(sigs)) == len(sigs)
    assert sigs[0] == OptimOptions(weight_decay=0.01).signature()
    assert all(s[:10] == sigs[0] and len(s) == 12 for s in sigs[1:])


def test_group_of_and_hyper_table():
    o = OptimOptions(weight_decay=0.01, amsgrad=True, groups=(ParamGroup(("visbl.",), lr=1e-4), ParamGroup(("conv", "fusion.12"), betas=(0.8, 0.5),
                                                                                                          eps=1e-6, weight_decay=0.0, amsgrad=False)))
    assert o.group_of("visbl.conv1.weight") == 1, "the first match wins"
    assert o.group_of("audbl.conv1.weight") == 2 and o.group_of("fusion.12.bias") == 2 and o.group_of("fusion.0.weight") == 0
    assert o.hyper_table(1e-3, (0.9, 0.999), 1e-8) == [(1e-3, 0.9, 0.999, 1e-8, 0.01, True), (1e-4, 0.9, 0.999, 1e-8, 0.01, True),
                                                       (1e-3, 0.8, 0.5, 1e-6, 0.0, False)]


# ---- group_ranges on the real spec list -------------------------------------------------------------------------------------------------
def _specs():
    m = AVM(audio_included=True)
    specs = m._param_specs(HW3, L2)
    return specs, {s.name: s for s in specs}


def _members(ranges, by):
    """name -> the range that holds the tensor, None if none; a tensor never straddles ranges"""
    out = {}
    for n, s in by.items():
        hit = [r for r in ranges if r[0] <= s.offset and s.offset + s.numel <= r[0] + r[1]]
        assert len(hit) <= 1 and (hit or not any(r[0] < s.offset + s.numel and s.offset < r[0] + r[1] for r in ranges)), n
        out[n] = hit[0] if hit else None
    return out


def test_group_ranges_on_the_real_specs():
    specs, by = _specs()
    assert len(specs) == 30
    args = (1e-3, (0.9, 0.999), 1e-8)
    last = max(specs, key=lambda s: s.offset)
    whole = (0, last.offset + last.numel)

    # no groups: optim_ranges with group 0 appended, and one table row
    o = OptimOptions(weight_decay=0.01, no_decay=("bias", "bnorm"), amsgrad=True)
    rs, table = group_ranges(specs, frozenset(), {}, o, *args)
    assert rs == [r + (0,) for r in optim_ranges(specs, frozenset(), {}, o)] and table == [(1e-3, 0.9, 0.999, 1e-8, 0.01, True)]
    rs, _ = group_ranges(specs, frozenset(), {}, OptimOptions(amsgrad=True), *args)
    assert rs == [whole + (0, False, 0)], "neighbours merge across the slot padding"

    # first match wins; every tensor sits in a range of its own group, sorted, disjoint, aligned
    o = OptimOptions(groups=(ParamGroup(("visbl.",), lr=1e-4), ParamGroup(("conv1", "fusion.12"), amsgrad=True)))
    rs, table = group_ranges(specs, frozenset(), {}, o, *args)
    mem = _members(rs, by)
    assert all(mem[n] is not None and mem[n][4] == o.group_of(n) for n in by)
    assert mem["visbl.conv1.weight"][4] == 1 and mem["audbl.conv1.weight"][4] == 2 and mem["fusion.12.weight"][4] == 2 and mem["fusion.0.weight"][4] == 0
    assert all(b % 4 == 0 and c > 0 for b, c, *_ in rs) and all(x[0] + x[1] <= y[0] for x, y in zip(rs, rs[1:]))
    assert all(x[2:] != y[2:] or x[0] + x[1] + 64 <= y[0] for x, y in zip(rs, rs[1:])), "equal neighbours would have merged"
    assert len(table) == 3 and table[1][0] == 1e-4 and table[2][5] is True and table[0][5] is False
    # the visbl.* tensors are neighbours in the arena: ONE range for the group
    assert len([r for r in rs if r[4] == 1]) == 1

    # an explicit group weight_decay beats no_decay; None keeps the rule
    o = OptimOptions(weight_decay=0.01, no_decay=("bias", "bnorm"), groups=(ParamGroup(("fusion.",), weight_decay=0.05), ParamGroup(("audbl.",), weight_decay=0.0),
                                                                            ParamGroup(("visbl.conv",), lr=1e-4)))
    rs, table = group_ranges(specs, frozenset(), {}, o, *args)
    mem = _members(rs, by)
    assert mem["fusion.0.bias"][3] is True and mem["fusion.0.weight"][3] is True and mem["fusion.0.bias"] == mem["fusion.0.weight"]
    assert mem["audbl.conv1.weight"][3] is False and mem["audbl.conv1.bias"][3] is False
    assert mem["visbl.conv1.weight"][3] is True and mem["visbl.conv1.bias"][3] is False and mem["visbl.conv1.weight"][4] == 3
    assert mem["visbl.linear5.weight"][3] is True and mem["visbl.linear5.bias"][3] is False and mem["visbl.linear5.bias"][4] == 0
    assert [t[4] for t in table] == [0.01, 0.05, 0.0, 0.01]

    # the count of sat-out steps splits a group's range, and frozen tensors drop out
    o = OptimOptions(groups=(ParamGroup(("visbl.",), lr=1e-4),))
    rs, _ = group_ranges(specs, frozenset(), {"visbl.conv2.weight": 2, "visbl.conv2.bias": 2}, o, *args)
    mem = _members(rs, by)
    assert [r[2] for r in rs if r[4] == 1].count(2) == 1 and len([r for r in rs if r[4] == 1]) in (2, 3), "the group's one range is cut around conv2"
    assert mem["visbl.conv2.weight"] == mem["visbl.conv2.bias"] and mem["visbl.conv2.weight"][2:] == (2, False, 1)
    assert all(mem[n][2] == 0 for n in by if "visbl.conv2." not in n)
    frozen = frozenset({"visbl.conv1.weight", "visbl.conv1.bias", "fusion.3.weight"})
    rs, _ = group_ranges(specs, frozen, {}, o, *args)
    mem = _members(rs, by)
    assert all((mem[n] is None) == (n in frozen) for n in by)
    assert group_ranges(specs, frozenset(by), {}, o, *args)[0] == []


def test_more_than_32_group_ranges_raise():
    specs = []
    for i in range(34):
        s = _Spec(f"t{i}.{'a' if i % 2 else 'b'}", "vec", (8,), 8)
        s.offset = 64 * i
        specs.append(s)
    o = OptimOptions(groups=(ParamGroup((".a",), lr=1e-4),))
    with pytest.raises(GoalnetError, match="34 trainable ranges"):
        group_ranges(specs, frozenset(), {}, o, 1e-3, (0.9, 0.999), 1e-8)
    rs, _ = group_ranges(specs[:32], frozenset(), {}, o, 1e-3, (0.9, 0.999), 1e-8)
    assert len(rs) == 32 and [r[4] for r in rs] == [0, 1] * 16


# ---- the drop-in optimizer -----------------------------------------------------------------------------------------------------------------
def _cpu_model():
    m = AVM(audio_included=True, device="cpu")
    return m


def test_drop_in_adam_accepts_groups_and_amsgrad():
    m = _cpu_model()
    opt = O.Adam([{"params": list(m.visbl.parameters()), "lr": 1e-4}, {"params": list(m.audbl.parameters()) + list(m.fusion.parameters())}],
                 lr=1e-3, amsgrad=True, model=m)
    assert len(opt.param_groups) == 2 and opt.param_groups[0]["lr"] == 1e-4 and opt.param_groups[1]["lr"] == 1e-3
    assert opt.param_groups[1]["betas"] == (0.9, 0.999) and opt.param_groups[0]["weight_decay"] is None
    sched = torch.optim.lr_scheduler.StepLR(opt, step_size=1, gamma=0.5)
    assert sched.get_last_lr() == [1e-4, 1e-3]
    w = O.AdamW([{"params": list(m.visbl.parameters()), "weight_decay": 0.0, "betas": (0.8, 0.5), "eps": 1e-6, "amsgrad": False},
                 {"params": list(m.audbl.parameters()) + list(m.fusion.parameters())}], lr=1e-3, amsgrad=True, model=m)
    assert w.options.weight_decay == 1e-2 and w.options.decoupled
    assert len(O.Adam(m.parameters(), lr=1e-3, model=m).param_groups) == 1


@pytest.mark.parametrize("group", [{"foreach": True}, {"capturable": False}, {"maximize": True}, {"momentum": 0.9}, {"lr": -1.0}, {"betas": (0.9, 1.0)},
                                   {"weight_decay": -0.1}], ids=repr)
def test_drop_in_adam_rejects_unknown_or_invalid_group_keys(group):
    m = _cpu_model()
    with pytest.raises(ValueError):
        O.Adam([{"params": list(m.visbl.parameters()), **group}, {"params": list(m.audbl.parameters()) + list(m.fusion.parameters())}], model=m)


def test_drop_in_adam_rejects_too_many_groups_and_groups_inside_options():
    m = _cpu_model()
    ps = list(m.parameters())
    with pytest.raises(ValueError, match="7"):
        O.Adam([{"params": [p]} for p in ps[:8]], model=m)
    with pytest.raises(ValueError, match="groups"):
        O.Adam(ps, model=m, options=OptimOptions(groups=(ParamGroup(("visbl.",), lr=1e-4),)))


def test_drop_in_adam_step_rejects_a_partial_union():
    m = AVM(audio_included=True)
    m._specs = m._param_specs(HW3, L2)
    m._garena = object()                              # "a backward has run": step() looks at the parameter sets before any launch
    opt = O.Adam([{"params": list(m.visbl.parameters()), "lr": 1e-4}, {"params": list(m.fusion.parameters())}], lr=1e-3, amsgrad=True, model=m)
    with pytest.raises(RuntimeError, match="ALL parameters"):
        opt.step()
