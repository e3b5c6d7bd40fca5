"""CPU: the weight average behind the fused step (include/goalnet_ema.h) — what holds without a GPU: the fifth header
against its ctypes table and the built library, the untouched other headers, the argument refusals of the two entry points (every one
returns before any launch; pointers are small fake integers, as in tests/test_optim_host.py), EmaOptions, the path decision, and
weight_at against the float64 restatement tests/ema_ref.py, which is itself held against torch's AveragedModel."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

import ema_ref as R
from cvml_goalnet_amd import EmaOptions, GoalnetError, _lib
from cvml_goalnet_amd.avm import ema_step_path

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
E_NULL, E_SHAPE, E_ALIGN, E_VALUE = -1, -2, -3, -5
A, A2, A3, A4 = 4096, 8192, 12288, 16384          # fake, 16-byte aligned "device addresses": never dereferenced


def _header(name="goalnet_ema.h"):
    return open(os.path.join(ROOT, "include", name)).read()


def _declared():
    text = re.sub(r"/\*.*?\*/", "", _header(), flags=re.S)
    return sorted(set(re.findall(r"\b(goalnet_[a-z0-9_]+)\s*\(", text)))


def test_ema_header_and_binding_agree():
    assert _declared() == sorted(_lib.EMA_PROTOTYPES)
    if not os.path.exists(_lib.LIB_PATH):
        import __graft_entry__ as g
        g.build()
    lib = ctypes.CDLL(_lib.LIB_PATH)
    for name in _declared():
        assert hasattr(lib, name), f"{name} missing from libgoalnet_hip.so"
    loaded = _lib.load()
    for name, (res, args) in _lib.EMA_PROTOTYPES.items():
        fn = getattr(loaded, name)
        assert fn.restype is res and list(fn.argtypes) == args, f"{name} was not bound by _lib.load()"


def test_the_other_four_headers_are_untouched_by_these_names():
    assert _lib.ABI_VERSION == 7 and _lib.load().goalnet_abi_version() == 7
    assert "#define GOALNET_ABI_VERSION 7" in _header("goalnet_hip.h")
    for table in (_lib.PROTOTYPES, _lib.LOSS_PROTOTYPES, _lib.EPOCH_PROTOTYPES, _lib.OPTIM_PROTOTYPES):
        assert set(_lib.EMA_PROTOTYPES).isdisjoint(table)
    for other in ("goalnet_hip.h", "goalnet_loss.h", "goalnet_epoch.h", "goalnet_optim.h"):
        text = _header(other)
        for name in (*_lib.EMA_PROTOTYPES, "goalnet_ema_opts"):
            assert name not in text, f"{name} belongs to include/goalnet_ema.h, not {other}"


def test_struct_matches_the_header():
    h = _header()
    assert ctypes.sizeof(_lib.EmaOpts) == 8 + 2 * 8 + 2 * 4
    opts = re.search(r"typedef struct \{([^}]*)\} goalnet_ema_opts;", h).group(1)
    assert re.findall(r"\b([a-z_0-9]+)\s*[,;]", opts) == [f for f, _ in _lib.EmaOpts._fields_]


# ---- argument refusals: every one before any launch ------------------------------------------------------------------------------------
def _ranges(rs):
    return (_lib.AdamRange * len(rs))(*[_lib.AdamRange(*r) for r in rs])


def _opts(decay=0.9, every=1, start=0, warmup=0):
    return _lib.EmaOpts(decay, every, start, warmup, 0)


GOOD = [(0, 100, 0), (128, 7, 0)]
MANY = [(64 * r, 8, 0) for r in range(33)]


# goalnet_ema_update_dev_ranges(p, e, ranges, count, opts, step, step_bias, bad_step, stream)
def _upd(p=A, e=A2, ranges=GOOD, count=None, opts=None, no_opts=False, step=A3, bad=None):
    o = None if no_opts else ctypes.byref(opts if opts is not None else _opts())
    arr = None if ranges is None else _ranges(ranges)
    return [p, e, arr, (len(ranges) if ranges else 1) if count is None else count, o, step, 1, bad, None]


UPDATE_REFUSALS = [
    ("null weights", _upd(p=None), E_NULL),
    ("null average", _upd(e=None), E_NULL),
    ("null step counter", _upd(step=None), E_NULL),
    ("null ranges", _upd(ranges=None), E_NULL),
    ("null options", _upd(no_opts=True), E_NULL),
    ("decay = 1", _upd(opts=_opts(decay=1.0)), E_VALUE),
    ("decay < 0", _upd(opts=_opts(decay=-0.1)), E_VALUE),
    ("decay = NaN", _upd(opts=_opts(decay=float("nan"))), E_VALUE),
    ("decay = inf", _upd(opts=_opts(decay=float("inf"))), E_VALUE),
    ("every = 0", _upd(opts=_opts(every=0)), E_VALUE),
    ("start_step < 0", _upd(opts=_opts(start=-1)), E_VALUE),
    ("average is the weights", _upd(e=A), E_VALUE),
    ("unsorted ranges", _upd(ranges=[GOOD[1], GOOD[0]]), E_SHAPE),
    ("overlapping ranges", _upd(ranges=[(0, 100, 0), (96, 8, 0)]), E_SHAPE),
    ("empty range", _upd(ranges=[(0, 0, 0)]), E_SHAPE),
    ("range begins off a multiple of 4", _upd(ranges=[(2, 8, 0)]), E_ALIGN),
    ("count = 0", _upd(count=0), E_SHAPE),
    ("count = 33", _upd(ranges=MANY), E_SHAPE),
    ("misaligned weights", _upd(p=A + 4), E_ALIGN),
    ("misaligned average", _upd(e=A2 + 8), E_ALIGN),
    ("misaligned counter", _upd(step=A3 + 4), E_ALIGN),
    ("misaligned guard word", _upd(bad=A4 + 4), E_ALIGN),
]


def _refused(name, args, code, what):
    lib = _lib.load()
    rc = getattr(lib, name)(*args)
    msg = lib.goalnet_last_error()
    assert rc == code, f"{name}, {what}: rc = {rc}, expected {code} ({msg!r})"
    assert rc < 0 and msg, f"{name}, {what}: no error message"


@pytest.mark.parametrize("what,args,code", UPDATE_REFUSALS, ids=[r[0] for r in UPDATE_REFUSALS])
def test_ema_update_refusals(what, args, code):
    _refused("goalnet_ema_update_dev_ranges", args, code, what)


# goalnet_swap_ranges(a, b, ranges, count, stream)
SWAP_REFUSALS = [
    ("null a", [None, A2, _ranges(GOOD), 2, None], E_NULL),
    ("null b", [A, None, _ranges(GOOD), 2, None], E_NULL),
    ("null ranges", [A, A2, None, 1, None], E_NULL),
    ("the same arena twice", [A, A, _ranges(GOOD), 2, None], E_VALUE),
    ("unsorted ranges", [A, A2, _ranges([GOOD[1], GOOD[0]]), 2, None], E_SHAPE),
    ("range begins off a multiple of 4", [A, A2, _ranges([(6, 8, 0)]), 1, None], E_ALIGN),
    ("count = 33", [A, A2, _ranges(MANY), 33, None], E_SHAPE),
    ("misaligned arena", [A, A2 + 4, _ranges(GOOD), 2, None], E_ALIGN),
]


@pytest.mark.parametrize("what,args,code", SWAP_REFUSALS, ids=[r[0] for r in SWAP_REFUSALS])
def test_swap_refusals(what, args, code):
    _refused("goalnet_swap_ranges", args, code, what)


# ---- EmaOptions ----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kw", [
    dict(decay=1.0), dict(decay=-0.01), dict(decay=float("nan")), dict(decay=float("inf")), dict(decay="0.9"), dict(decay=True),
    dict(every=0), dict(every=-2), dict(every=1.5), dict(every=True), dict(start_step=-1), dict(start_step=0.5), dict(warmup="yes"),
], ids=lambda kw: ",".join(f"{k}={v}" for k, v in kw.items()))
def test_options_validate_in_the_constructor(kw):
    with pytest.raises(ValueError):
        EmaOptions(**kw)


def test_options_defaults_and_signature():
    e = EmaOptions()
    assert (e.decay, e.warmup, e.every, e.start_step) == (0.999, False, 1, 0)
    sigs = {EmaOptions().signature(), EmaOptions(decay=0.9).signature(), EmaOptions(warmup=True).signature(),
            EmaOptions(every=2).signature(), EmaOptions(start_step=3).signature()}
    assert len(sigs) == 5, "options that bake different launch arguments have different signatures"
    assert EmaOptions(decay=0).signature() == EmaOptions(decay=0.0).signature()
    hash(e.signature())
    with pytest.raises(Exception):
        e.decay = 0.5                                                                        # frozen


def test_path_decision():
    assert ema_step_path(None, sharded=False) is False and ema_step_path(None, sharded=True) is False
    assert ema_step_path(EmaOptions(), sharded=False) is True
    with pytest.raises(GoalnetError, match="shard_linear5"):
        ema_step_path(EmaOptions(), sharded=True)
    with pytest.raises(ValueError):
        ema_step_path({"decay": 0.9}, sharded=False)


def test_python_surface_refuses_before_any_launch():
    from cvml_goalnet_amd import optim as O
    from cvml_goalnet_amd.loop import VideoTrainer
    prm = [torch.nn.Parameter(torch.zeros(1))]
    with pytest.raises(ValueError):
        O.Adam(prm, ema=0.999)
    with pytest.raises(ValueError):
        O.AdamW(prm, ema={"decay": 0.9})
    assert O.Adam(prm).ema is None and O.AdamW(prm, ema=EmaOptions(0.5)).ema == EmaOptions(0.5)
    with pytest.raises(ValueError):
        VideoTrainer(object(), ema=0.999)


# ---- weight_at against the restatement, the restatement against torch ---------------------------------------------------------------------
@pytest.mark.parametrize("every", [1, 3])
@pytest.mark.parametrize("start", [0, 2])
@pytest.mark.parametrize("warmup", [False, True])
def test_weight_at_equals_the_restatement(every, start, warmup):
    o = EmaOptions(decay=0.97, warmup=warmup, every=every, start_step=start)
    seen = set()
    for t in range(1, 41):
        got, want = o.weight_at(t), R.weight(t, 0.97, every, start, warmup)
        assert got == want, (t, got, want)
        seen.add("none" if got is None else "copy" if t <= start else "avg")
    assert seen == {"avg"} | ({"none"} if every > 1 else set()) | ({"copy"} if start else set())
    if warmup:
        first = start + every
        # k = 0: d = 1 / 10; (1 + k) / (10 + k) passes the decay 0.97 at k = 290, from where the weight is 1 - decay
        assert o.weight_at(first) == 1.0 - 1.0 / 10.0 and o.weight_at(start + 301 * every) == 1.0 - 0.97


def test_restatement_by_hand():
    e, p = np.array([1.0, -2.0]), np.array([3.0, 2.0])
    e1, wrote, copied = R.update(e, p, 1, 0.75)
    assert wrote and not copied and np.array_equal(e1, np.array([1.5, -1.0]))
    e2, wrote, copied = R.update(e, p, 1, 0.75, start_step=1)
    assert wrote and copied and np.array_equal(e2, p)
    e3, wrote, _ = R.update(e, p, 3, 0.75, every=2)
    assert not wrote and e3 is e


def test_restatement_matches_torch_averaged_model():
    swa = pytest.importorskip("torch.optim.swa_utils")
    if not hasattr(swa, "get_ema_multi_avg_fn"):
        pytest.skip("this torch has no get_ema_multi_avg_fn")
    decay = 0.9
    torch.manual_seed(3)
    net = torch.nn.Linear(5, 3).double()
    avg = swa.AveragedModel(net, multi_avg_fn=swa.get_ema_multi_avg_fn(decay))
    flat = lambda m: np.concatenate([q.detach().numpy().ravel() for q in m.parameters()])      # noqa: E731
    e = flat(net)                                                     # before any update (t = 0) nothing has been written
    for t in range(1, 6):
        with torch.no_grad():
            for q in net.parameters():
                q.add_(torch.randn_like(q))
        avg.update_parameters(net)                                    # its first call copies: start_step = 1
        e, wrote, _ = R.update(e, flat(net), t, decay, every=1, start_step=1, warmup=False)
        assert wrote
        got = flat(avg.module)
        assert np.abs(got - e).max() <= 4 * 2.0 ** -52 * np.abs(e).max(), t
