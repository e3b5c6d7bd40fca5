"""CPU: gradient accumulation over the sub-batches of a window (include/goalnet_accum.h) — what holds without a GPU: the
sixth header against its ctypes table and the built library, the untouched other headers, the argument refusals of the entry point
(every one returns before any launch; pointers are small fake integers, as in tests/test_ema_host.py), the cut of a video's sub-batches
into windows, the Python-side ValueErrors, and the state of a default trainer, which is what it was."""
import ctypes
import os
import re

import pytest

from cvml_goalnet_amd import GoalnetError, _lib
from cvml_goalnet_amd.avm import AVM, accum_count, accum_windows
from cvml_goalnet_amd.loop import VideoTrainer

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
E_NULL, E_SHAPE, E_ALIGN, E_VALUE = -1, -2, -3, -5
A, A2 = 4096, 8192                                 # fake, 16-byte aligned "device addresses": never dereferenced
OTHER_HEADERS = ("goalnet_hip.h", "goalnet_loss.h", "goalnet_epoch.h", "goalnet_optim.h", "goalnet_ema.h")


def _header(name="goalnet_accum.h"):
    return open(os.path.join(ROOT, "include", name)).read()


def _declared():
    text = re.sub(r"/\*.*?\*/", "", _header(), flags=re.S)
    return sorted(set(re.findall(r"\b(goalnet_[a-z0-9_]+)\s*\(", text)))


def test_accum_header_and_binding_agree():
    assert _declared() == sorted(_lib.ACCUM_PROTOTYPES) == ["goalnet_grad_accum_dev_ranges"]
    if not os.path.exists(_lib.LIB_PATH):
        import __graft_entry__ as g
        g.build()
    lib = ctypes.CDLL(_lib.LIB_PATH)
    for name in _declared():
        assert hasattr(lib, name), f"{name} missing from libgoalnet_hip.so"
    loaded = _lib.load()
    for name, (res, args) in _lib.ACCUM_PROTOTYPES.items():
        fn = getattr(loaded, name)
        assert fn.restype is res and list(fn.argtypes) == args, f"{name} was not bound by _lib.load()"


def test_the_other_five_headers_are_untouched_by_these_names():
    assert _lib.ABI_VERSION == 7 and _lib.load().goalnet_abi_version() == 7
    assert "#define GOALNET_ABI_VERSION 7" in _header("goalnet_hip.h")
    for table in (_lib.PROTOTYPES, _lib.LOSS_PROTOTYPES, _lib.EPOCH_PROTOTYPES, _lib.OPTIM_PROTOTYPES, _lib.EMA_PROTOTYPES):
        assert set(_lib.ACCUM_PROTOTYPES).isdisjoint(table)
    for other in OTHER_HEADERS:
        text = _header(other)
        for name in _lib.ACCUM_PROTOTYPES:
            assert name not in text, f"{name} belongs to include/goalnet_accum.h, not {other}"


def test_the_build_depends_on_the_header():
    text = open(os.path.join(ROOT, "__graft_entry__.py")).read()
    assert '"goalnet_accum.h"' in text


# ---- argument refusals: every one before any launch ------------------------------------------------------------------------------------
def _ranges(rs):
    return (_lib.AdamRange * len(rs))(*[_lib.AdamRange(*r) for r in rs])


GOOD = [(0, 100, 0), (128, 7, 0)]
MANY = [(64 * r, 8, 0) for r in range(33)]


# goalnet_grad_accum_dev_ranges(acc, g, ranges, count, scale, first, stream)
def _acc(acc=A, g=A2, ranges=GOOD, count=None, scale=0.5, first=0):
    arr = None if ranges is None else _ranges(ranges)
    return [acc, g, arr, (len(ranges) if ranges else 1) if count is None else count, scale, first, None]


REFUSALS = [
    ("null accumulator", _acc(acc=None), E_NULL),
    ("null gradients", _acc(g=None), E_NULL),
    ("null ranges", _acc(ranges=None), E_NULL),
    ("scale = 0", _acc(scale=0.0), E_VALUE),
    ("scale < 0", _acc(scale=-0.25), E_VALUE),
    ("scale = NaN", _acc(scale=float("nan")), E_VALUE),
    ("scale = inf", _acc(scale=float("inf")), E_VALUE),
    ("scale = NaN, first", _acc(scale=float("nan"), first=1), E_VALUE),
    ("accumulator is the gradients", _acc(g=A), E_VALUE),
    ("accumulator is the gradients, first", _acc(g=A, first=1), E_VALUE),
    ("unsorted ranges", _acc(ranges=[GOOD[1], GOOD[0]]), E_SHAPE),
    ("overlapping ranges", _acc(ranges=[(0, 100, 0), (96, 8, 0)]), E_SHAPE),
    ("empty range", _acc(ranges=[(0, 0, 0)]), E_SHAPE),
    ("range below 0", _acc(ranges=[(-4, 8, 0)]), E_SHAPE),
    ("range begins off a multiple of 4", _acc(ranges=[(2, 8, 0)]), E_ALIGN),
    ("count = 0", _acc(count=0), E_SHAPE),
    ("count = 33", _acc(ranges=MANY), E_SHAPE),
    ("misaligned accumulator", _acc(acc=A + 4), E_ALIGN),
    ("misaligned gradients", _acc(g=A2 + 8), E_ALIGN),
]


@pytest.mark.parametrize("what,args,code", REFUSALS, ids=[r[0] for r in REFUSALS])
def test_grad_accum_refusals(what, args, code):
    lib = _lib.load()
    rc = lib.goalnet_grad_accum_dev_ranges(*args)
    msg = lib.goalnet_last_error()
    assert rc == code, f"{what}: rc = {rc}, expected {code} ({msg!r})"
    assert rc < 0 and msg, f"{what}: no error message"


# ---- the cut of a video into windows ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("k", [1, 2, 3, 7])
@pytest.mark.parametrize("sb", [1, 4, 10])
def test_accum_windows_properties(sb, k):
    for n_frames in range(1, 46):
        cut = accum_windows(n_frames, sb, k)
        rows = [r for r, _, _ in cut]
        assert sum(rows) == n_frames and len(cut) == -(-n_frames // sb)
        assert all(r == sb for r in rows[:-1]) and 1 <= rows[-1] <= sb, "the reference's sub-batches: full ones and a shorter last one"
        windows, i = [], 0
        while i < len(cut):
            length = cut[i][2]
            assert 1 <= length <= k and i + length <= len(cut)
            assert [(p, ln) for _, p, ln in cut[i:i + length]] == [(p, length) for p in range(length)], (n_frames, sb, k, cut)
            windows.append(length)
            i += length
        assert all(ln == k for ln in windows[:-1]), "only the last window may be shorter"
        if k == 1:
            assert windows == [1] * len(cut)


def test_accum_windows_by_hand():
    assert accum_windows(30, 4, 3) == [(4, 0, 3), (4, 1, 3), (4, 2, 3), (4, 0, 3), (4, 1, 3), (4, 2, 3), (4, 0, 2), (2, 1, 2)]
    assert accum_windows(10, 10, 4) == [(10, 0, 1)]
    assert accum_windows(25, 10, 1) == [(10, 0, 1), (10, 0, 1), (5, 0, 1)]


# ---- the Python side refuses before anything is launched -------------------------------------------------------------------------------
@pytest.mark.parametrize("k", [0, -1, 1.0, 2.5, "2", None, True], ids=repr)
def test_accumulate_must_be_an_integer_of_at_least_one(k):
    with pytest.raises(ValueError, match="accumulate"):
        accum_count(k)
    with pytest.raises(ValueError, match="accumulate"):
        accum_windows(10, 4, k)
    with pytest.raises(ValueError, match="accumulate"):
        VideoTrainer(AVM(True, device="cpu"), accumulate=k)
    with pytest.raises(ValueError, match="accumulate"):
        AVM(True, device="cpu").train_step(None, None, None, accumulate=k)          # before the inputs are looked at


def test_model_level_refusals_need_no_gpu():
    m = AVM(True, device="cpu", precision="fp16")
    with pytest.raises(GoalnetError, match="fp16"):
        m.train_step(None, None, None, accumulate=2)
    m = AVM(True, device="cpu")
    m.grad_sync = object()
    with pytest.raises(GoalnetError, match="grad_sync"):
        m.train_step(None, None, None, accumulate=2)
    m = AVM(True, device="cpu")
    assert m.accum_position == (0, 1) and m._gacc is None
    with pytest.raises(GoalnetError, match="no accumulated gradient"):
        m.accum_of("fusion.0.weight")


def test_a_default_trainers_state_is_unchanged():
    m = AVM(True, device="cpu")
    plain, one, three = VideoTrainer(m), VideoTrainer(m, accumulate=1), VideoTrainer(m, accumulate=3)
    assert plain._signatures() == one._signatures()
    assert set(plain._signatures()) == {"loss", "plan", "optim", "ema", "subbatch_size", "step"}
    assert three._signatures() == {**plain._signatures(), "accumulate": 3}
    assert plain._phase == (True, True, 1) and plain._step_kw() == {}
    # a state saved by a trainer without accumulation loads into one; one saved under accumulate=3 does not load into another window
    state = {"format": 1, "signatures": three._signatures()}
    with pytest.raises(ValueError, match="accumulate"):
        plain.load_state_dict(state)
