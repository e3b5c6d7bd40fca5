"""CPU: shuffled, augmented passes (include/goalnet_epoch.h) — what holds without a GPU: the third header against its
ctypes table and the built library, the untouched first two tables, the argument refusals of the new entry points (every one returns
before any launch; pointers are small fake integers, as in tests/test_abi.py), the properties of the numpy restatement the GPU tests
compare against, and VideoTrainer's argument validation."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

import _augment_ref as R
from cvml_goalnet_amd import AVM, _lib, augment, synth
from cvml_goalnet_amd.loop import VideoTrainer

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
E_NULL, E_SHAPE, E_ALIGN, E_VALUE = -1, -2, -3, -5
A, A2, A3, A4, A5 = 4096, 8192, 12288, 16384, 20480        # fake, 16-byte aligned "device addresses": never dereferenced
SIZES = (1, 2, 63, 64, 65, 256, 257, 1000, 4097, 65536)    # the sizes tests/test_gpu_epoch.py runs


def _header():
    return open(os.path.join(ROOT, "include", "goalnet_epoch.h")).read()


def _declared():
    text = re.sub(r"/\*.*?\*/", "", _header(), flags=re.S)
    return sorted(set(re.findall(r"\b(goalnet_[a-z0-9_]+)\s*\(", text)))


def test_epoch_header_and_binding_agree():
    assert _declared() == sorted(_lib.EPOCH_PROTOTYPES)
    if not os.path.exists(_lib.LIB_PATH):
        import __graft_entry__ as g
        g.build()
    lib = ctypes.CDLL(_lib.LIB_PATH)
    for name in _declared():
        assert hasattr(lib, name), f"{name} missing from libgoalnet_hip.so"
    loaded = _lib.load()
    for name, (res, args) in _lib.EPOCH_PROTOTYPES.items():
        fn = getattr(loaded, name)
        assert fn.restype is res and list(fn.argtypes) == args, f"{name} was not bound by _lib.load()"


def test_epoch_constants_match_the_header():
    h = _header()
    for name, want in (("TID_PLAN", synth.TID_PLAN), ("EPOCH_MAX_N", _lib.EPOCH_MAX_N), ("PLAN_WORDS", _lib.PLAN_WORDS),
                       ("MAX_SHIFT", _lib.MAX_SHIFT)):
        assert int(re.search(rf"#define GOALNET_{name} (\d+)", h).group(1)) == want, name
    assert (_lib.EPOCH_MAX_N, _lib.PLAN_WORDS, _lib.MAX_SHIFT) == (65536, 8, 32767)
    first = open(os.path.join(ROOT, "include", "goalnet_hip.h")).read()
    assert int(re.search(r"#define GOALNET_ROWCOPY_MAX (\d+)", first).group(1)) == _lib.ROWCOPY_MAX
    # the segment struct of the indexed copy is its own: goalnet_rowcopy keeps its seven fields
    assert [f[0] for f in _lib.RowCopy._fields_] == ["src", "dst", "row_bytes", "nrows", "gather", "cursor", "cursor_bias"]
    fields = re.search(r"typedef struct \{(.*?)\} goalnet_rowcopy_indexed;", h, flags=re.S).group(1)
    assert re.findall(r"(\w+);", fields) == [f[0] for f in _lib.RowCopyIndexed._fields_]


def test_first_two_tables_are_untouched():
    assert set(_lib.EPOCH_PROTOTYPES).isdisjoint(_lib.PROTOTYPES) and set(_lib.EPOCH_PROTOTYPES).isdisjoint(_lib.LOSS_PROTOTYPES)
    assert _lib.ABI_VERSION == 7 and _lib.load().goalnet_abi_version() == 7
    for hdr in ("goalnet_hip.h", "goalnet_loss.h"):
        text = open(os.path.join(ROOT, "include", hdr)).read()
        for name in _lib.EPOCH_PROTOTYPES:
            assert name + "(" not in text, f"{name} belongs to include/goalnet_epoch.h"


def _refused(name, args, code, what):
    lib = _lib.load()
    rc = getattr(lib, name)(*args)
    msg = lib.goalnet_last_error()
    assert rc == code, f"{name}, {what}: rc = {rc}, expected {code} ({msg!r})"
    assert rc < 0 and msg, f"{name}, {what}: no error message"


# goalnet_epoch_plan(plan, n, seed, index, shuffle, flip_p, max_shift, contrast, brightness, stream)
def _pl(plan=A, n=10, index=0, flip_p=0.5, max_shift=2, contrast=0.25, brightness=0.125):
    return [plan, n, 1, index, 1, flip_p, max_shift, contrast, brightness, None]


PLAN_REFUSALS = [
    ("plan = NULL", _pl(plan=None), E_NULL),
    ("misaligned plan", _pl(plan=A + 8), E_ALIGN),
    ("n = 0", _pl(n=0), E_SHAPE),
    ("n = -1", _pl(n=-1), E_SHAPE),
    ("n = 65537", _pl(n=65537), E_SHAPE),
    ("flip_p < 0", _pl(flip_p=-0.01), E_VALUE),
    ("flip_p > 1", _pl(flip_p=1.5), E_VALUE),
    ("flip_p = NaN", _pl(flip_p=float("nan")), E_VALUE),
    ("max_shift = -1", _pl(max_shift=-1), E_VALUE),
    ("max_shift = 32768", _pl(max_shift=32768), E_VALUE),
    ("contrast = 1", _pl(contrast=1.0), E_VALUE),
    ("contrast > 1", _pl(contrast=3.0), E_VALUE),
    ("contrast < 0", _pl(contrast=-0.1), E_VALUE),
    ("contrast = NaN", _pl(contrast=float("nan")), E_VALUE),
    ("brightness < 0", _pl(brightness=-0.1), E_VALUE),
    ("brightness = inf", _pl(brightness=float("inf")), E_VALUE),
    ("index = 2^28", _pl(index=1 << 28), E_VALUE),
]


@pytest.mark.parametrize("what,args,code", PLAN_REFUSALS, ids=[r[0] for r in PLAN_REFUSALS])
def test_epoch_plan_refuses_before_any_launch(what, args, code):
    _refused("goalnet_epoch_plan", args, code, what)


# goalnet_frames_gather_aug(table, table_rows, out, plan, plan_rows, C, H, W, nrows, cursor, cursor_bias, colour, stream)
def _ga(table=A, table_rows=23, out=A2, plan=A3, plan_rows=23, C=3, H=40, W=40, nrows=10, cursor=A4):
    return [table, table_rows, out, plan, plan_rows, C, H, W, nrows, cursor, 0, 1, None]


GATHER_REFUSALS = [
    ("table = NULL", _ga(table=None), E_NULL),
    ("out = NULL", _ga(out=None), E_NULL),
    ("plan = NULL", _ga(plan=None), E_NULL),
    ("cursor = NULL", _ga(cursor=None), E_NULL),
    ("misaligned plan", _ga(plan=A3 + 4), E_ALIGN),
    ("nrows = 0", _ga(nrows=0), E_SHAPE),
    ("W = 0", _ga(W=0), E_SHAPE),
    ("H < 0", _ga(H=-3), E_SHAPE),
    ("an empty table", _ga(table_rows=0), E_SHAPE),
    ("an empty plan", _ga(plan_rows=0), E_SHAPE),
    ("a frame of 2^31 elements", _ga(C=8, H=16384, W=16384), E_SHAPE),
]


@pytest.mark.parametrize("what,args,code", GATHER_REFUSALS, ids=[r[0] for r in GATHER_REFUSALS])
def test_frames_gather_aug_refuses_before_any_launch(what, args, code):
    _refused("goalnet_frames_gather_aug", args, code, what)


def _seg(src=A, dst=A2, row_bytes=4, nrows=10, gather=1, cursor=A4, indexed=1, table_rows=23):
    return _lib.RowCopyIndexed(src, dst, row_bytes, nrows, gather, cursor, 0, indexed, table_rows)


def _segs(*segs):
    return (_lib.RowCopyIndexed * len(segs))(*segs)


INDEXED_REFUSALS = [
    ("segs = NULL", [None, 1, A3, 23, None], E_NULL),
    ("plan = NULL", [_segs(_seg()), 1, None, 23, None], E_NULL),
    ("no segment", [_segs(_seg()), 0, A3, 23, None], E_SHAPE),
    ("five segments", [_segs(*[_seg()] * 5), 5, A3, 23, None], E_SHAPE),
    ("an empty plan", [_segs(_seg()), 1, A3, 0, None], E_SHAPE),
    ("src = NULL in segment 1", [_segs(_seg(), _seg(src=None)), 2, A3, 23, None], E_NULL),
    ("dst = NULL", [_segs(_seg(dst=None)), 1, A3, 23, None], E_NULL),
    ("cursor = NULL", [_segs(_seg(cursor=None)), 1, A3, 23, None], E_NULL),
    ("rows of 6 bytes", [_segs(_seg(row_bytes=6)), 1, A3, 23, None], E_SHAPE),
    ("rows of 0 bytes", [_segs(_seg(row_bytes=0)), 1, A3, 23, None], E_SHAPE),
    ("nrows = 0", [_segs(_seg(nrows=0)), 1, A3, 23, None], E_SHAPE),
    ("an indexed segment on an empty table", [_segs(_seg(table_rows=0)), 1, A3, 23, None], E_SHAPE),
]


@pytest.mark.parametrize("what,args,code", INDEXED_REFUSALS, ids=[r[0] for r in INDEXED_REFUSALS])
def test_rows_copy_indexed_refuses_before_any_launch(what, args, code):
    _refused("goalnet_rows_copy_indexed", args, code, what)


# ---- the restatement's own properties -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", SIZES)
def test_order_is_a_permutation(n):
    src = R.plan(n, index=3, **R.ALL_ON)[:, 0]
    assert np.array_equal(np.sort(src), np.arange(n))


def test_everything_off_is_the_identity_plan():
    for n in (1, 65, 1000):
        p = R.plan(n, index=7)
        want = np.zeros((n, 8), np.int32)
        want[:, 0] = np.arange(n)
        want[:, 4] = 0x3F800000                 # 1.0f
        assert np.array_equal(p, want)


def test_index_and_seed_change_the_order():
    n = 257
    base = R.plan(n, R.SEED, 0, shuffle=True)[:, 0]
    assert not np.array_equal(base, R.plan(n, R.SEED, 1, shuffle=True)[:, 0])
    assert not np.array_equal(base, R.plan(n, R.SEED + 1, 0, shuffle=True)[:, 0])
    assert np.array_equal(base, R.plan(n, R.SEED, 0, shuffle=True)[:, 0])


def test_a_frames_draws_do_not_depend_on_shuffling():
    n = 1000
    opts = dict(R.ALL_ON)
    shuffled = R.plan(n, index=2, **opts)
    opts["shuffle"] = False
    ordered = R.plan(n, index=2, **opts)
    assert np.array_equal(ordered[:, 0], np.arange(n))
    assert np.array_equal(shuffled[:, 1:], ordered[shuffled[:, 0], 1:])


def _fired(p, opts):
    """every option that is on takes both a trivial and a non-trivial value somewhere in the plan"""
    n = len(p)
    if opts.get("shuffle"):
        assert not np.array_equal(p[:, 0], np.arange(n)), "the order is the identity"
    if opts.get("flip_p", 0) > 0:
        assert set(p[:, 1]) == {0, 1}, "flip"
    if opts.get("max_shift", 0) > 0:
        for col in (2, 3):
            assert (p[:, col] == 0).any() and (p[:, col] != 0).any(), "shift"
            assert p[:, col].min() < 0 < p[:, col].max() and np.abs(p[:, col]).max() <= opts["max_shift"]
    gain, bias = p[:, 4].copy().view(np.float32), p[:, 5].copy().view(np.float32)
    if opts.get("contrast", 0) > 0:
        assert (gain < 1).any() and (gain > 1).any() and (np.abs(gain - 1) <= opts["contrast"]).all(), "gain"
    else:
        assert (gain == 1).all()
    if opts.get("brightness", 0) > 0:
        assert (bias < 0).any() and (bias > 0).any() and (np.abs(bias) <= opts["brightness"]).all(), "bias"
    else:
        assert (bias == 0).all()


def test_the_plans_the_gpu_tests_use_do_fire():
    """seed / index / size combinations of tests/test_gpu_epoch.py: a test must not pass on an augmentation that never happened.
    (Continuous draws have no exactly trivial value; their both-sides-of-identity spread is what is checked.)"""
    for n in (63, 257, 1000):                   # the plan and gather tests: index 1 (and 2 for the plans)
        for index in (1, 2):
            _fired(R.plan(n, R.SEED, index, **R.ALL_ON), R.ALL_ON)
    for opts in R.ALONE.values():
        _fired(R.plan(257, R.SEED, 1, **opts), opts)
    # the trainer tests: 23 frames, passes 0..3 — every option fires in every pass, and the first sub-batch is not frames 0..9
    for index in range(4):
        p = R.plan(R.TRAINER_FRAMES, R.TRAINER_SEED, index, **R.ALL_ON)
        _fired(p, R.ALL_ON)
        assert not np.array_equal(np.sort(p[:10, 0]), np.arange(10))
        assert not np.array_equal(p[:, 0], R.plan(R.TRAINER_FRAMES, R.TRAINER_SEED, (index + 1) % 4, **R.ALL_ON)[:, 0])


def test_gather_restatement_on_a_hand_made_plan():
    t = np.arange(2 * 1 * 2 * 3, dtype=np.float32).reshape(2, 1, 2, 3) / 8          # frame 1 = [[.75 .875 1.0], [1.125 1.25 1.375]]
    one, half = np.array([1.0, 0.5], np.float32).view(np.int32)
    p = np.array([[1, 1, 0, 0, one, 0, 0, 0],          # flip
                  [1, 0, 1, 0, one, 0, 0, 0],          # dx = +1: content moves right, the left column is replicated
                  [1, 0, 0, -5, one, 0, 0, 0],         # dy = -5: every row is the last row
                  [1, 0, 0, 0, one, half, 0, 0]], np.int32)
    g = R.gather(t, p, 0, 4, colour=False)
    f1 = t[1, 0]
    assert np.array_equal(g[0, 0], f1[:, ::-1])
    assert np.array_equal(g[1, 0], f1[:, [0, 0, 1]])
    assert np.array_equal(g[2, 0], f1[[1, 1]])
    assert np.array_equal(g[3, 0], f1)
    c = R.gather(t, p, 3, 1, colour=True)
    assert np.array_equal(c[0, 0], np.minimum(f1 + np.float32(0.5), 1))


# ---- Python-level validation, no GPU ---------------------------------------------------------------------------------------------
BAD_AUGMENT = [dict(rotate=3), dict(flip_p=0.5, shear=1), dict(flip_p=-0.1), dict(flip_p=1.01), dict(flip_p=float("nan")), dict(flip_p="x"),
               dict(max_shift=-1), dict(max_shift=32768), dict(max_shift=1.5), dict(max_shift=True), dict(contrast=1.0), dict(contrast=-0.5),
               dict(brightness=-1.0), dict(brightness=float("inf")), [("flip_p", 0.5)], "flip"]


@pytest.mark.parametrize("aug", BAD_AUGMENT, ids=str)
def test_video_trainer_refuses_a_bad_augment(aug):
    with pytest.raises(ValueError):
        VideoTrainer(AVM(audio_included=True), augment=aug)


def test_video_trainer_accepts_the_options_and_counts_passes():
    m = AVM(audio_included=True)
    tr = VideoTrainer(m)
    assert (tr.shuffle, tr.passes, tr.seed, tr._planned) == (False, 0, synth.BASE_SEED, False)
    assert tr.augment == dict(flip_p=0.0, max_shift=0, contrast=0.0, brightness=0.0)
    assert not VideoTrainer(m, augment={})._planned and not VideoTrainer(m, augment=dict(flip_p=0.0, max_shift=0))._planned
    tr = VideoTrainer(m, shuffle=True, seed=5)
    assert tr._planned and not tr._colour and not tr._augments and tr.seed == 5
    tr = VideoTrainer(m, augment=dict(max_shift=2))
    assert tr._planned and tr._augments and not tr._colour
    tr = VideoTrainer(m, augment=dict(brightness=0.1))
    assert tr._planned and tr._augments and tr._colour
    assert tr.augment["brightness"] == float(np.float32(0.1)), "the options are held as the fp32 values the draws use"
    for bad in (-1, 1.0, True, 1 << 28):
        with pytest.raises(ValueError):
            tr.train_video(torch.zeros(4, 30, 30), torch.zeros(4, 3, 40, 40), torch.ones(4), plan_index=bad)


def test_epoch_plan_python_errors():
    for kw in (dict(flip_p=2.0), dict(max_shift=-1), dict(contrast=1.0), dict(brightness=-0.5)):
        with pytest.raises(ValueError):
            augment.epoch_plan(10, **kw)
    import cvml_goalnet_amd
    assert cvml_goalnet_amd.epoch_plan is augment.epoch_plan and cvml_goalnet_amd.gather_augmented is augment.gather_augmented
