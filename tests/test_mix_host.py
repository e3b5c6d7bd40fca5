"""CPU: audio augmentation and mixup on a shuffled / augmented pass (include/goalnet_mix.h) — what holds without a
GPU: the eighth header against its ctypes table and the built library, the untouched seven older headers and tables, the argument
refusals of the four entry points (every one returns before any launch; pointers are small fake integers, as in
tests/test_epoch_host.py), the properties of the numpy restatement the GPU tests compare against, and VideoTrainer's validation."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

import _augment_ref as R
import _mix_ref as M
from cvml_goalnet_amd import AVM, _lib, augment, ops, synth
from cvml_goalnet_amd.loop import TRAINER_STATE_FORMAT, VideoTrainer

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
E_NULL, E_SHAPE, E_ALIGN, E_VALUE = -1, -2, -3, -5
A, A2, A3, A4, A5 = 4096, 8192, 12288, 16384, 20480        # fake, 16-byte aligned "device addresses": never dereferenced
NAN, INF = float("nan"), float("inf")
OLDER_HEADERS = ("goalnet_hip.h", "goalnet_loss.h", "goalnet_epoch.h", "goalnet_optim.h", "goalnet_ema.h", "goalnet_accum.h", "goalnet_groups.h")
OLDER_TABLES = ("PROTOTYPES", "LOSS_PROTOTYPES", "EPOCH_PROTOTYPES", "OPTIM_PROTOTYPES", "EMA_PROTOTYPES", "ACCUM_PROTOTYPES", "GROUPS_PROTOTYPES")
ONE = M.ONE


def _header(name="goalnet_mix.h"):
    return open(os.path.join(ROOT, "include", name)).read()


def _declared():
    text = re.sub(r"/\*.*?\*/", "", _header(), flags=re.S)
    return sorted(set(re.findall(r"\b(goalnet_[a-z0-9_]+)\s*\(", text)))


def test_mix_header_and_binding_agree():
    assert _declared() == sorted(_lib.MIX_PROTOTYPES) == ["goalnet_audio_gather_aug", "goalnet_epoch_plan2", "goalnet_frames_gather_mix",
                                                          "goalnet_rows_mix_indexed"]
    if not os.path.exists(_lib.LIB_PATH):
        import __graft_entry__ as g
        g.build()
    lib = ctypes.CDLL(_lib.LIB_PATH)
    for name in _declared():
        assert hasattr(lib, name), f"{name} missing from libgoalnet_hip.so"
    loaded = _lib.load()
    for name, (res, args) in _lib.MIX_PROTOTYPES.items():
        fn = getattr(loaded, name)
        assert fn.restype is res and list(fn.argtypes) == args, f"{name} was not bound by _lib.load()"


def test_mix_constants_match_the_header():
    h = _header()
    for name, want in (("TID_PLAN2", synth.TID_PLAN2), ("PLAN2_WORDS", _lib.PLAN2_WORDS), ("PLAN2_MAX_INDEX", _lib.PLAN2_MAX_INDEX),
                       ("AUDIO_GAIN", _lib.AUDIO_GAIN), ("AUDIO_NOISE", _lib.AUDIO_NOISE), ("AUDIO_MIX", _lib.AUDIO_MIX)):
        assert int(re.search(rf"#define GOALNET_{name} (\d+)", h).group(1)) == want, name
    assert synth.TID_PLAN2 == M.TID_PLAN2 == 3 * 2 ** 30 and _lib.PLAN2_WORDS == 12 and _lib.PLAN2_MAX_INDEX == 2 ** 26
    # above every stream of the first plan, and inside the 32 bits of a tensor id up to the last pass
    assert synth.TID_PLAN2 > synth.TID_PLAN + 8 * (2 ** 28 - 1) + 7 and synth.TID_PLAN2 + 16 * (2 ** 26 - 1) + 15 < 2 ** 32
    fields = re.search(r"typedef struct \{(.*?)\} goalnet_rowmix;", h, flags=re.S).group(1)
    assert re.findall(r"(\w+);", fields) == [f[0] for f in _lib.RowMix._fields_]


def test_the_seven_older_headers_and_tables_are_untouched_by_these_names():
    assert _lib.ABI_VERSION == 7 and _lib.load().goalnet_abi_version() == 7
    assert "#define GOALNET_ABI_VERSION 7" in _header("goalnet_hip.h")
    for table in OLDER_TABLES:
        assert set(_lib.MIX_PROTOTYPES).isdisjoint(getattr(_lib, table)), table
    for other in OLDER_HEADERS:
        text = _header(other)
        for name in (*_lib.MIX_PROTOTYPES, "goalnet_rowmix", "GOALNET_PLAN2_WORDS", "GOALNET_TID_PLAN2", "GOALNET_AUDIO_"):
            assert name not in text, f"{name} belongs to include/goalnet_mix.h, not {other}"


def test_the_build_depends_on_the_header():
    assert '"goalnet_mix.h"' in open(os.path.join(ROOT, "__graft_entry__.py")).read()


# ---- argument refusals: every one before any launch --------------------------------------------------------------------------------
def _refused(name, args, code, what):
    lib = _lib.load()
    rc = getattr(lib, name)(*args)
    msg = lib.goalnet_last_error()
    assert rc == code, f"{name}, {what}: rc = {rc}, expected {code} ({msg!r})"
    assert rc < 0 and msg, f"{name}, {what}: no error message"


# goalnet_epoch_plan2(plan2, plan, n, seed, index, C, B, max_shift, time_mask, coeff_mask, gain, noise, strength, p, stream)
def _p2(plan2=A, plan=A2, n=10, index=0, C=30, B=30, max_shift=3, time_mask=6, coeff_mask=5, gain=0.25, noise=0.5, strength=0.5, p=0.5):
    return [plan2, plan, n, 1, index, C, B, max_shift, time_mask, coeff_mask, gain, noise, strength, p, None]


PLAN2_REFUSALS = [
    ("plan2 = NULL", _p2(plan2=None), E_NULL),
    ("plan = NULL", _p2(plan=None), E_NULL),
    ("misaligned plan2", _p2(plan2=A + 8), E_ALIGN),
    ("misaligned plan", _p2(plan=A2 + 4), E_ALIGN),
    ("n = 0", _p2(n=0), E_SHAPE),
    ("n = -1", _p2(n=-1), E_SHAPE),
    ("n = 65537", _p2(n=65537), E_SHAPE),
    ("C = 0", _p2(C=0, coeff_mask=0), E_SHAPE),
    ("B = 0", _p2(B=0, time_mask=0), E_SHAPE),
    ("C * B = 2^31", _p2(C=32768, B=65536), E_SHAPE),
    ("max_shift = -1", _p2(max_shift=-1), E_VALUE),
    ("max_shift = 32768", _p2(max_shift=32768), E_VALUE),
    ("time_mask = -1", _p2(time_mask=-1), E_VALUE),
    ("time_mask = B + 1", _p2(time_mask=31), E_VALUE),
    ("coeff_mask = -1", _p2(coeff_mask=-1), E_VALUE),
    ("coeff_mask = C", _p2(coeff_mask=30), E_VALUE),
    ("gain = 1", _p2(gain=1.0), E_VALUE),
    ("gain < 0", _p2(gain=-0.1), E_VALUE),
    ("gain = NaN", _p2(gain=NAN), E_VALUE),
    ("noise < 0", _p2(noise=-0.5), E_VALUE),
    ("noise = inf", _p2(noise=INF), E_VALUE),
    ("noise = NaN", _p2(noise=NAN), E_VALUE),
    ("strength > 1", _p2(strength=1.5), E_VALUE),
    ("strength < 0", _p2(strength=-0.5), E_VALUE),
    ("strength = NaN", _p2(strength=NAN), E_VALUE),
    ("p > 1", _p2(p=1.01), E_VALUE),
    ("p < 0", _p2(p=-0.01), E_VALUE),
    ("p = NaN", _p2(p=NAN), E_VALUE),
    ("index = 2^26", _p2(index=1 << 26), E_VALUE),
]


@pytest.mark.parametrize("what,args,code", PLAN2_REFUSALS, ids=[r[0] for r in PLAN2_REFUSALS])
def test_epoch_plan2_refuses_before_any_launch(what, args, code):
    _refused("goalnet_epoch_plan2", args, code, what)


# goalnet_audio_gather_aug(table, table_rows, out, plan, plan2, plan_rows, C, B, nrows, cursor, cursor_bias, flags, noise, stream)
def _ag(table=A, table_rows=23, out=A2, plan=A3, plan2=A4, plan_rows=23, C=30, B=30, nrows=10, cursor=A5, flags=7, noise=0.5):
    return [table, table_rows, out, plan, plan2, plan_rows, C, B, nrows, cursor, 0, flags, noise, None]


AUDIO_REFUSALS = [
    ("table = NULL", _ag(table=None), E_NULL),
    ("out = NULL", _ag(out=None), E_NULL),
    ("plan = NULL", _ag(plan=None), E_NULL),
    ("plan2 = NULL", _ag(plan2=None), E_NULL),
    ("cursor = NULL", _ag(cursor=None), E_NULL),
    ("misaligned plan", _ag(plan=A3 + 4), E_ALIGN),
    ("misaligned plan2", _ag(plan2=A4 + 8), E_ALIGN),
    ("nrows = 0", _ag(nrows=0), E_SHAPE),
    ("C = 0", _ag(C=0), E_SHAPE),
    ("B < 0", _ag(B=-3), E_SHAPE),
    ("an empty table", _ag(table_rows=0), E_SHAPE),
    ("an empty plan", _ag(plan_rows=0), E_SHAPE),
    ("a row of 2^31 elements", _ag(C=32768, B=65536), E_SHAPE),
    ("an unknown flag", _ag(flags=8), E_VALUE),
    ("a negative flag word", _ag(flags=-1), E_VALUE),
    ("noise < 0", _ag(noise=-1.0), E_VALUE),
    ("noise = inf", _ag(noise=INF), E_VALUE),
    ("noise = NaN", _ag(noise=NAN), E_VALUE),
]


@pytest.mark.parametrize("what,args,code", AUDIO_REFUSALS, ids=[r[0] for r in AUDIO_REFUSALS])
def test_audio_gather_aug_refuses_before_any_launch(what, args, code):
    _refused("goalnet_audio_gather_aug", args, code, what)


# goalnet_frames_gather_mix(table, table_rows, out, plan, plan2, plan_rows, C, H, W, nrows, cursor, cursor_bias, colour, stream)
def _fm(table=A, table_rows=23, out=A2, plan=A3, plan2=A4, plan_rows=23, C=3, H=40, W=40, nrows=10, cursor=A5):
    return [table, table_rows, out, plan, plan2, plan_rows, C, H, W, nrows, cursor, 0, 1, None]


FRAMES_REFUSALS = [
    ("table = NULL", _fm(table=None), E_NULL),
    ("out = NULL", _fm(out=None), E_NULL),
    ("plan = NULL", _fm(plan=None), E_NULL),
    ("plan2 = NULL", _fm(plan2=None), E_NULL),
    ("cursor = NULL", _fm(cursor=None), E_NULL),
    ("misaligned plan", _fm(plan=A3 + 4), E_ALIGN),
    ("misaligned plan2", _fm(plan2=A4 + 4), E_ALIGN),
    ("nrows = 0", _fm(nrows=0), E_SHAPE),
    ("W = 0", _fm(W=0), E_SHAPE),
    ("H < 0", _fm(H=-3), E_SHAPE),
    ("C = 0", _fm(C=0), E_SHAPE),
    ("an empty table", _fm(table_rows=0), E_SHAPE),
    ("an empty plan", _fm(plan_rows=0), E_SHAPE),
    ("a frame of 2^31 elements", _fm(C=8, H=16384, W=16384), E_SHAPE),
]


@pytest.mark.parametrize("what,args,code", FRAMES_REFUSALS, ids=[r[0] for r in FRAMES_REFUSALS])
def test_frames_gather_mix_refuses_before_any_launch(what, args, code):
    _refused("goalnet_frames_gather_mix", args, code, what)


def _seg(table=A, dst=A2, row_elems=1, nrows=10, cursor=A5, table_rows=23):
    return _lib.RowMix(table, dst, row_elems, nrows, cursor, 0, table_rows)


def _segs(*segs):
    return (_lib.RowMix * len(segs))(*segs)


ROWS_REFUSALS = [
    ("segs = NULL", [None, 1, A3, A4, 23, None], E_NULL),
    ("plan = NULL", [_segs(_seg()), 1, None, A4, 23, None], E_NULL),
    ("plan2 = NULL", [_segs(_seg()), 1, A3, None, 23, None], E_NULL),
    ("misaligned plan", [_segs(_seg()), 1, A3 + 8, A4, 23, None], E_ALIGN),
    ("misaligned plan2", [_segs(_seg()), 1, A3, A4 + 4, 23, None], E_ALIGN),
    ("no segment", [_segs(_seg()), 0, A3, A4, 23, None], E_SHAPE),
    ("five segments", [_segs(*[_seg()] * 5), 5, A3, A4, 23, None], E_SHAPE),
    ("an empty plan", [_segs(_seg()), 1, A3, A4, 0, None], E_SHAPE),
    ("table = NULL in segment 1", [_segs(_seg(), _seg(table=None)), 2, A3, A4, 23, None], E_NULL),
    ("dst = NULL", [_segs(_seg(dst=None)), 1, A3, A4, 23, None], E_NULL),
    ("cursor = NULL", [_segs(_seg(cursor=None)), 1, A3, A4, 23, None], E_NULL),
    ("rows of 0 elements", [_segs(_seg(row_elems=0)), 1, A3, A4, 23, None], E_SHAPE),
    ("rows of 2^31 elements", [_segs(_seg(row_elems=1 << 31)), 1, A3, A4, 23, None], E_SHAPE),
    ("nrows = 0", [_segs(_seg(nrows=0)), 1, A3, A4, 23, None], E_SHAPE),
    ("an empty table", [_segs(_seg(table_rows=0)), 1, A3, A4, 23, None], E_SHAPE),
]


@pytest.mark.parametrize("what,args,code", ROWS_REFUSALS, ids=[r[0] for r in ROWS_REFUSALS])
def test_rows_mix_indexed_refuses_before_any_launch(what, args, code):
    _refused("goalnet_rows_mix_indexed", args, code, what)


# ---- the restatement's own properties ---------------------------------------------------------------------------------------------
def _lam(p2):
    return p2[:, 7].copy().view(np.float32)


@pytest.mark.parametrize("B", [1, 7, 30, 61])
@pytest.mark.parametrize("n", [1, 2, 23, 1000])
def test_draw_ranges(n, B):
    C = 30
    opts = dict(M.ALL_ON, time_mask=min(6, B))
    for index in (0, 3):
        pl = R.plan(n, R.SEED, index, **R.ALL_ON)
        p2 = M.plan2(pl, R.SEED, index, C, B, **opts)
        a_shift, t0, tw, c0, cw, _, partner = (p2[:, k].astype(np.int64) for k in range(7))
        assert (np.abs(a_shift) <= opts["max_shift"]).all()
        assert (0 <= t0).all() and (0 <= tw).all() and (tw <= opts["time_mask"]).all() and (t0 + tw <= B).all()
        assert (0 <= cw).all() and (cw <= opts["coeff_mask"]).all() and (1 <= c0).all() and (c0 + cw <= C).all()
        assert (0 <= partner).all() and (partner < n).all()
        lam = _lam(p2)
        assert (lam >= np.float32(1) - np.float32(opts["strength"])).all() and (lam <= 1).all()
        gain = p2[:, 5].copy().view(np.float32)
        assert (np.abs(gain - 1) <= opts["gain"]).all()
        unmixed = p2[:, 7] == ONE
        assert np.array_equal(partner[unmixed], np.arange(n)[unmixed]), "an unmixed row names itself"
        assert (partner[~unmixed] != np.arange(n)[~unmixed]).all(), "a mixed row names another position"
        assert not p2[:, 10:].any()


def test_a_frames_draws_do_not_depend_on_shuffling():
    n = 1000
    shuffled = R.plan(n, index=2, **R.ALL_ON)
    ordered = R.plan(n, index=2, **dict(R.ALL_ON, shuffle=False))
    s2, o2 = M.plan2(shuffled, R.SEED, 2, **M.AUDIO_ON), M.plan2(ordered, R.SEED, 2, **M.AUDIO_ON)
    assert np.array_equal(o2[:, 6], np.arange(n)) and np.array_equal(s2[:, 6], np.arange(n))
    cols = [0, 1, 2, 3, 4, 5, 7, 8, 9]
    assert np.array_equal(s2[:, cols], o2[shuffled[:, 0]][:, cols])
    # with mixup the partner is a POSITION, and q == i compares positions: lambda and apply are the frame's own draws
    s2, o2 = M.plan2(shuffled, R.SEED, 2, **M.ALL_ON), M.plan2(ordered, R.SEED, 2, **M.ALL_ON)
    both = (s2[:, 7] != ONE) & (o2[shuffled[:, 0], 7] != ONE)
    assert both.sum() > 300 and np.array_equal(s2[both, 7], o2[shuffled[:, 0]][both, 7])


def test_everything_off_is_the_identity_table():
    for n in (1, 65, 1000):
        pl = R.plan(n, index=7, shuffle=True)
        want = np.zeros((n, 12), np.int32)
        want[:, 5] = want[:, 7] = ONE             # gain 1.0f, lambda 1.0f
        want[:, 6] = np.arange(n)
        assert np.array_equal(M.plan2(pl, R.SEED, 7), want)
        assert np.array_equal(M.plan2(pl, R.SEED, 7, strength=0.5, p=0.0), want) and np.array_equal(M.plan2(pl, R.SEED, 7, strength=0.0, p=1.0), want)


def _fired(p2, opts):
    n = len(p2)
    if opts.get("max_shift", 0) > 0:
        assert p2[:, 0].min() < 0 < p2[:, 0].max(), "both shift signs"
    else:
        assert not p2[:, 0].any()
    if opts.get("time_mask", 0) > 0:
        assert (p2[:, 2] > 0).any(), "a time mask of positive width"
    else:
        assert not p2[:, 1:3].any()
    if opts.get("coeff_mask", 0) > 0:
        assert (p2[:, 4] > 0).any(), "a coefficient mask of positive width"
    else:
        assert not p2[:, 3:5].any()
    gain = p2[:, 5].copy().view(np.float32)
    if opts.get("gain", 0) > 0:
        assert (gain < 1).any() and (gain > 1).any(), "gain"
    else:
        assert (gain == 1).all()
    assert p2[:, 8:10].any() == (opts.get("noise", 0) > 0), "noise keys"
    if opts.get("strength", 0) > 0 and opts.get("p", 0) > 0:
        assert (p2[:, 7] != ONE).any() and (p2[:, 7] == ONE).any(), "a mixed row and an unmixed row"
    else:
        assert (p2[:, 7] == ONE).all()


def test_the_plans_the_gpu_tests_use_do_fire():
    """seed / index / size combinations of tests/test_gpu_mix.py: a test must not pass on an augmentation that never happened"""
    for n in (63, 257, 1000):
        for index in (1, 2):
            for shuffle in (True, False):
                _fired(M.plan2(R.plan(n, R.SEED, index, shuffle=shuffle), R.SEED, index, **M.ALL_ON), M.ALL_ON)
    for opts in M.ALONE.values():
        _fired(M.plan2(R.plan(257, R.SEED, 1, shuffle=True), R.SEED, 1, **opts), opts)
    for B in (30, 7, 3, 61):                      # the gather tests: 23 rows, index 1
        opts = dict(M.ALL_ON, time_mask=min(6, B), coeff_mask=4)
        _fired(M.plan2(R.plan(R.TRAINER_FRAMES, R.SEED, 1, **R.ALL_ON), R.SEED, 1, 5 if B == 3 else 30, B, **opts), opts)
    # the trainer tests: 23 frames, passes 0..3 — every option fires in every pass, and each of the three sub-batches holds a mixed row
    for index in range(4):
        p2 = M.plan2(R.plan(R.TRAINER_FRAMES, R.TRAINER_SEED, index, **R.ALL_ON), R.TRAINER_SEED, index, **M.ALL_ON)
        _fired(p2, M.ALL_ON)
        mixed = p2[:, 7] != ONE
        assert 6 <= mixed.sum() <= 17 and mixed[:10].any() and mixed[10:20].any()
        p2m = M.plan2(R.plan(R.TRAINER_FRAMES, R.TRAINER_SEED, index), R.TRAINER_SEED, index, **M.MIX_ON)
        _fired(p2m, M.MIX_ON)


def _bits(*vals):
    return [int(v) for v in np.array(vals, np.float32).view(np.int32)]


def test_restatement_on_a_hand_made_plan():
    one, half, quarter, two = _bits(1.0, 0.5, 0.25, 2.0)
    pl = np.zeros((3, 8), np.int32)
    pl[:, 0] = [2, 0, 1]
    pl[:, 4] = one
    pl[1, 1] = 1                                  # position 1 (frame 0) is flipped
    # position 0: shift +1, mixed with position 1 at lambda 0.25; position 1: time mask [1, 2), gain 2; position 2: coefficient mask [1, 2)
    p2 = np.array([[1, 0, 0, 0, 0, one, 1, quarter, 0, 0, 0, 0],
                   [0, 1, 1, 0, 0, two, 1, one, 0, 0, 0, 0],
                   [0, 0, 0, 1, 1, one, 2, one, 0, 0, 0, 0]], np.int32)
    aud = np.arange(3 * 2 * 3, dtype=np.float32).reshape(3, 2, 3) + 1       # frame f, coefficient c, bin t -> 6 f + 3 c + t + 1
    g = M.audio_gather(aud, pl, p2, 0, 3, gain=True, mix=True)
    a0 = aud[2][:, [0, 0, 1]]                                               # shift +1: content moves right, bin 0 is replicated
    b0 = aud[0] * 2
    b0[1, 1] = 0                                                            # the partner's own gain and time mask; coefficient 0 is not masked
    assert np.array_equal(g[0], a0 * np.float32(0.25) + b0 * np.float32(0.75))
    assert np.array_equal(g[1], b0)
    assert np.array_equal(g[2], np.array([[7, 8, 9], [0, 0, 0]], np.float32))
    assert np.array_equal(M.audio_gather(aud, pl, p2, 0, 1)[0], a0), "no flag: neither gain nor mix"
    lab = np.array([10.0, 20.0, 30.0], np.float32)
    assert np.array_equal(M.rows_mix(lab, pl, p2, 0, 3), np.array([30 * 0.25 + 10 * 0.75, 10, 20], np.float32))
    frames = np.arange(3 * 1 * 1 * 2, dtype=np.float32).reshape(3, 1, 1, 2)
    f = M.frames_mix(frames, pl, p2, 0, 3, colour=False)
    assert np.array_equal(f[0, 0, 0], frames[2, 0, 0] * np.float32(0.25) + frames[0, 0, 0, ::-1] * np.float32(0.75)), "the partner is flipped"
    assert np.array_equal(f[1:], R.gather(frames, pl, 1, 2, False))
    # noise: inside [-noise, noise), the same for the same key, different for another
    p2[0, 8:10] = [123, 456]
    p2[1, 8:10] = [123, 457]
    nz = M.audio_gather(np.zeros_like(aud), pl, p2, 0, 2, noise=0.5)
    assert (np.abs(nz) <= 0.5).all() and not np.array_equal(nz[0], nz[1]) and np.unique(nz[0]).size == 6
    assert nz[1, 1, 1] == 0 and np.array_equal(nz, M.audio_gather(np.zeros_like(aud), pl, p2, 0, 2, noise=0.5))


# ---- Python-level validation, no GPU ------------------------------------------------------------------------------------------------
BAD_AUDIO = [dict(pitch=3), dict(max_shift=2, reverb=1), dict(max_shift=-1), dict(max_shift=32768), dict(max_shift=1.5), dict(max_shift=True),
             dict(time_mask=-1), dict(time_mask=2.0), dict(coeff_mask=30), dict(coeff_mask=-1), dict(coeff_mask="x"), dict(gain=1.0),
             dict(gain=-0.5), dict(gain=NAN), dict(noise=-1.0), dict(noise=INF), dict(noise=NAN), dict(noise="x"), [("gain", 0.5)], "gain"]
BAD_MIXUP = [dict(alpha=0.4), dict(strength=1.5), dict(strength=-0.1), dict(strength=NAN), dict(p=1.01), dict(p=-0.5), dict(p=NAN), dict(p="x"),
             [("p", 0.5)], "mixup"]


@pytest.mark.parametrize("aug", BAD_AUDIO, ids=str)
def test_video_trainer_refuses_a_bad_audio_augment(aug):
    with pytest.raises(ValueError):
        VideoTrainer(AVM(audio_included=True), audio_augment=aug)


@pytest.mark.parametrize("mix", BAD_MIXUP, ids=str)
def test_video_trainer_refuses_a_bad_mixup(mix):
    with pytest.raises(ValueError):
        VideoTrainer(AVM(audio_included=True), mixup=mix)


def test_video_trainer_refuses_what_the_model_cannot_take():
    with pytest.raises(ValueError, match="audio_included"):
        VideoTrainer(AVM(audio_included=False), audio_augment=dict(gain=0.25))
    with pytest.raises(ValueError, match="classifier|class labels"):
        VideoTrainer(AVM(audio_included=True, head="classifier"), mixup=dict(strength=0.5, p=0.5))
    # switched-off options are no request: these construct
    VideoTrainer(AVM(audio_included=False), audio_augment=dict(gain=0.0), mixup=dict(strength=0.5, p=0.5))
    VideoTrainer(AVM(audio_included=True, head="classifier"), mixup=dict(strength=0.5, p=0.0), audio_augment=dict(noise=0.5))


def test_time_mask_longer_than_the_bins_is_refused_before_anything_is_launched():
    tr = VideoTrainer(AVM(audio_included=True), audio_augment=dict(time_mask=8))
    with pytest.raises(ValueError, match="time_mask"):           # no GPU here: reaching any launch would raise something else
        tr.train_video(torch.zeros(4, 30, 7), torch.zeros(4, 3, 40, 40), torch.ones(4))
    assert tr.passes == 0 and tr._key is None, "nothing was allocated, no pass was counted"
    for kw in (dict(time_mask=31), dict(coeff_mask=30)):
        with pytest.raises(ValueError):
            ops.epoch_plan2(None, None, 10, 1, 0, 30, 30, **kw)


def test_video_trainer_accepts_the_options():
    m = AVM(audio_included=True)
    tr = VideoTrainer(m)
    assert tr.audio_augment == dict(max_shift=0, time_mask=0, coeff_mask=0, gain=0.0, noise=0.0) and tr.mixup == dict(strength=0.0, p=0.0)
    assert not tr._planned and tr._mix_sig == () and not tr._mix and not tr._audio_aug
    for kw in (dict(audio_augment=None, mixup=None), dict(audio_augment={}, mixup={}), dict(audio_augment=dict(gain=0.0, noise=0), mixup=dict(p=1.0)),
               dict(mixup=dict(strength=1.0))):
        off = VideoTrainer(m, **kw)
        assert not off._planned and off._mix_sig == () and set(off._signatures()) == set(tr._signatures()), kw
    tr = VideoTrainer(m, audio_augment=dict(time_mask=4))
    assert tr._planned and tr._audio_aug and not tr._mix and not tr.shuffle and not tr._augments, "an identity plan carries the new options"
    tr = VideoTrainer(m, mixup=dict(strength=0.1, p=1.0))
    assert tr._planned and tr._mix and not tr._audio_aug
    assert tr.mixup["strength"] == float(np.float32(0.1)), "the options are held as the fp32 values the draws use"
    with pytest.raises(ValueError):
        tr.train_video(torch.zeros(4, 30, 30), torch.zeros(4, 3, 40, 40), torch.ones(4), plan_index=1 << 26)


def test_signatures_of_a_default_trainer_are_unchanged():
    m = AVM(audio_included=True)
    assert TRAINER_STATE_FORMAT == 1
    assert sorted(VideoTrainer(m)._signatures()) == ["ema", "loss", "optim", "plan", "step", "subbatch_size"]
    on = VideoTrainer(m, audio_augment=M.AUDIO_ON, mixup=M.MIX_ON)
    sig = on._signatures()
    assert sorted(sig) == ["ema", "loss", "optim", "plan", "plan2", "step", "subbatch_size"]
    assert sig["plan2"] == on._mix_sig == (tuple(on.audio_augment.items()), tuple(on.mixup.items()))
    assert sig["plan"] == VideoTrainer(m)._signatures()["plan"], "the first plan's signature does not know the new options"
    other = VideoTrainer(m, audio_augment=M.AUDIO_ON, mixup=dict(strength=0.5, p=0.25))
    with pytest.raises(ValueError, match="plan2"):
        other.load_state_dict({"format": 1, "signatures": sig, "model_state": None, "passes": 0, "seed": 1})


def test_python_functions_refuse_without_a_gpu():
    for kw in (dict(max_shift=-1), dict(time_mask=-2), dict(coeff_mask=30), dict(gain=1.0), dict(noise=-0.5), dict(strength=2.0), dict(p=-1.0)):
        with pytest.raises(ValueError):
            augment.epoch_plan2(None, **kw)
    with pytest.raises(ValueError):
        ops.audio_augment_spec(gain=NAN)
    with pytest.raises(ValueError):
        ops.mixup_spec(p=NAN)
    assert ops.audio_augment_spec() == (0, 0, 0, 0.0, 0.0) and ops.mixup_spec() == (0.0, 0.0)
    assert augment.AUGMENT_KEYS == ("flip_p", "max_shift", "contrast", "brightness"), "the frame options stay what they were"
    import cvml_goalnet_amd
    for name in ("epoch_plan2", "gather_audio_augmented", "gather_mixed", "mix_rows"):
        assert getattr(cvml_goalnet_amd, name) is getattr(augment, name)
