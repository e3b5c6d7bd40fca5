"""CPU: the static summary (include/goalnet_storyboard.h, cvml_goalnet_amd/storyboard.py) — what holds without a GPU:
the eleventh header against its ctypes table and the built library, the untouched ten older headers and tables, every argument
refusal (each returns before any launch; device pointers are small fake integers, as in tests/test_nv12_host.py, the colour table is
real host memory), the oracle of the GPU tests (tests/storyboard_ref.py) against hand-worked cases and an evaluation in exact
fractions, and the Python-side validation."""
import ctypes
import os
import re
from fractions import Fraction

import numpy as np
import pytest
import torch

import storyboard_ref as S
from cvml_goalnet_amd import GoalnetError, VideoSummarizer, _lib, storyboard
from cvml_goalnet_amd.storyboard import check_options, clip_lengths, render_thumbnails, select_keyframes, sheet_shape

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
E_NULL, E_SHAPE, E_VALUE = -1, -2, -5
A, A2, A3, A4 = 4096, 8192, 12288, 16384          # fake, aligned "device addresses": never dereferenced
OLDER_HEADERS = ("goalnet_hip.h", "goalnet_loss.h", "goalnet_epoch.h", "goalnet_optim.h", "goalnet_ema.h", "goalnet_accum.h", "goalnet_groups.h",
                 "goalnet_mix.h", "goalnet_wave.h", "goalnet_nv12.h")
OLDER_TABLES = ("PROTOTYPES", "LOSS_PROTOTYPES", "EPOCH_PROTOTYPES", "OPTIM_PROTOTYPES", "EMA_PROTOTYPES", "ACCUM_PROTOTYPES", "GROUPS_PROTOTYPES",
                "MIX_PROTOTYPES", "WAVE_PROTOTYPES", "NV12_PROTOTYPES")
NAMES = ["goalnet_storyboard_keyframes", "goalnet_storyboard_render", "goalnet_storyboard_render_nv12"]
BT601 = [16, 1220542, 2116026, -409993, -852492, 1673527, 20, 0]


def _header(name="goalnet_storyboard.h"):
    return open(os.path.join(ROOT, "include", name)).read()


def _declared():
    text = re.sub(r"/\*.*?\*/", "", _header(), flags=re.S)
    return sorted(set(re.findall(r"\b(goalnet_[a-z0-9_]+)\s*\(", text)))


def _lib_loaded():
    if not os.path.exists(_lib.LIB_PATH):
        import __graft_entry__ as g
        g.build()
    return _lib.load()


# ---- header, binding, library ----------------------------------------------------------------------------------------------------
def test_storyboard_header_and_binding_agree():
    assert _declared() == sorted(_lib.STORYBOARD_PROTOTYPES) == NAMES
    loaded = _lib_loaded()
    lib = ctypes.CDLL(_lib.LIB_PATH)
    for name in _declared():
        assert hasattr(lib, name), f"{name} missing from libgoalnet_hip.so"
    for name, (res, args) in _lib.STORYBOARD_PROTOTYPES.items():
        fn = getattr(loaded, name)
        assert fn.restype is res and list(fn.argtypes) == args, f"{name} was not bound by _lib.load()"
    h = _header()
    assert int(re.search(r"#define GOALNET_STORYBOARD_MAX_CLIPS (\d+)", h).group(1)) == _lib.STORYBOARD_MAX_CLIPS >= 4096
    assert int(re.search(r"#define GOALNET_STORYBOARD_MAX_DIM (\d+)", h).group(1)) == _lib.STORYBOARD_MAX_DIM == 16384
    # every name the header adds carries the prefix
    body = re.sub(r"/\*.*?\*/", "", h, flags=re.S)
    for macro in re.findall(r"#define (\w+)", body):
        assert macro.startswith("GOALNET_STORYBOARD_"), macro


def test_the_ten_older_headers_and_tables_are_untouched_by_these_names():
    assert _lib.ABI_VERSION == 7 and _lib_loaded().goalnet_abi_version() == 7
    assert "#define GOALNET_ABI_VERSION 7" in _header("goalnet_hip.h")
    for table in OLDER_TABLES:
        assert set(_lib.STORYBOARD_PROTOTYPES).isdisjoint(getattr(_lib, table)), table
        assert not any(name.startswith("goalnet_storyboard_") for name in getattr(_lib, table)), table
    for other in OLDER_HEADERS:
        text = _header(other)
        for name in ("goalnet_storyboard_", "GOALNET_STORYBOARD_"):
            assert name not in text, f"{name} belongs to include/goalnet_storyboard.h, not {other}"


def test_the_build_depends_on_the_header():
    assert '"goalnet_storyboard.h"' in open(os.path.join(ROOT, "__graft_entry__.py")).read()


def test_the_package_exports_the_module():
    import cvml_goalnet_amd as pkg
    assert pkg.storyboard is storyboard and pkg.select_keyframes is select_keyframes and pkg.render_thumbnails is render_thumbnails
    assert pkg.Storyboard is storyboard.Storyboard
    assert {"storyboard", "Storyboard", "select_keyframes", "render_thumbnails"} <= set(pkg.__all__)
    assert pkg.VideoSummary.__dataclass_fields__["storyboard"].default is None


# ---- refusals of the C ABI (all before any launch) --------------------------------------------------------------------------------
def _keyframes(lib, pred=A, n_sampled=12, skip=10, full_n=120, cps=A2, flags=A3, n_clips=6, max_kf=0, fi=A4, clip=A, score=A2, capacity=6,
               count=A3):
    return lib.goalnet_storyboard_keyframes(pred, n_sampled, skip, full_n, cps, flags, n_clips, max_kf, fi, clip, score, capacity, count, None)


def _render(lib, frames=A, full_n=3, h0=4, w0=6, fi=A2, k=2, th=2, tw=3, thumbs=A3, sheet=A4, cols=2, gap=1, bg=(0, 0, 0)):
    return lib.goalnet_storyboard_render(frames, full_n, h0, w0, fi, k, th, tw, thumbs, sheet, cols, gap, *bg, None)


def _render_nv12(lib, frames=A, full_n=3, h0=4, w0=6, pitch=6, uv=24, fp=36, c=BT601, fi=A2, k=2, th=2, tw=3, thumbs=A3, sheet=A4, cols=2,
                 gap=1, bg=(0, 0, 0)):
    table = None if c is None else (ctypes.c_int32 * 8)(*c)
    return lib.goalnet_storyboard_render_nv12(frames, full_n, h0, w0, pitch, uv, fp, table, fi, k, th, tw, thumbs, sheet, cols, gap, *bg, None)


def _refused(rc, code, what):
    assert rc == code, what
    assert _lib_loaded().goalnet_last_error(), what


def test_keyframes_refusals():
    lib = _lib_loaded()
    for kw in (dict(pred=None), dict(cps=None), dict(fi=None), dict(clip=None), dict(score=None), dict(count=None)):
        _refused(_keyframes(lib, **kw), E_NULL, kw)
    for kw in (dict(n_sampled=0), dict(skip=0), dict(skip=-1), dict(full_n=0), dict(n_clips=0), dict(n_clips=-3),
               dict(n_clips=_lib.STORYBOARD_MAX_CLIPS + 1), dict(capacity=0)):
        _refused(_keyframes(lib, **kw), E_SHAPE, kw)
    # flags may be null (every clip): the call then fails on the next check, still before any launch
    _refused(_keyframes(lib, flags=None, n_clips=0), E_SHAPE, "flags=None")
    _refused(_keyframes(lib, n_clips=_lib.STORYBOARD_MAX_CLIPS, skip=0), E_SHAPE, "n_clips at the limit is not what is refused")


@pytest.mark.parametrize("call", [_render, _render_nv12])
def test_render_refusals(call):
    lib = _lib_loaded()
    for kw in (dict(frames=None), dict(fi=None), dict(thumbs=None, sheet=None)):
        _refused(call(lib, **kw), E_NULL, kw)
    for kw in (dict(k=0), dict(th=0), dict(tw=0), dict(th=-1), dict(full_n=0), dict(h0=0), dict(w0=0), dict(cols=0), dict(gap=-1),
               dict(th=_lib.STORYBOARD_MAX_DIM + 1), dict(tw=_lib.STORYBOARD_MAX_DIM + 1), dict(thumbs=None, cols=0), dict(thumbs=None, gap=-1),
               dict(k=1 << 30, th=16384, cols=1)):                      # a sheet of 2^44 rows
        _refused(call(lib, **kw), E_SHAPE, kw)
    for bg in ((256, 0, 0), (0, -1, 0), (0, 0, 1000)):
        _refused(call(lib, bg=bg), E_VALUE, bg)


def test_render_bgr_refuses_oversized_frames():
    lib = _lib_loaded()
    for kw in (dict(h0=_lib.STORYBOARD_MAX_DIM + 1), dict(w0=_lib.STORYBOARD_MAX_DIM + 1)):
        _refused(_render(lib, **kw), E_SHAPE, kw)


def test_render_nv12_layout_and_table_refusals():
    """the layout rules and the table rules of goalnet_nv12.h (tests/test_nv12_host.py has the same lists for its three calls)"""
    lib = _lib_loaded()
    for kw in (dict(h0=3), dict(w0=5), dict(h0=-2), dict(pitch=5), dict(uv=23), dict(fp=35), dict(pitch=8, uv=32, fp=32 + 8 + 5),
               dict(pitch=8, uv=31, fp=64)):
        _refused(_render_nv12(lib, **kw), E_SHAPE, kw)
    assert _render_nv12(lib, pitch=8, uv=32, fp=32 + 8 + 6, c=[16, 1, 1, 1, 1, 1, 7, 0]) == E_VALUE    # the smallest legal frame_pitch
    for shift in (7, 25, 0, -1, 32):
        _refused(_render_nv12(lib, c=[16, 256, 0, 0, 0, 0, shift, 0]), E_VALUE, shift)
    for y_off in (-1, 256):
        _refused(_render_nv12(lib, c=[y_off] + BT601[1:]), E_VALUE, y_off)
    edge = (1 << 31) - (1 << 19)
    for slot, sign in ((2, 1), (3, -1), (4, -1), (5, 1)):
        t = [0, 0, 0, 0, 0, 0, 20, 0]
        t[slot] = sign * (edge // 128)
        _refused(_render_nv12(lib, c=t), E_VALUE, t)
    _refused(_render_nv12(lib, c=[0, 8419449, 0, 0, 0, 0, 20, 0]), E_VALUE, "255 cy + 2^19 >= 2^31")
    _refused(_render_nv12(lib, c=None), E_NULL, "coeffs")
    # cols, gap and the background are not read without a sheet: the call gets past them and is refused for the table
    _refused(_render_nv12(lib, sheet=None, cols=0, gap=-1, bg=(999, 0, 0), c=[16, 256, 0, 0, 0, 0, 7, 0]), E_VALUE, "no sheet")


# ---- the oracle: the box filter ---------------------------------------------------------------------------------------------------
def test_weights_sum_to_the_source_length():
    for h0 in range(1, 41):
        for th in range(1, 41):
            w = S.weights(h0, th)
            assert w.shape == (th, h0) and (w >= 0).all()
            assert (w.sum(axis=1) == h0).all() and (w.sum(axis=0) == th).all()
            # the formula, entry by entry, in Python integers
            i, r = th - 1, h0 - 1
            assert w[i, r] == max(0, min((i + 1) * h0, (r + 1) * th) - max(i * h0, r * th))
            assert w[0, 0] == min(h0, th)


def test_box_filter_identity_constant_and_hand_worked():
    rng = np.random.default_rng(0)
    img = rng.integers(0, 256, size=(16, 24, 3), dtype=np.uint8)
    assert np.array_equal(S.box_resize(img, 16, 24), img)
    for v in (0, 1, 127, 254, 255):
        for (h0, w0, th, tw) in ((7, 11, 3, 4), (5, 7, 8, 12), (33, 1, 4, 1)):
            assert (S.box_resize(np.full((h0, w0, 3), v, dtype=np.uint8), th, tw) == v).all()
    # (0 + 1 + 2 + 4 + 2) // 4 = 2: 1.75 rounds up
    assert S.box_resize(np.array([[[0], [1]], [[2], [4]]], dtype=np.uint8), 1, 1).tolist() == [[[2]]]
    # 3 -> 2: output 0 takes 2/3 of pixel 0 and 1/3 of pixel 1 (weights 2, 1 of 3): (2 * 10 + 40 + 1) // 3 = 20
    assert S.box_resize(np.array([[[10], [40], [100]]], dtype=np.uint8), 1, 2)[0, :, 0].tolist() == [20, (40 + 200 + 1) // 3]
    # 2 -> 3 (enlarging): weights (2), (1, 1), (2) of 2
    assert S.box_resize(np.array([[[10], [41]]], dtype=np.uint8), 1, 3)[0, :, 0].tolist() == [10, (10 + 41 + 1) // 2, 41]


def test_box_filter_equals_exact_fractions():
    rng = np.random.default_rng(1)
    h0, w0, th, tw = 7, 11, 3, 4
    img = rng.integers(0, 256, size=(h0, w0, 3), dtype=np.uint8)
    got = S.box_resize(img, th, tw)

    def overlap(lo0, hi0, lo1, hi1):
        return max(Fraction(0), min(hi0, hi1) - max(lo0, lo1))

    for i in range(th):
        for j in range(tw):
            for ch in range(3):
                # the mean of the image over the output cell [i H0 / th, (i + 1) H0 / th) x [j W0 / tw, (j + 1) W0 / tw), pixels as unit squares
                total = Fraction(0)
                for r in range(h0):
                    for c in range(w0):
                        total += (overlap(Fraction(i * h0, th), Fraction((i + 1) * h0, th), r, r + 1)
                                  * overlap(Fraction(j * w0, tw), Fraction((j + 1) * w0, tw), c, c + 1) * int(img[r, c, ch]))
                mean = total / (Fraction(h0, th) * Fraction(w0, tw))
                # (n + area // 2) // area with n / area = mean: round half up, where area = 77 is odd so area // 2 = 38
                n = mean * h0 * w0
                assert n.denominator == 1
                assert got[i, j, ch] == (int(n) + (h0 * w0) // 2) // (h0 * w0)
                assert abs(Fraction(int(got[i, j, ch])) - mean) <= Fraction(1, 2)


def test_sheet_layout():
    thumbs = np.arange(5 * 2 * 3 * 3, dtype=np.uint8).reshape(5, 2, 3, 3)
    sh = S.sheet(thumbs, 3, 2, (1, 2, 3))
    assert sh.shape == (2 + 2 * 4, 2 + 3 * 5, 3) == (*sheet_shape(5, (3, 2), 3, 2), 3)
    assert np.array_equal(sh[2:4, 2:5], thumbs[0]) and np.array_equal(sh[6:8, 7:10], thumbs[4])
    assert (sh[6:8, 12:15] == (1, 2, 3)).all() and (sh[:2] == (1, 2, 3)).all() and (sh[:, 5:7] == (1, 2, 3)).all()
    covered = np.zeros(sh.shape[:2], dtype=bool)
    for k in range(5):
        covered[2 + (k // 3) * 4:4 + (k // 3) * 4, 2 + (k % 3) * 5:5 + (k % 3) * 5] = True
    assert (sh[~covered] == (1, 2, 3)).all() and covered.sum() == 5 * 6
    assert np.array_equal(S.sheet(thumbs, 1, 0, (9, 9, 9)), thumbs.reshape(10, 3, 3))


# ---- the oracle: keyframes --------------------------------------------------------------------------------------------------------
def _kf(*args, **kw):
    f, c, s = S.keyframes(*args, **kw)
    return f.tolist(), c.tolist(), s.tolist()


def test_keyframes_hand_worked():
    inf = float("inf")
    # a tie goes to the first sample; [0, 30) holds samples 0, 1, 2
    assert _kf([1, 5, 5, 2], 10, 40, [[0, 30]]) == ([10], [0], [5.0])
    # a clip between two samples, [31, 33): frame 31 + 1 = 32, score of sample 3
    assert _kf([1, 5, 5, 2], 10, 40, [[31, 33]]) == ([32], [0], [2.0])
    # ... and behind the last sample: [35, 40) with n_sampled = 3 holds frame 30's expansion, min(37 // 10, 2) = 2
    assert _kf([1, 5, 7], 10, 40, [[35, 40]]) == ([37], [0], [7.0])
    # NaN counts as -inf: it loses to anything, and wins only alone (then the first of them)
    assert _kf([np.nan, -3, np.nan], 10, 30, [[0, 30], [0, 10], [20, 30]]) == ([10, 0, 20], [0, 1, 2], [-3.0, -inf, -inf])
    assert _kf([np.nan, np.nan], 10, 20, [[0, 20]]) == ([0], [0], [-inf])
    # the end is exclusive and clamped to the video: [25, 99) of 38 frames holds sample 3 only; [38, 50) is empty; [-8, -1) = [30, 37)
    assert _kf([9, 8, 7, 6], 10, 38, [[25, 99], [38, 50], [-8, -1]]) == ([30, 30], [0, 2], [6.0, 6.0])
    # [20, 30) ends exactly where sample 3 begins
    assert _kf([1, 2, 3, 4], 10, 40, [[20, 30], [30, 40]]) == ([20, 30], [0, 1], [3.0, 4.0])
    # flags
    assert _kf([1, 2, 3, 4], 10, 40, [[0, 10], [10, 20], [20, 40]], flags=[0, 1, 1]) == ([10, 30], [1, 2], [2.0, 4.0])
    # max_keyframes with tied scores: the lower clips stay, in clip order
    cps = [[0, 10], [10, 20], [20, 30], [30, 40]]
    assert _kf([5, 7, 5, 5], 10, 40, cps, max_keyframes=2) == ([0, 10], [0, 1], [5.0, 7.0])
    assert _kf([5, 7, 5, 5], 10, 40, cps, max_keyframes=3) == ([0, 10, 20], [0, 1, 2], [5.0, 7.0, 5.0])
    assert _kf([5, 7, 5, 9], 10, 40, cps, max_keyframes=1) == ([30], [3], [9.0])
    assert _kf([5, 7, 5, 9], 10, 40, cps, max_keyframes=9) == ([0, 10, 20, 30], [0, 1, 2, 3], [5.0, 7.0, 5.0, 9.0])
    assert clip_lengths([[25, 99], [38, 50], [-8, -1], [5, 5], [7, 3]], 38).tolist() == [13, 0, 7, 0, 0]


# ---- Python-side validation (raised before the GPU is needed) ---------------------------------------------------------------------
def test_options_validation():
    o = check_options(dict(size=(8, 6), cols=2))
    assert o == dict(size=(8, 6), cols=2, gap=4, background=(0, 0, 0), max_keyframes=None, clips="selected")
    for bad in (dict(size=(0, 6)), dict(size=(8,)), dict(size=8), dict(size=(8, 1 << 15)), dict(cols=0), dict(gap=-1), dict(background=(0, 0)),
                dict(background=(0, 0, 256)), dict(background=7), dict(max_keyframes=0), dict(clips="some"), dict(colour="red"), [], "all"):
        with pytest.raises(ValueError):
            check_options(bad)


def test_python_validation_of_the_public_calls():
    pred = np.zeros(4, dtype=np.float32)
    with pytest.raises(ValueError):
        select_keyframes(pred, [[0, 10, 2]], 10, 40)
    with pytest.raises(ValueError):
        select_keyframes(pred, np.zeros((_lib.STORYBOARD_MAX_CLIPS + 1, 2)), 10, 40)
    with pytest.raises(ValueError):
        select_keyframes(pred, [[0, 10]], 0, 40)
    with pytest.raises(ValueError):
        select_keyframes(pred, [[0, 10]], 10, 0)
    with pytest.raises(ValueError):
        select_keyframes(pred, [[0, 10]], 10, 40, selected=[1])
    with pytest.raises(ValueError):
        select_keyframes(pred, [[0, 10]], 10, 40, max_keyframes=0)
    with pytest.raises(ValueError):
        select_keyframes(np.zeros((2, 2), dtype=np.float32), [[0, 10]], 10, 40)
    video = np.zeros((3, 4, 6, 3), dtype=np.uint8)
    for kw in (dict(size=(0, 2)), dict(cols=0), dict(gap=-2), dict(background=(300, 0, 0)), dict(pixel_format="i420"),
               dict(pixel_format="nv12"), dict(pixel_format="nv12", frame_size=(4, 5))):
        with pytest.raises(ValueError):
            render_thumbnails(video if kw.get("pixel_format") != "nv12" else video[..., 0], [0, 1], **kw)
    with pytest.raises(ValueError):
        render_thumbnails(video.astype(np.float32), [0])
    with pytest.raises(ValueError):
        render_thumbnails(video, [])
    with pytest.raises(ValueError):
        storyboard.storyboard(pred, [[0, 10]], 10, video, size=(2, 0))


def test_no_cpu_fallback(monkeypatch):
    """valid arguments on a machine without a GPU: GoalnetError, as everywhere else in the package"""
    monkeypatch.setattr(torch.cuda, "is_available", lambda: False)
    pred = np.zeros(4, dtype=np.float32)
    video = np.zeros((40, 4, 6, 3), dtype=np.uint8)
    with pytest.raises(GoalnetError):
        storyboard.storyboard(pred, [[0, 10], [10, 40]], 10, video, size=(3, 2), cols=2)
    with pytest.raises(GoalnetError):
        select_keyframes(pred, [[0, 10]], 10, 40)
    with pytest.raises(GoalnetError):
        render_thumbnails(video, [0, 1], size=(3, 2))


class _Model:
    head = "regression"
    audio_included = False

    def _require_device(self):
        raise AssertionError("validation must fail before the device is touched")


def test_video_summarizer_validates_the_option_before_the_device():
    vs = VideoSummarizer(_Model(), [[0, 2]], skip_frames=2)
    bgr = np.zeros((3, 4, 6, 3), dtype=np.uint8)
    for bad in (dict(size=(0, 1)), dict(cols=0), dict(clips="none"), dict(rows=2), "all", dict(max_keyframes=-1)):
        with pytest.raises(ValueError):
            vs(bgr, storyboard=bad)
    with pytest.raises(AssertionError, match="before the device"):
        vs(bgr, storyboard=dict(size=(3, 2), cols=2))                   # a valid option gets past the validation
