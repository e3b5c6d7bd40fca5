"""GPU: the audio front end (include/goalnet_wave.h, csrc/wave.hip, cvml_goalnet_amd/waveform.py).

* every fixture of tests/golden/wave_*.npz (scipy.signal.resample_poly's own float64 output) through the raw C ABI, with input,
  tap table and output between guard bands (tests/_abi_guard.py): every element within wave_ref.bound — the final float32
  rounding plus the worst case of L fma's against L multiply-adds, nothing measured — the bands intact, a second call bit-equal;
* up = down = 1 copies float32 bit for bit and averages int16 stereo exactly;
* 22 051 -> 22 050 Hz over 200 000 samples: k * down passes 2^31 and 2^32 inside the signal;
* to_mono / load_audio / extract_audio_features(path, ...) / VideoSummarizer(audio_fp=..., target_sr=...) on a 3 s stereo WAV.

PARITY WITH LIBROSA UNPINNED: librosa.load resamples with soxr_hq; scipy is the oracle here."""
import glob
import os
import wave

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import wave_ref as W  # noqa: E402
from _abi_guard import Bands, bits_equal, ptr  # noqa: E402
from cvml_goalnet_amd import AVM, VideoSummarizer, _lib, load_audio, read_wav, synth, to_mono  # noqa: E402
from cvml_goalnet_amd.ops import _s  # noqa: E402
from cvml_goalnet_amd.preprocess import extract_audio_features  # noqa: E402
from cvml_goalnet_amd.waveform import phase_major, resample_taps  # noqa: E402
from oracle import audio_ref  # noqa: E402

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
FIXTURES = sorted(glob.glob(os.path.join(GOLDEN, "wave_[0-9]*.npz")))
_TABLES = {}


def table_of(sr, up, down):
    """the (up, L) table from the fixture's own firwin taps; at 22 051 Hz (3.5 MB of taps, not kept) from resample_taps, which
    tests/test_wave_host.py pins against firwin"""
    if sr not in _TABLES:
        z = np.load(os.path.join(GOLDEN, f"wave_taps_{sr}.npz"))
        _TABLES[sr] = resample_taps(up, down) if "idx" in z.files else phase_major(z["h"], up)
    return _TABLES[sr]


def raw_resample(bands, x, hp, up, down, n_out, fill=None):
    """one call through the C ABI on guarded buffers; returns the guarded output view (not synchronised)"""
    xt = torch.from_numpy(np.ascontiguousarray(x))
    n_in = xt.shape[0]
    channels = xt.shape[1] if xt.dim() == 2 else 1
    xd = bands.place(xt, name="x")
    td = bands.place(torch.from_numpy(hp), name="taps") if hp is not None else None
    half_len, taps, want_n = W.plan(up, down, n_in)
    assert want_n == n_out
    y = bands.guarded(n_out, torch.float32, fill=fill, name="y")
    rc = _lib.load().goalnet_wave_resample(ptr(xd), _lib.WAVE_S16 if xt.dtype == torch.int16 else _lib.WAVE_F32, n_in, channels, ptr(td) or None,
                                           up, down, half_len, taps, ptr(y), n_out, _s())
    assert rc == 0, _lib.load().goalnet_last_error()
    return y


@pytest.mark.parametrize("path", FIXTURES, ids=lambda p: os.path.basename(p)[5:-4])
def test_fixture_parity_through_the_c_abi(path):
    z = np.load(path, allow_pickle=False)
    sr, up, down = int(z["sr_in"][0]), int(z["up"][0]), int(z["down"][0])
    x, y64 = z["x"], z["y64"]
    hp = table_of(sr, up, down)
    bands = Bands()
    y = raw_resample(bands, x, hp, up, down, y64.size)
    bands.assert_bands_intact()
    got = y.cpu().numpy()
    assert got.dtype == np.float32 and got.shape == y64.shape
    s = W.mono(x)
    lim = W.bound(y64, hp.shape[1], W.tap_mass(hp), float(np.abs(s).max()))
    err = np.abs(got.astype(np.float64) - y64)
    print(f"[parity] {os.path.basename(path)}: max err / bound = {float((err / lim).max()):.3f}, max |err| = {float(err.max()):.3e}")
    assert np.isfinite(got).all() and (err <= lim).all(), f"{int((err > lim).sum())} of {err.size} outside the bound, first at {int(np.argmax(err > lim))}"
    again = Bands()
    y2 = raw_resample(again, x, hp, up, down, y64.size, fill=0.0)
    again.assert_bands_intact()
    assert bits_equal(y, y2)


def test_fixtures_cover_the_table():
    assert len(FIXTURES) == 39


def test_identity_is_exact():
    rng = np.random.default_rng(5)
    x = rng.standard_normal(1000).astype(np.float32)
    x[:8] = (0.0, -0.0, 1e-45, -1e-40, 3.4e38, -3.4e38, 1.0, -1.0)              # signed zeros, subnormals, the largest finite values
    bands = Bands()
    y = raw_resample(bands, x, None, 1, 1, 1000)
    bands.assert_bands_intact()
    assert bits_equal(y.cpu(), torch.from_numpy(x))
    s = rng.integers(-32768, 32768, size=(777, 2)).astype(np.int16)
    s[:3] = ((-32768, -32768), (32767, 32767), (32767, -32768))
    bands = Bands()
    y = raw_resample(bands, s, None, 1, 1, 777)
    bands.assert_bands_intact()
    want = (s[:, 0].astype(np.float64) + s[:, 1].astype(np.float64)) / 2.0 * 2.0 ** -15       # 17 significant bits: exact in float32
    assert np.array_equal(y.cpu().numpy().astype(np.float64), want)
    # the same through to_mono, (n, 1) and (n,) alike
    assert bits_equal(to_mono(x, 22050).cpu(), torch.from_numpy(x)) and bits_equal(to_mono(x[:, None], 22050).cpu(), torch.from_numpy(x))


def test_positions_beyond_32_bits():
    up, down = 22050, 22051
    x = W.long_signal()
    hp = resample_taps(up, down)
    half_len, taps, n_out = W.plan(up, down, x.size)
    assert (n_out - 1) * down + half_len > 2 ** 32 and 97390 * down > 2 ** 31 and 194790 * down > 2 ** 32
    bands = Bands()
    y = raw_resample(bands, x, hp, up, down, n_out)
    bands.assert_bands_intact()
    ref = W.resample(x.astype(np.float64), hp, up, down)
    lim = W.bound(ref, taps, W.tap_mass(hp), float(np.abs(x).max()))
    err = np.abs(y.cpu().numpy().astype(np.float64) - ref)
    print(f"[parity] long case: max err / bound = {float((err / lim).max()):.3f}")
    assert (err <= lim).all(), f"first outside the bound at k = {int(np.argmax(err > lim))}"
    assert bits_equal(y, to_mono(x, 22051))                                      # the cached device table, ordinary allocations


# ---- a sound track as the reference exports it: 16-bit stereo at 44 100 Hz -------------------------------------------------------------------
def _stereo_track(seconds=3.0, sr=44100, seed=11):
    rng = np.random.default_rng(seed)
    n = int(seconds * sr)
    t = np.arange(n) / sr
    left = 0.3 * np.sin(2 * np.pi * (200.0 + 900.0 * t) * t) + 0.05 * rng.standard_normal(n)        # a chirp over noise
    right = 0.25 * np.sin(2 * np.pi * 440.0 * t) + 0.05 * rng.standard_normal(n)
    left[n // 3: n // 3 + 8000] *= 0.001                                                            # a near-silent stretch
    return np.clip(np.round(np.stack([left, right], axis=1) * 32768.0), -32768, 32767).astype(np.int16)


@pytest.fixture(scope="module")
def track(tmp_path_factory):
    """(path, int16 (n, 2) samples, wave_ref's float64 waveform at 22 050 Hz, its bound): computed once, never modified"""
    x = _stereo_track()
    fp = tmp_path_factory.mktemp("wave") / "track.wav"
    with wave.open(str(fp), "wb") as f:
        f.setnchannels(2)
        f.setsampwidth(2)
        f.setframerate(44100)
        f.writeframes(x.astype("<i2").tobytes())
    hp = resample_taps(1, 2)
    s = W.mono(x)
    ref = W.resample(s, hp, 1, 2)
    lim = W.bound(ref, hp.shape[1], W.tap_mass(hp), float(np.abs(s).max()))
    return fp, x, ref, lim


def test_load_audio_and_to_mono(track):
    fp, x, ref, lim = track
    y, sr = load_audio(fp)
    assert sr == 22050 and y.is_cuda and y.dtype == torch.float32 and tuple(y.shape) == ((x.shape[0] + 1) // 2,) == ref.shape
    data, rate = read_wav(fp)
    assert rate == 44100 and np.array_equal(data, x)
    assert bits_equal(y, to_mono(data, rate))
    assert bits_equal(y, to_mono(torch.from_numpy(x).cuda(), 44100, 22050)) and bits_equal(y, load_audio(str(fp), 22050, "cuda:0")[0])
    assert (np.abs(y.cpu().numpy().astype(np.float64) - ref) <= lim).all()
    # float32 samples of the same values give the same waveform: the conversion of int16 is exact
    assert bits_equal(y, to_mono(x.astype(np.float32) / np.float32(32768.0), 44100))


def test_extract_audio_features_takes_the_file(track):
    fp, x, ref, _ = track
    got = extract_audio_features(fp, 3, 30)
    assert tuple(got.shape) == (3, 30, 30) and got.dtype == torch.float32 and got.is_cuda
    assert bits_equal(got, extract_audio_features(load_audio(fp)[0], 3, 30)) and bits_equal(got, extract_audio_features(str(fp), 3, 30))
    want = audio_ref.extract_audio_features(ref.astype(np.float32), 3, 30)
    err = np.abs(got.cpu().numpy().astype(np.float64) - want)
    print(f"[parity] mfcc of the resampled track: max |err| {err.max():.3e} (max |mfcc| {np.abs(want).max():.1f})")
    assert err.max() <= 2e-4 and np.abs(want).max() > 50.0
    # an array is still taken as it is, at the rate the caller names: today's behaviour
    raw = x[:, 0].astype(np.float32) / np.float32(32768.0)
    as_given = extract_audio_features(raw, 3, 30, sr=44100)
    assert np.abs(as_given.cpu().numpy() - audio_ref.extract_audio_features(raw, 3, 30, sr=44100)).max() <= 2e-4
    assert bits_equal(as_given, extract_audio_features(torch.from_numpy(raw).cuda(), 3, 30, sr=44100))
    assert not torch.equal(as_given, got)


def test_video_summarizer_takes_the_file_or_the_raw_samples(track):
    fp, x, _, _ = track
    torch.manual_seed(31)
    frames = torch.from_numpy(np.random.default_rng(32).integers(0, 256, size=(60, 8, 8, 3), dtype=np.uint8)).cuda()
    cps = np.array([[a, a + 4] for a in range(0, 60, 5)], dtype=np.int32)           # 5-frame clips: the summary holds int(0.15 * 60) = 9 frames
    model = AVM(audio_included=True, device="cuda:0", seed=synth.BASE_SEED).eval()
    vs = VideoSummarizer(model, cps, skip_frames=20)
    feats = extract_audio_features(load_audio(fp)[0], 3, 30)
    by_hand = vs(frames, audio_features=feats)
    assert tuple(by_hand.predictions.shape) == (3, 1)
    from_file = vs(frames, audio_fp=fp, bin_length=30)
    from_samples = vs(frames, waveform=x, sr=44100, target_sr=22050, bin_length=30)
    assert bits_equal(from_file.predictions, by_hand.predictions) and bits_equal(from_samples.predictions, by_hand.predictions)
    assert np.array_equal(from_file.frame_indices, by_hand.frame_indices) and torch.equal(from_file.frames, by_hand.frames)
    # target_sr=None: the waveform is taken as mono at `sr`, as before
    raw = x[:, 0].astype(np.float32) / np.float32(32768.0)
    untouched = vs(frames, waveform=raw, sr=44100, bin_length=30)
    want = vs(frames, audio_features=extract_audio_features(raw, 3, 30, sr=44100))
    assert bits_equal(untouched.predictions, want.predictions)
    with pytest.raises(ValueError, match="not both"):
        vs(frames, waveform=raw, audio_fp=fp, bin_length=30)
