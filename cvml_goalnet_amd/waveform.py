"""The audio front end on the GPU: what `y, sr = librosa.load(audio_fp)` (the reference's utils.py:319) does after decoding —
average the channels to mono and resample to 22 050 Hz — for samples that are already decoded, plus a reader for the file the
reference itself writes (`export_audio_from_video`, utils.py:307-311: moviepy's default, 16-bit PCM WAV). The result is the mono
float32 waveform `preprocess.extract_audio_features` takes, left on the device (csrc/wave.hip, include/goalnet_wave.h).

EXTENSION, PARITY WITH LIBROSA UNPINNED: `librosa.load` resamples with soxr_hq, which is neither installed nor restated here. The
arithmetic is DEFINED to be that of `scipy.signal.resample_poly(mono, up, down)` with its default filter (a Kaiser (beta 5)
windowed sinc, 10 * max(up, down) taps each side, zero phase, zeros outside the signal), in float64 with one rounding to float32.
That filter is gentler than soxr's: see DESIGN.md §4.19 for what leaks through it. The tap table is an argument of the C ABI.

numpy and the standard library only: scipy is the oracle of the tests, never a dependency of the package.
No CPU fallback: without the library / a GPU, `to_mono` raises.
"""
from __future__ import annotations

import math
import os
import wave

import numpy as np
import torch

from . import _lib
from ._lib import GoalnetError, check
from .ops import _s
from .preprocess import _CONST, SR


def resample_plan(sr_in: int, sr_out: int = SR, n_in=None):
    """goalnet_wave_plan in Python: (up, down, half_len, taps_per_phase, n_out); n_out is None when n_in is."""
    sr_in, sr_out = int(sr_in), int(sr_out)
    if not (1 <= sr_in <= _lib.WAVE_MAX_RATE and 1 <= sr_out <= _lib.WAVE_MAX_RATE):
        raise ValueError(f"sampling rates must lie in 1 .. {_lib.WAVE_MAX_RATE}, got {sr_in} -> {sr_out}")
    g = math.gcd(sr_in, sr_out)
    up, down = sr_out // g, sr_in // g
    if down > _lib.WAVE_MAX_RATIO * up:
        raise ValueError(f"{sr_in} -> {sr_out} Hz reduces to {up} / {down}: down > {_lib.WAVE_MAX_RATIO} * up is not supported")
    if up == 1 and down == 1:
        half_len, taps = 0, 0
    else:
        half_len = 10 * max(up, down)
        taps = -(-(2 * half_len + 1) // up)
    n_out = None
    if n_in is not None:
        n_in = int(n_in)
        if n_in < 0 or n_in * max(up, down) >= 1 << 62:
            raise ValueError(f"n_in = {n_in}: 0 <= n_in and n_in * max(up, down) < 2^62")
        n_out = -(-n_in * up // down)
    return up, down, half_len, taps, n_out


def phase_major(h: np.ndarray, up: int) -> np.ndarray:
    """(up, L) float64 from the filter h[0 .. 2 half_len]: hp[p][j] = h[p + j * up], zero-filled; L = ceil(len(h) / up)"""
    h = np.asarray(h, dtype=np.float64)
    taps = -(-h.size // up)
    flat = np.zeros(up * taps, dtype=np.float64)
    flat[:h.size] = h
    return np.ascontiguousarray(flat.reshape(taps, up).T)


def resample_filter(up: int, down: int) -> np.ndarray:
    """scipy.signal.resample_poly's default filter, `firwin(2 * half_len + 1, 1 / max(up, down), window=('kaiser', 5.0)) * up`,
    restated with numpy (tests/test_wave_host.py pins it against firwin itself)"""
    half_len = 10 * max(up, down)
    n = 2 * half_len + 1
    m = np.arange(n) - half_len
    fc = 1.0 / max(up, down)
    h = fc * np.sinc(fc * m) * np.kaiser(n, 5.0)
    h /= h.sum()
    h *= up
    return h


def resample_taps(up: int, down: int) -> np.ndarray:
    """the (up, L) float64 phase-major table goalnet_wave_resample takes for up / down (not both 1)"""
    up, down = int(up), int(down)
    if up < 1 or down < 1 or (up == 1 and down == 1):
        raise ValueError("resample_taps needs a ratio other than 1 / 1")
    return phase_major(resample_filter(up, down), up)


def _device_taps(dev, up, down):
    key = ("wave_taps", str(dev), up, down)
    if key not in _CONST:
        _CONST[key] = torch.from_numpy(resample_taps(up, down)).to(dev)
    return _CONST[key]


def to_mono(y, sr: int, target_sr: int = SR, device=None) -> torch.Tensor:
    """y: (n,) or (n, C) frames x channels (the layout of the `wave` module and of soundfile), float32 or int16 (int16 = PCM,
    value / 32768), numpy or torch, on the host or the device; `sr` its sampling rate. Returns the (ceil(n * up / down),) float32
    mono waveform at `target_sr` on the GPU. float64 is refused: nothing is rounded silently. The output length follows from
    n on the host; no synchronisation."""
    t = y if torch.is_tensor(y) else torch.from_numpy(np.ascontiguousarray(y))
    if t.dtype not in (torch.float32, torch.int16):
        raise ValueError(f"samples must be float32 or int16, got {t.dtype} (convert explicitly: nothing is rounded silently)")
    if t.dim() not in (1, 2):
        raise ValueError(f"samples must be (n,) or (n, channels), got {tuple(t.shape)}")
    n_in = int(t.shape[0])
    channels = int(t.shape[1]) if t.dim() == 2 else 1
    if n_in < 1:
        raise ValueError("no audio")
    if not 1 <= channels <= _lib.WAVE_MAX_CHANNELS:
        raise ValueError(f"{channels} channels: 1 .. {_lib.WAVE_MAX_CHANNELS} are supported (frames x channels, not channels x frames)")
    up, down, half_len, taps, n_out = resample_plan(sr, target_sr, n_in)
    if not torch.cuda.is_available():
        raise GoalnetError("the audio front end runs on the GPU (torch.cuda.is_available() is False); there is no CPU fallback")
    dev = torch.device(device if device is not None else "cuda:0")
    t = t.detach().to(dev).contiguous()
    table = None if up == down == 1 else _device_taps(dev, up, down)
    out = torch.empty(n_out, dtype=torch.float32, device=dev)
    with torch.cuda.device(dev):
        check(_lib.load().goalnet_wave_resample(t.data_ptr(), _lib.WAVE_S16 if t.dtype == torch.int16 else _lib.WAVE_F32, n_in, channels,
                                                None if table is None else table.data_ptr(), up, down, half_len, taps, out.data_ptr(),
                                                n_out, _s()), "wave_resample")
    return out


def read_wav(fp):
    """A 16-bit PCM WAV file -> ((n, C) int16 array, sampling rate), with the standard library's `wave`. Any other sample width
    is a ValueError; other containers and codecs stay the caller's decoding."""
    with wave.open(os.fspath(fp), "rb") as f:
        width, channels, sr, n = f.getsampwidth(), f.getnchannels(), f.getframerate(), f.getnframes()
        if width != 2:
            raise ValueError(f"{os.fspath(fp)}: {8 * width}-bit samples ({width} bytes wide); only 16-bit PCM is read")
        data = f.readframes(n)
    return np.frombuffer(data, dtype="<i2").astype(np.int16).reshape(-1, channels), sr


def load_audio(fp, sr: int = SR, device=None):
    """`librosa.load(fp)`'s shape of result for a 16-bit PCM WAV: (mono float32 waveform at `sr` on the GPU, sr)."""
    x, sr_in = read_wav(fp)
    return to_mono(x, sr_in, sr, device), int(sr)
