#!/usr/bin/env python3
"""Writes tests/golden/wave_*.npz: vectors for the audio front end (include/goalnet_wave.h), produced by running
`scipy.signal.resample_poly` and `scipy.signal.firwin` THEMSELVES. The reference holds no resampler (it calls `librosa.load`, and
librosa is not importable here), so scipy is the only oracle and parity with librosa stays unpinned.

    wave_<sr>_n<n>[_<tag>].npz   x (float32 or int16, (n,) or (n, C)), sr_in, up, down,
                                 y64 = resample_poly(mono(x) as float64, up, down)             -> 22 050 Hz
    wave_taps_<sr>.npz           h = firwin(2 * half_len + 1, 1 / max(up, down), window=('kaiser', 5.0)) * up, up, down
                                 (one file per rate, not one copy per case: 6 401 taps at 48 kHz are 51 KB);
                                 at 22 051 Hz the filter has 441 021 taps (3.5 MB), so `idx` and h[idx] are kept: every 997th
                                 tap and the 1 001 around the centre

Lengths: one multiple of the kernel's 256 outputs per block from both sides, a signal shorter than one phase row, n_in = 1.

    python tests/golden/make_golden_wave.py
"""
import math
import os

import numpy as np
from scipy.signal import firwin, resample_poly

HERE = os.path.dirname(os.path.abspath(__file__))
SR = 22050
CASES = {
    44100: [1, 2, 7, 511, 512, 513, 1537],          # 1 / 2, 41 taps: one shared phase
    48000: [1, 7, 43, 557, 558, 2000],              # 147 / 320, 44 taps; 557 -> 256 outputs, 558 -> 257
    16000: [1, 20, 185, 186, 700],                  # 441 / 320, 21 taps: upsampling; 186 -> 257 outputs
    11025: [1, 128, 129, 500],                      # 2 / 1, 21 taps
    96000: [1, 87, 1114, 1115, 3000],               # 147 / 640, 88 taps
    352800: [5, 4096, 4097, 9000],                  # 1 / 16, 321 taps: the ratio limit
    22051: [7, 300],                                # 22 050 / 22 051, 21 taps: a 3.6 MB table
}
FORMATS = {"s16c1": (np.int16, 1), "s16c2": (np.int16, 2), "f32c3": (np.float32, 3)}       # at 44 100 and 48 000 Hz, n_in = 700


def mono(x):
    x2 = x.reshape(x.shape[0], -1)
    s = x2[:, 0].astype(np.float64)
    for c in range(1, x2.shape[1]):
        s = s + x2[:, c].astype(np.float64)
    s = s / float(x2.shape[1])
    return s * 2.0 ** -15 if x.dtype == np.int16 else s


def signal(rng, n, dtype, channels):
    shape = (n,) if channels == 1 and dtype == np.float32 else (n, channels)
    if dtype == np.int16:
        return rng.integers(-32768, 32768, size=shape).astype(np.int16)
    return rng.uniform(-1.0, 1.0, size=shape).astype(np.float32)


def main():
    rng = np.random.default_rng(22050_44100)
    for sr, lengths in CASES.items():
        g = math.gcd(sr, SR)
        up, down = SR // g, sr // g
        half_len = 10 * max(up, down)
        h = firwin(2 * half_len + 1, 1.0 / max(up, down), window=("kaiser", 5.0)) * up
        if h.nbytes > 1 << 19:
            idx = np.unique(np.r_[0:h.size:997, half_len - 500:half_len + 501]).astype(np.int64)
            np.savez(os.path.join(HERE, f"wave_taps_{sr}.npz"), idx=idx, h=h[idx], up=np.array([up]), down=np.array([down]))
        else:
            np.savez(os.path.join(HERE, f"wave_taps_{sr}.npz"), h=h, up=np.array([up]), down=np.array([down]))
        cases = [(n, "", np.float32, 1) for n in lengths]
        if sr in (44100, 48000):
            cases += [(700, "_" + tag, dt, c) for tag, (dt, c) in FORMATS.items()]
        for n, tag, dt, c in cases:
            x = signal(rng, n, dt, c)
            y64 = resample_poly(mono(x), up, down)
            assert y64.dtype == np.float64 and y64.size == -(-n * up // down)
            np.savez(os.path.join(HERE, f"wave_{sr}_n{n}{tag}.npz"), x=x, sr_in=np.array([sr]), up=np.array([up]), down=np.array([down]), y64=y64)
            print(sr, f"{up}/{down}", x.shape, x.dtype, "->", y64.shape)


if __name__ == "__main__":
    main()
