"""numpy float64 restatement of include/goalnet_wave.h's definition (the audio front end), and the error bound the
tests hold the kernel to. Vectorised per tap j over all outputs k, in the header's ascending-j order; numpy has no fma, so every
step is a rounded multiply and a rounded add where the kernel has one rounded fma. tests/test_wave_host.py pins this file against
scipy.signal.resample_poly's own output (tests/golden/wave_*.npz)."""
import numpy as np

U24, U53 = 2.0 ** -24, 2.0 ** -53


def mono(x):
    """s_i = (sum of the channels in order, as doubles) / C; int16 times 2^-15 as well"""
    x = np.asarray(x)
    assert x.dtype in (np.float32, np.int16) and x.ndim in (1, 2)
    x2 = x.reshape(x.shape[0], -1)
    s = x2[:, 0].astype(np.float64)
    for c in range(1, x2.shape[1]):
        s = s + x2[:, c].astype(np.float64)
    s = s / float(x2.shape[1])
    return s * 2.0 ** -15 if x.dtype == np.int16 else s


def plan(up, down, n_in):
    """(half_len, L, n_out)"""
    if up == 1 and down == 1:
        return 0, 0, n_in
    half_len = 10 * max(up, down)
    return half_len, -(-(2 * half_len + 1) // up), -(-n_in * up // down)


def resample(s, hp, up, down):
    """float64 acc of every output (before the final rounding) from the mono float64 signal s and the (up, L) table hp"""
    s = np.asarray(s, dtype=np.float64)
    n_in = s.size
    half_len, taps, n_out = plan(up, down, n_in)
    if up == 1 and down == 1:
        return s.copy()
    assert hp.shape == (up, taps) and hp.dtype == np.float64
    t = np.arange(n_out, dtype=np.int64) * down + half_len
    p, q = t % up, t // up
    acc = np.zeros(n_out)
    for j in range(taps):
        i = q - j
        ok = (i >= 0) & (i < n_in)
        acc[ok] = acc[ok] + hp[p[ok], j] * s[i[ok]]
    return acc


def tap_mass(hp):
    """A = max over the phases of sum_j |hp[p][j]|"""
    return float(np.abs(hp).sum(axis=1).max())


def bound(ref, taps, a, smax):
    """|float32 result - ref| allowed per element: the final float32 rounding, plus `taps` rounded fma's against `taps` rounded
    multiply-adds at their worst (each step within 2^-53 of a partial sum that never exceeds A * smax). Nothing here is measured."""
    return U24 * np.abs(ref) + 2.0 * taps * U53 * a * smax


def long_signal():
    """the 64-bit-position case: 200 000 float32 samples at 22 051 Hz (k * down passes 2^31 near k = 97 390, 2^32 near 194 790)"""
    return np.random.default_rng(22051).uniform(-1.0, 1.0, 200000).astype(np.float32)
