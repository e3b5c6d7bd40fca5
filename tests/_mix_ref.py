"""numpy restatement of audio augmentation and mixup on a shuffled / augmented pass (include/goalnet_mix.h), written
from the formulas and independently of cvml_goalnet_amd/augment.py and the new ops: built on synth.raw_bits / synth.stream_key (and
tests/_augment_ref.py for the frames) only. Everything is integer arithmetic or single fp32 operations, so the device results are
compared with these bit for bit.

    plan2(pl, seed, index, C, B, ...)                      -> int32 (n, 12): {a_shift, t0, tw, c0, cw, gain, partner, lambda, nkey lo, nkey hi, 0, 0}
    audio_gather(table, pl, pl2, start, count, gain, noise, mix) -> the augmented (and mixed) audio sub-batch
    frames_mix(table, pl, pl2, start, count, colour)       -> _augment_ref.gather plus the mix
    rows_mix(table, pl, pl2, start, count)                 -> labels / weights through the plan with the mix
"""
import numpy as np

import _augment_ref as R
from cvml_goalnet_amd import synth

F = np.float32
U64 = np.uint64
ONE = 0x3F800000                 # the bits of 1.0f: the lambda of an unmixed row
TID_PLAN2 = 3 << 30
GAMMA = U64(0x9E3779B97F4A7C15)
AUDIO_ON = dict(max_shift=3, time_mask=6, coeff_mask=5, gain=0.25, noise=0.5)
MIX_ON = dict(strength=0.5, p=0.5)
ALL_ON = dict(AUDIO_ON, **MIX_ON)
ALONE = {"shift": dict(max_shift=3), "time_mask": dict(time_mask=6), "coeff_mask": dict(coeff_mask=5), "gain": dict(gain=0.25),
         "noise": dict(noise=0.5), "mixup": dict(MIX_ON)}


def _mix64(z):
    z = z.astype(U64, copy=True)
    with np.errstate(over="ignore"):
        z ^= z >> U64(30)
        z *= U64(0xBF58476D1CE4E5B9)
        z ^= z >> U64(27)
        z *= U64(0x94D049BB133111EB)
        z ^= z >> U64(31)
    return z


def _bits(seed, index, k, src):
    """element r of stream k of pass `index`, for every r in src"""
    n = int(src.max()) + 1
    return synth.raw_bits(TID_PLAN2 + 16 * index + k, n, seed)[src]


def _u24(seed, index, k, src):
    return _bits(seed, index, k, src) >> U64(40)


def _unit(seed, index, k, src):
    return _u24(seed, index, k, src).astype(F) * F(2.0 ** -24)


def _f32bits(x):
    return np.asarray(x, F).view(np.int32)


def _as_f32(word):
    return np.array([word], np.int32).view(F)[0]


def plan2(pl, seed=R.SEED, index=0, C=30, B=30, max_shift=0, time_mask=0, coeff_mask=0, gain=0.0, noise=0.0, strength=0.0, p=0.0):
    """pl: the finished (n, 8) plan of the same pass; every draw is indexed by the SOURCE frame pl[i, 0]"""
    n = len(pl)
    src = pl[:, 0].astype(np.int64)
    out = np.zeros((n, 12), np.int32)
    out[:, 5] = ONE
    out[:, 6] = np.arange(n)
    out[:, 7] = ONE
    if max_shift > 0:
        out[:, 0] = ((_u24(seed, index, 0, src) * U64(2 * max_shift + 1)) >> U64(24)).astype(np.int64) - max_shift
    if time_mask > 0:
        tw = (_u24(seed, index, 1, src) * U64(time_mask + 1)) >> U64(24)
        out[:, 2] = tw
        out[:, 1] = (_u24(seed, index, 2, src) * (U64(B + 1) - tw)) >> U64(24)
    if coeff_mask > 0:
        cw = (_u24(seed, index, 3, src) * U64(coeff_mask + 1)) >> U64(24)
        out[:, 4] = cw
        out[:, 3] = 1 + ((_u24(seed, index, 4, src) * (U64(C) - cw)) >> U64(24)).astype(np.int64)
    if F(gain) > 0:
        g = F(gain)
        out[:, 5] = _f32bits(R._uniform(_unit(seed, index, 5, src), F(1) - g, F(1) + g))
    if F(noise) > 0:
        key = _bits(seed, index, 6, src)
        out[:, 8] = (key & U64(0xFFFFFFFF)).astype(np.uint32).view(np.int32)
        out[:, 9] = (key >> U64(32)).astype(np.uint32).view(np.int32)
    if F(strength) > 0 and F(p) > 0:
        q = ((_u24(seed, index, 7, src) * U64(n)) >> U64(24)).astype(np.int64)
        lam = _f32bits(R._uniform(_unit(seed, index, 8, src), F(1) - F(strength), F(1)))
        mixed = (_unit(seed, index, 9, src) < F(p)) & (q != np.arange(n)) & (lam != ONE)
        out[mixed, 6] = q[mixed]
        out[mixed, 7] = lam[mixed]
    return out


def _audio_row(table, pl, pl2, row, gain, noise):
    """steps 1-4 for plan row `row`: (C, B) fp32"""
    _, C, B = table.shape
    a_shift, t0, tw, c0, cw, gbits = (int(v) for v in pl2[row, :6])
    ts = np.arange(B, dtype=np.int64)
    v = table[int(pl[row, 0])][:, np.clip(ts - a_shift, 0, B - 1)].copy()
    if gain:
        v = (v * _as_f32(gbits)).astype(F)
    if F(noise) > 0:
        key = U64(int(pl2[row, 8]) & 0xFFFFFFFF) | (U64(int(pl2[row, 9]) & 0xFFFFFFFF) << U64(32))
        with np.errstate(over="ignore"):
            bits = _mix64(key + np.arange(1, C * B + 1, dtype=U64) * GAMMA)
        u = (bits >> U64(40)).astype(F) * F(2.0 ** -24)
        v = (v + R._uniform(u, -F(noise), F(noise)).reshape(C, B)).astype(F)
    cs = np.arange(C, dtype=np.int64)[:, None]
    masked = (cs >= 1) & (((ts >= t0) & (ts < t0 + tw))[None, :] | ((cs >= c0) & (cs < c0 + cw)))
    v.view(np.int32)[masked] = 0              # exactly +0.0
    return v


def _mix(a, b, lbits):
    """fp32 product, fp32 product, fp32 sum: no fused multiply-add across them"""
    lam = _as_f32(lbits)
    mu = F(F(1) - lam)
    return ((a * lam).astype(F) + (b * mu).astype(F)).astype(F)


def audio_gather(table, pl, pl2, start, count, gain=False, noise=0.0, mix=False):
    """table (N, C, B) fp32 -> (count, C, B); gain / noise / mix are the launch-level flags (noise: the amplitude, 0 = off)"""
    out = np.empty((count,) + table.shape[1:], F)
    for i in range(count):
        row = start + i
        v = _audio_row(table, pl, pl2, row, gain, noise)
        if mix and int(pl2[row, 7]) != ONE:
            v = _mix(v, _audio_row(table, pl, pl2, int(pl2[row, 6]), gain, noise), pl2[row, 7])
        out[i] = v
    return out


def frames_mix(table, pl, pl2, start, count, colour):
    """_augment_ref.gather with the mix: the partner is read through its own plan row — its own flip, shift and colour"""
    out = R.gather(table, pl, start, count, colour)
    for i in range(count):
        row = start + i
        if int(pl2[row, 7]) != ONE:
            out[i] = _mix(out[i], R.gather(table, pl, int(pl2[row, 6]), 1, colour)[0], pl2[row, 7])
    return out


def rows_mix(table, pl, pl2, start, count):
    """table (N, ...) fp32 -> (count, ...): rows in the plan's order, a mixed row blended with its partner's"""
    out = table[pl[start:start + count, 0]].copy()
    for i in range(count):
        row = start + i
        if int(pl2[row, 7]) != ONE:
            out[i] = _mix(out[i], table[pl[int(pl2[row, 6]), 0]], pl2[row, 7])
    return out
