"""numpy restatement of the shuffled / augmented pass (include/goalnet_epoch.h), written from the formulas and
independently of cvml_goalnet_amd/augment.py: built on synth.raw_bits / synth.stream_key only. Everything is integer arithmetic or
single fp32 operations, so the device results are compared with these bit for bit.

    plan(n, seed, index, ...)            -> int32 (n, 8): {src, flip, dx, dy, gain bits, bias bits, 0, 0}
    gather(table, plan, start, count, colour) -> the augmented sub-batch
"""
import numpy as np

from cvml_goalnet_amd import synth

F = np.float32
SEED = synth.BASE_SEED
TRAINER_SEED = SEED + 1      # the trainer tests' 23-frame passes 0..3: every option fires in each (tests/test_epoch_host.py checks it)
TRAINER_FRAMES = 23
ALL_ON = dict(shuffle=True, flip_p=0.5, max_shift=3, contrast=0.25, brightness=0.125)
ALONE = {"shuffle": dict(shuffle=True), "flip": dict(flip_p=0.5), "shift": dict(max_shift=3), "contrast": dict(contrast=0.25),
         "brightness": dict(brightness=0.125)}


def _bits(seed, index, k, n):
    return synth.raw_bits(synth.TID_PLAN + 8 * index + k, n, seed)


def _u24(seed, index, k, n):
    return _bits(seed, index, k, n) >> np.uint64(40)


def _unit(seed, index, k, n):
    return _u24(seed, index, k, n).astype(F) * F(2.0 ** -24)


def order(n, seed, index):
    r = np.arange(n, dtype=np.uint64)
    key = (_bits(seed, index, 0, n) & ~np.uint64(0xFFFFFF)) | r
    assert len(np.unique(key)) == n
    return np.argsort(key, kind="stable").astype(np.int32)


def _uniform(u, lo, hi):
    """synth.uniform's two roundings: fp32 product, then fp32 sum"""
    lo = F(lo)
    span = F(F(hi) - lo)
    return (lo + (span * u).astype(F)).astype(F)


def plan(n, seed=SEED, index=0, shuffle=False, flip_p=0.0, max_shift=0, contrast=0.0, brightness=0.0):
    flip = np.zeros(n, np.int32)
    dx = np.zeros(n, np.int32)
    dy = np.zeros(n, np.int32)
    gain = np.ones(n, F)
    bias = np.zeros(n, F)
    if flip_p > 0:
        flip = (_unit(seed, index, 1, n) < F(flip_p)).astype(np.int32)
    if max_shift > 0:
        width = np.uint64(2 * max_shift + 1)
        dx = ((_u24(seed, index, 2, n) * width) >> np.uint64(24)).astype(np.int64) - max_shift
        dy = ((_u24(seed, index, 3, n) * width) >> np.uint64(24)).astype(np.int64) - max_shift
    if contrast > 0:
        c = F(contrast)
        gain = _uniform(_unit(seed, index, 4, n), F(1) - c, F(1) + c)
    if brightness > 0:
        b = F(brightness)
        bias = _uniform(_unit(seed, index, 5, n), -b, b)
    src = order(n, seed, index) if shuffle else np.arange(n, dtype=np.int32)
    out = np.zeros((n, 8), np.int32)
    out[:, 0] = src                         # every draw is indexed by the SOURCE frame
    out[:, 1] = flip[src]
    out[:, 2] = dx[src]
    out[:, 3] = dy[src]
    out[:, 4] = gain[src].view(np.int32)
    out[:, 5] = bias[src].view(np.int32)
    return out


def gather(table, pl, start, count, colour):
    """table (N, C, H, W) fp32, pl an (n, 8) plan -> (count, C, H, W)"""
    _, C, H, W = table.shape
    out = np.empty((count, C, H, W), F)
    ys, xs = np.arange(H, dtype=np.int64), np.arange(W, dtype=np.int64)
    for i in range(count):
        src, flip, dx, dy, gbits, bbits = (int(v) for v in pl[start + i, :6])
        sy = np.clip(ys - dy, 0, H - 1)
        sx = np.clip((W - 1 - xs if flip else xs) - dx, 0, W - 1)
        v = table[src][:, sy][:, :, sx]
        if colour:
            g = np.array([gbits], np.int32).view(F)[0]
            b = np.array([bbits], np.int32).view(F)[0]
            v = np.minimum(np.maximum(((v * g).astype(F) + b).astype(F), F(0)), F(1))
        out[i] = v
    return out


def colour_on(opts):
    return opts.get("contrast", 0) > 0 or opts.get("brightness", 0) > 0
