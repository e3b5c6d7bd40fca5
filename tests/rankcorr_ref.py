"""numpy restatement of the rank-correlation kernels (csrc/rankcorr.hip) — extension, parity unpinned (no
reference code). The oracle for tau and rho themselves is SciPy, through the fixtures tests/golden/rankcorr_*.npz; this file
restates the definitions so that the eight int64 counts, which SciPy does not expose, have an oracle too: the O(n^2) comparison
matrices, exact integer sums, and the two float64 formulas. Imported by tests only; never imports SciPy.

    x_b[i] = x[b][i // x_repeat]        y_a[i] = y[a][i * y_stride]        i = 0 .. n-1
"""
import os

import numpy as np

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
COUNT_NAMES = ("S", "tx", "ty", "txy", "cxy", "cxx", "cyy", "bad")
CASES = ("typical", "ties", "skip1", "tiny")


def align(x_row, y_row, x_repeat, y_stride, n):
    """the element rule: the two float32 vectors of length n that are compared"""
    i = np.arange(n)
    return np.asarray(x_row, dtype=np.float32)[i // x_repeat], np.asarray(y_row, dtype=np.float32)[i * y_stride]


def _half(v):
    v = int(v)
    assert v % 2 == 0, "the full square holds every unordered pair twice"
    return v // 2


def counts(xv, yv):
    """the eight counts of two float32 vectors, python ints. IEEE < and == only: -0.0 ties with 0.0, a NaN is less than, greater
    than and equal to nothing (itself included)."""
    xv, yv = np.asarray(xv, dtype=np.float32), np.asarray(yv, dtype=np.float32)
    n = xv.shape[0]
    assert xv.shape == yv.shape == (n,)
    with np.errstate(invalid="ignore"):
        ltx, gtx, eqx = xv[None, :] < xv[:, None], xv[:, None] < xv[None, :], xv[None, :] == xv[:, None]     # [i][j]: x_j < x_i, ...
        lty, gty, eqy = yv[None, :] < yv[:, None], yv[:, None] < yv[None, :], yv[None, :] == yv[:, None]
    sx = ltx.astype(np.int8) - gtx.astype(np.int8)                 # the sign matrices: -1, 0, 1
    sy = lty.astype(np.int8) - gty.astype(np.int8)
    off = ~np.eye(n, dtype=bool)
    S = _half((sx * sy).sum(dtype=np.int64))
    tx = _half((eqx & off).sum())
    ty = _half((eqy & off).sum())
    txy = _half((eqx & eqy & off).sum())
    dx = 2 * ltx.sum(axis=1).astype(np.int64) + eqx.sum(axis=1).astype(np.int64) - n      # twice the average rank minus (n + 1)
    dy = 2 * lty.sum(axis=1).astype(np.int64) + eqy.sum(axis=1).astype(np.int64) - n
    cxy, cxx, cyy = int((dx * dy).sum()), int((dx * dx).sum()), int((dy * dy).sum())
    bad = int((~(np.isfinite(xv) & np.isfinite(yv))).sum())
    return [S, tx, ty, txy, cxy, cxx, cyy, bad]


def tau_rho(c, n):
    """the two formulas on exact integers, in float64"""
    S, tx, ty, txy, cxy, cxx, cyy, bad = (int(v) for v in c)
    n0 = n * (n - 1) // 2
    tau = rho = float("nan")
    if n >= 2 and n0 != tx and n0 != ty and bad == 0:
        tau = float(S) / float(np.sqrt(np.float64(n0 - tx) * np.float64(n0 - ty)))
    if cxx != 0 and cyy != 0 and bad == 0:
        rho = float(cxy) / float(np.sqrt(np.float64(cxx) * np.float64(cyy)))
    return tau, rho


def _mean_defined(v):
    s, c = 0.0, 0
    for t in v:                                                    # annotator order
        if t == t:
            s += float(t)
            c += 1
    return (s / c if c else float("nan")), c


def rank_corr(x, y, x_repeat=1, y_stride=1, n=None):
    """every (b, a) pair, as goalnet_rank_corr: dict of counts (B, A, 8) int64, tau / rho (B, A), mean (B, 2), n_valid (B, 2) int32,
    status (B,) int32"""
    x, y = np.atleast_2d(np.asarray(x, dtype=np.float32)), np.atleast_2d(np.asarray(y, dtype=np.float32))
    B, A = x.shape[0], y.shape[0]
    if n is None:
        n = x.shape[1] * x_repeat
    out = dict(counts=np.zeros((B, A, 8), dtype=np.int64), tau=np.zeros((B, A)), rho=np.zeros((B, A)), mean=np.zeros((B, 2)),
               n_valid=np.zeros((B, 2), dtype=np.int32), status=np.zeros(B, dtype=np.int32))
    for b in range(B):
        for a in range(A):
            xv, yv = align(x[b], y[a], x_repeat, y_stride, n)
            c = counts(xv, yv)
            out["counts"][b, a] = c
            out["tau"][b, a], out["rho"][b, a] = tau_rho(c, n)
        for k, name in enumerate(("tau", "rho")):
            out["mean"][b, k], out["n_valid"][b, k] = _mean_defined(out[name][b])
        out["status"][b] = int(out["counts"][b, :, 7].sum() > 0)
    return out


def evaluator(scores, skip, frames, predictions):
    """what RankEvaluator(scores, skip, frames).batch(predictions) computes; predictions (B, N) or (N,)"""
    scores = np.asarray(scores, dtype=np.float32)
    full_n = scores.shape[1]
    if frames == "sampled":
        return rank_corr(predictions, scores, 1, skip, -(-full_n // skip))
    return rank_corr(predictions, scores, skip, 1, full_n)


def human(scores, skip, frames):
    """RankEvaluator.human(): the annotators against each other, diagonal left out"""
    scores = np.asarray(scores, dtype=np.float32)
    A, full_n = scores.shape
    if frames == "sampled":
        r = rank_corr(np.ascontiguousarray(scores[:, ::skip]), scores, 1, skip, -(-full_n // skip))
    else:
        r = rank_corr(scores, scores, 1, 1, full_n)
    out = {}
    for name in ("tau", "rho"):
        m = r[name].copy()
        np.fill_diagonal(m, np.nan)
        per, cnt = zip(*[_mean_defined(m[a]) for a in range(A)])
        out[name] = dict(matrix=m, per=np.array(per), n_valid=np.array(cnt, dtype=np.int32), overall=_mean_defined(per)[0])
    return out


def load(name):
    """a fixture of tests/golden/make_golden_rankcorr.py: predictions float32 (N,), scores uint8 (A, full_n), skip, full_n and
    SciPy's tau / rho per annotator for both `frames` modes"""
    z = np.load(os.path.join(GOLDEN, f"rankcorr_{name}.npz"))
    d = {k: z[k] for k in z.files}
    d["skip"], d["full_n"] = int(d["skip"][0]), int(d["full_n"][0])
    return d
