#!/usr/bin/env python3
"""Generate tests/golden/rankcorr_*.npz with SciPy itself (build container only; never imported by a test).

Rank correlation of predicted importances with annotator scores (cvml_goalnet_amd/rankcorr.py, csrc/rankcorr.hip) is an
EXTENSION, PARITY UNPINNED (no reference code): the oracle is `scipy.stats.kendalltau(x, y, variant="b")` and
`scipy.stats.spearmanr(x, y)`, called here on seeded inputs once per annotator and per way of aligning predictions with
annotations, and stored:

  predictions   float32 (N,), N = ceil(full_n / skip)
  scores        uint8 (A, full_n): TVSum-like integers 1..5, piecewise constant over shots
  skip, full_n
  tau_sampled / rho_sampled   float64 (A,): predictions[i] against scores[a, i skip]              (the frames get_annotations labels)
  tau_full / rho_full         float64 (A,): predictions[j // skip] against scores[a, j], every j   (expand_array, utils.py:396-410)

NaN is what SciPy returns for a constant input (it warns; the warning is silenced here).

Usage: python tests/golden/make_golden_rankcorr.py [case ...]
"""
from __future__ import annotations

import os
import sys
import warnings

import numpy as np
import scipy
import scipy.stats

HERE = os.path.dirname(os.path.abspath(__file__))

# shot: frames over which an annotator's score is constant (60 = 2 seconds at 30 frames per second); flat: an annotator who gives
# every frame a 3; step: predictions rounded to multiples of it
CASES = {
    "typical": dict(seed=41, full_n=1003, skip=30, n_users=20, shot=60, flat=7, step=None),
    "ties": dict(seed=42, full_n=600, skip=30, n_users=20, shot=60, flat=None, step=0.25),
    "skip1": dict(seed=43, full_n=257, skip=1, n_users=20, shot=60, flat=None, step=None),
    "tiny": dict(seed=44, full_n=5, skip=2, n_users=3, shot=2, flat=None, step=None),
}


def make_case(seed, full_n, skip, n_users, shot, flat, step):
    rng = np.random.default_rng(seed)
    n_shots = (full_n + shot - 1) // shot
    scores = np.repeat(rng.integers(1, 6, size=(n_users, n_shots)), shot, axis=1)[:, :full_n].astype(np.uint8)
    if flat is not None:
        scores[flat, :] = 3
    n = (full_n + skip - 1) // skip
    # importances that follow the annotators' mean loosely, so that the correlations are neither 0 nor 1
    pred = scores[:, ::skip].mean(axis=0) + rng.normal(0.0, 0.8, size=n)
    if step is not None:
        pred = np.round(pred / step) * step
    return scores, pred.astype(np.float32)


def scipy_pair(x, y):
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        tau = scipy.stats.kendalltau(x, y, variant="b").statistic
        rho = scipy.stats.spearmanr(x, y).statistic
    return float(tau), float(rho)


def main():
    names = sys.argv[1:] or list(CASES)
    for name in names:
        c = CASES[name]
        scores, pred = make_case(**c)
        skip, full_n = c["skip"], c["full_n"]
        out = {k: np.zeros(scores.shape[0]) for k in ("tau_sampled", "rho_sampled", "tau_full", "rho_full")}
        expanded = pred[np.arange(full_n) // skip]
        for a, row in enumerate(scores.astype(np.float32)):
            out["tau_sampled"][a], out["rho_sampled"][a] = scipy_pair(pred, row[::skip])
            out["tau_full"][a], out["rho_full"][a] = scipy_pair(expanded, row)
        path = os.path.join(HERE, f"rankcorr_{name}.npz")
        np.savez_compressed(path, predictions=pred, scores=scores, skip=np.array([skip]), full_n=np.array([full_n]), **out)
        print(f"rankcorr_{name}: scipy {scipy.__version__}, annotators={scores.shape[0]} n_sampled={pred.shape[0]} "
              f"tau_sampled[:4]={np.round(out['tau_sampled'][:4], 4).tolist()} NaN annotators "
              f"{np.flatnonzero(np.isnan(out['tau_full'])).tolist()} size {os.path.getsize(path)} B")


if __name__ == "__main__":
    main()
