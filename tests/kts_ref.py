"""The oracle of csrc/kts.hip: Kernel Temporal Segmentation (Potapov et al., ECCV 2014) with the linear kernel, restated in numpy
float64 from the algorithm as DESIGN.md §4.8 fixes it. EXTENSION, PARITY UNPINNED (no reference code): the
reference holds no segmentation code, so this file is the project's own statement of the published algorithm, not a port.

Plain loops over k and l like tests/eval_ref.py; only the innermost minimum over t is a numpy call (np.argmin returns the FIRST
minimum, which is the rule "the smallest t that attains it")."""
import itertools
import math

import numpy as np

INF = float("inf")


def planted(n, d, bounds, sigma, seed=1):
    r = np.random.default_rng(seed); X = np.zeros((n, d), np.float32); e = [0] + bounds + [n]
    for a, b in zip(e[:-1], e[1:]): X[a:b] = r.standard_normal(d)
    X += sigma * r.standard_normal((n, d)).astype(np.float32)
    return X / np.linalg.norm(X, axis=1, keepdims=True)


def prefix_sums(X, normalize=True):
    """steps 1-2: S [(n+1)][d], D [n+1] in float64, summed left to right"""
    X = np.asarray(X, dtype=np.float32).astype(np.float64)
    n, d = X.shape
    if normalize:
        for i in range(n):
            nr = math.sqrt(float(np.sum(X[i] * X[i])))
            if nr > 0.0:
                X[i] = X[i] / nr
    S = np.zeros((n + 1, d))
    D = np.zeros(n + 1)
    for i in range(n):
        S[i + 1] = S[i] + X[i]
        D[i + 1] = D[i] + float(np.sum(X[i] * X[i]))
    return S, D


def scatter(S, D, i, j, lmin=1, lmax=None):
    """step 3: J(i, j) of the samples [i, j], both inclusive"""
    L = j - i + 1
    if L < lmin or (lmax is not None and L > lmax):
        return INF
    diff = S[j + 1] - S[i]
    return (D[j + 1] - D[i]) - float(np.sum(diff * diff)) / L


def total_scatter(S, D, samples, lmin=1, lmax=None):
    """the sum of J over the segments that the change points `samples` cut [0, n) into"""
    n = len(D) - 1
    e = [0] + [int(c) for c in samples] + [n]
    return sum(scatter(S, D, a, b - 1, lmin, lmax) for a, b in zip(e[:-1], e[1:]))


def penalty(m, n, vmax=1.0):
    return 0.0 if m == 0 else (vmax * m / (2.0 * n)) * (math.log(n / m) + 1.0)


def select(cost, n, vmax=1.0):
    """step 5: (objective [max_cp+1], the smallest m that minimises it among the finite ones or None)"""
    obj = np.array([c / n + penalty(m, n, vmax) if c < INF else INF for m, c in enumerate(cost)])
    best = None
    for m, o in enumerate(obj):
        if o < INF and (best is None or o < obj[best]):
            best = m
    return obj, best


def kts(X, max_cp, lmin=1, lmax=None, vmax=1.0, normalize=True):
    """steps 1-6. Returns dict(m, samples, cost, objective, feasible)."""
    S, D = prefix_sums(X, normalize)
    n = len(D) - 1
    lmax = n if lmax is None else lmax
    Jt = np.full((n + 1, n), INF)                       # Jt[l][t] = J(t, l - 1)
    for l in range(1, n + 1):
        diff = S[l][None, :] - S[:l]
        Ls = l - np.arange(l)
        row = (D[l] - D[:l]) - np.sum(diff * diff, axis=1) / Ls
        row[(Ls < lmin) | (Ls > lmax)] = INF
        Jt[l, :l] = row
    I = np.full((max_cp + 1, n + 1), INF)
    P = np.full((max_cp + 1, n + 1), -1, dtype=np.int64)
    for l in range(1, n + 1):
        I[0][l] = Jt[l][0]
    for k in range(1, max_cp + 1):
        for l in range(1, n + 1):
            lo, hi = k * lmin, l - lmin
            if lo > hi:
                continue
            c = I[k - 1][lo:hi + 1] + Jt[l][lo:hi + 1]
            a = int(np.argmin(c))
            if c[a] < INF:
                I[k][l] = c[a]
                P[k][l] = lo + a
    cost = I[:, n].copy()
    obj, m = select(cost, n, vmax)
    samples = []
    if m is not None:
        cur = n
        for k in range(m, 0, -1):
            cur = int(P[k][cur])
            samples.append(cur)
        samples.reverse()
    return dict(m=m, samples=samples, cost=cost, objective=obj, feasible=m is not None, S=S, D=D)


def to_frames(samples, skip_frames, full_n_frames):
    """step 7: [n_clips][2] int32, end inclusive, the last clip ends at full_n_frames - 1"""
    c = [0] + [int(s) for s in samples]
    ends = [s * skip_frames - 1 for s in c[1:]] + [full_n_frames - 1]
    return np.array([[a * skip_frames, b] for a, b in zip(c, ends)], dtype=np.int32)


def brute_force(X, max_cp, lmin=1, lmax=None, normalize=True):
    """every segmentation of n <= 9 samples enumerated: the optimal total scatter for every m, +inf where lmin / lmax allow none"""
    S, D = prefix_sums(X, normalize)
    n = len(D) - 1
    assert n <= 9
    lmax = n if lmax is None else lmax
    cost = np.full(max_cp + 1, INF)
    for m in range(max_cp + 1):
        for cps in itertools.combinations(range(1, n), m):
            cost[m] = min(cost[m], total_scatter(S, D, cps, lmin, lmax))
    return cost


# the cases of tests/test_gpu_kts.py: (n, d, planted boundaries, lmin, lmax (None: n), max_cp, what the restatement returns)
CASES = {
    "off_tile_n97_d37": (97, 37, [11, 30, 31, 64, 90], 1, None, 48, [11, 30, 31, 64, 90]),
    "multiples_n96_d64": (96, 64, [12, 40, 41, 70], 1, None, 20, [12, 40, 41, 70]),
    "band_n130_d640": (130, 640, [20, 45, 77, 100], 3, 40, 30, [20, 45, 77, 100]),
    "blocks_n1100_d48": (1100, 48, [100, 333, 334, 700, 1023], 1, None, 24, [100, 333, 700, 1023]),
    "tiny_n5_d8": (5, 8, [2], 1, None, 4, [2]),
    "flat_n64_d16": (64, 16, [], 1, None, 10, []),
    "single_n1_d8": (1, 8, [], 1, 1, 0, []),
}
PLANT_RECOVERED = ("off_tile_n97_d37", "multiples_n96_d64", "band_n130_d640")
SIGMA = 0.05
_cache = {}


def case(name):
    """(X float32, the restatement's result) of a case, computed once per process and shared: treat both as read-only"""
    if name not in _cache:
        n, d, bounds, lmin, lmax, max_cp, _ = CASES[name]
        X = planted(n, d, list(bounds), SIGMA)
        _cache[name] = (X, kts(X, max_cp, lmin, lmax))
    return _cache[name]
