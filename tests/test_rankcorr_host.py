"""CPU: rank correlation (csrc/rankcorr.hip, cvml_goalnet_amd/rankcorr.py) — extension, parity unpinned (no reference code).
The numpy restatement tests/rankcorr_ref.py against SciPy's stored values (tests/golden/rankcorr_*.npz, written by
tests/golden/make_golden_rankcorr.py with scipy.stats.kendalltau variant b and scipy.stats.spearmanr), and the argument contract
of goalnet_rank_corr, which returns before any launch (no GPU is needed and none is touched).

Tolerance of restatement against SciPy: 1e-12 absolute, NaN in identical places. The restatement does two float64
multiplications, one square root and one division on exact integers; on n in {2, 3, 63, 64, 65, 255, 256, 257, 1023, 1025, 1300}
with continuous, quantised, 30-fold repeated and shot-constant inputs the largest difference to SciPy 1.15.3 was 1.1e-16. 1e-12
leaves four decades for another SciPy build's summation order and still catches one miscounted pair: one pair in n0 = 2e8 moves
tau by 5e-9."""
import numpy as np
import pytest
import torch

import rankcorr_ref as R
import test_abi_contract_host as C
from cvml_goalnet_amd import _lib, rankcorr
from oracle import postproc_ref

TOL = 1e-12

# goalnet_rank_corr joins the table of tests/test_abi_contract_host.py (the pattern of tests/test_kts_host.py): one valid call with
# fake addresses and the mutations that must be refused. That file's rows became test cases when it was collected, so this row's
# mutations run below, through that file's own helpers.
# arguments: 0 x, 1 ldx, 2 x_repeat, 3 y, 4 ldy, 5 y_stride, 6 batch, 7 n_annotators, 8 n, 9 counts, 10 tau, 11 rho, 12 mean,
# 13 n_valid, 14 status, 15 stream
C.ROWS.setdefault("goalnet_rank_corr", C.auto(
    "goalnet_rank_corr", {1: 34, 2: 1, 4: 1003, 5: 30, 6: 3, 7: 20, 8: 34},
    shape=[(8, 0), (8, 65537), (7, 0), (7, 129), (6, 0), (6, 65536), (2, 0), (5, 0), (1, 33), (4, 990)],
    align=[(9, 4), (10, 4), (11, 4), (12, 4)]))
ROW = C.ROWS["goalnet_rank_corr"]


def _mutations():
    for i in ROW["null"]:
        yield "null", i, None, C.E_NULL
    for i, v in ROW["shape"]:
        yield "shape", i, v, C.E_SHAPE
    for i, v in ROW["align"]:
        yield "align", i, v, C.E_ALIGN


@pytest.mark.parametrize("kind,index,value,code", list(_mutations()), ids=lambda v: str(v))
def test_rank_corr_bad_argument_is_refused_before_any_launch(kind, index, value, code):
    args = list(ROW["args"])
    args[index] = value
    C._refused(_lib.load(), "goalnet_rank_corr", args, code, f"{kind}: argument {index} = {value}")


def test_rank_corr_row_covers_every_pointer_and_the_abi_version_stays():
    types = _lib.PROTOTYPES["goalnet_rank_corr"][1]
    assert len(ROW["args"]) == len(types) == 16
    assert set(ROW["null"]) == {i for i, t in enumerate(types[:-1]) if t is _lib.P} == {0, 3, 9, 10, 11, 12, 13, 14}, "no pointer is nullable"
    assert {i for i, _ in ROW["align"]} == {9, 10, 11, 12}, "counts, tau, rho and mean are 8-byte aligned"
    assert _lib.load().goalnet_abi_version() == _lib.ABI_VERSION == 7


def test_rank_corr_argument_errors_do_not_need_a_gpu():
    """codes and words of the messages, and the limits at their edges: the last refused value on each side"""
    lib = _lib.load()
    A = 4096
    good = dict(x=A, ldx=34, x_repeat=1, y=2 * A, ldy=1003, y_stride=30, batch=3, n_annotators=20, n=34, counts=3 * A, tau=4 * A, rho=5 * A,
                mean=6 * A, n_valid=7 * A, status=8 * A)

    def call(**kw):
        return lib.goalnet_rank_corr(*{**good, **kw}.values(), None)

    assert call(y=None) == -1 and b"null" in lib.goalnet_last_error()
    assert call(n=0) == -2 and call(n=65537, ldx=1 << 20, ldy=1 << 30) == -2 and b"65536" in lib.goalnet_last_error()
    assert call(n_annotators=129) == -2 and b"128" in lib.goalnet_last_error()
    assert call(batch=65536) == -2 and b"65535" in lib.goalnet_last_error()
    assert call(x_repeat=0) == -2 and call(y_stride=-1) == -2 and b"positive" in lib.goalnet_last_error()
    assert call(ldx=33) == -2 and b"ldx" in lib.goalnet_last_error()
    assert call(x_repeat=30, y_stride=1, n=1003, ldx=33) == -2 and b"ldx" in lib.goalnet_last_error()        # ceil(1003 / 30) = 34
    assert call(ldy=990) == -2 and b"ldy" in lib.goalnet_last_error()                                        # 33 * 30 + 1 = 991
    assert call(y_stride=1 << 30, ldy=(1 << 31) - 1) == -2 and b"ldy" in lib.goalnet_last_error()            # (n - 1) y_stride in 64 bits
    assert call(mean=6 * A + 4) == -3 and b"aligned" in lib.goalnet_last_error()
    assert call(counts=3 * A + 4) == -3 and call(tau=4 * A + 4) == -3 and call(rho=5 * A + 4) == -3


@pytest.mark.parametrize("frames", ["sampled", "full"])
@pytest.mark.parametrize("name", R.CASES)
def test_restatement_equals_scipy_on_the_fixtures(name, frames):
    d = R.load(name)
    assert d["predictions"].dtype == np.float32 and d["scores"].dtype == np.uint8
    assert d["predictions"].shape == (-(-d["full_n"] // d["skip"]),) and d["scores"].shape[1] == d["full_n"]
    r = R.evaluator(d["scores"], d["skip"], frames, d["predictions"])
    for key in ("tau", "rho"):
        got, want = r[key][0], d[f"{key}_{frames}"]
        assert np.array_equal(np.isnan(got), np.isnan(want)), f"{name} {frames} {key}: NaN in other places\n{got}\n{want}"
        fin = ~np.isnan(want)
        err = float(np.max(np.abs(got[fin] - want[fin]))) if fin.any() else 0.0
        print(f"{name} {frames} {key}: max |restatement - scipy| = {err:.3e}")
        assert err <= TOL
        assert r["n_valid"][0, ("tau", "rho").index(key)] == int(fin.sum())
    if name == "typical":
        assert np.flatnonzero(np.isnan(d[f"tau_{frames}"])).tolist() == [7], "the constant annotator, and nobody else"
        n = d["full_n"] if frames == "full" else len(d["predictions"])
        assert r["counts"][0, 7, 2] == n * (n - 1) // 2 and r["counts"][0, 7, 6] == 0               # ty = n0 and cyy = 0
    assert r["status"][0] == 0 and np.all(r["counts"][0, :, 7] == 0)


def test_counts_are_the_textbook_quantities():
    """five values by hand: x = 1 2 2 3 5, y = 1 3 3 2 2"""
    S, tx, ty, txy, cxy, cxx, cyy, bad = R.counts([1, 2, 2, 3, 5], [1, 3, 3, 2, 2])
    assert (tx, ty, txy, bad) == (1, 2, 1, 0)                      # (2, 2); (3, 3) and (2, 2); the pair of indices 1, 2
    # concordant: 0-1 0-2 0-3 0-4; discordant: 1-3 1-4 2-3 2-4; 3-4 is tied in y, 1-2 in both
    assert S == 0
    # average ranks x: 1 2.5 2.5 4 5, y: 1 4.5 4.5 2.5 2.5; d = 2 rank - 6
    dx, dy = np.array([-4, -1, -1, 2, 4]), np.array([-4, 3, 3, -1, -1])
    assert (cxy, cxx, cyy) == (int(dx @ dy), int(dx @ dx), int(dy @ dy)) and dx.sum() == dy.sum() == 0


@pytest.mark.parametrize("n", [2, 3, 64, 257])
def test_monotone_and_reversed_inputs_give_exactly_one(n):
    x = np.arange(n, dtype=np.float32) * 0.37 - 5.0
    for y, want in ((np.exp(x / 40.0), 1.0), (-x ** 3, -1.0)):
        r = R.rank_corr(x, y.astype(np.float32))
        assert r["tau"][0, 0] == want and r["rho"][0, 0] == want
        assert np.array_equal(r["mean"][0], [want, want]) and r["n_valid"][0].tolist() == [1, 1]
    # a monotone map that merges neighbours ties them in y only: tau-b stays below 1 and is not NaN
    if n >= 3:
        r = R.rank_corr(x, np.floor(np.arange(n) / 2).astype(np.float32))
        assert 0.0 < r["tau"][0, 0] < 1.0 and r["counts"][0, 0, 1] == 0 and r["counts"][0, 0, 2] == n // 2


def test_constant_nonfinite_and_single_inputs_are_nan():
    x = np.array([0.5, 1.5, -2.0, 4.0], dtype=np.float32)
    r = R.rank_corr(x, np.full(4, 3.0, dtype=np.float32))
    assert np.isnan(r["tau"][0, 0]) and np.isnan(r["rho"][0, 0]) and r["status"][0] == 0 and r["n_valid"][0].tolist() == [0, 0]
    assert np.isnan(r["mean"][0]).all() and r["counts"][0, 0].tolist()[1:4] == [0, 6, 0]
    for v in (np.nan, np.inf, -np.inf):
        xb = x.copy()
        xb[2] = v
        r = R.rank_corr(xb, np.array([1, 2, 3, 4], dtype=np.float32))
        assert np.isnan(r["tau"][0, 0]) and np.isnan(r["rho"][0, 0]) and r["status"][0] == 1 and r["counts"][0, 0, 7] == 1
    r = R.rank_corr(np.array([1.0], dtype=np.float32), np.array([2.0], dtype=np.float32))            # n = 1
    assert np.isnan(r["tau"][0, 0]) and np.isnan(r["rho"][0, 0]) and r["counts"][0, 0].tolist() == [0] * 8
    # -0.0 ties with 0.0
    assert R.counts(np.array([-0.0, 0.0, 1.0], dtype=np.float32), np.array([1, 2, 3], dtype=np.float32))[1] == 1


@pytest.mark.parametrize("full_n,skip", [(1003, 30), (600, 30), (257, 1), (5, 2), (31, 30), (60, 30)])
def test_full_frames_alignment_is_expand_array(full_n, skip):
    """frames="full": prediction j // skip for frame j is the reference's expand_array (utils.py:396-410) on the predictions; with
    N = ceil(full_n / skip) its pad branch never runs"""
    N = -(-full_n // skip)
    pred = np.arange(N, dtype=np.float32) + 0.5
    xv, yv = R.align(pred, np.arange(full_n, dtype=np.float32), skip, 1, full_n)
    assert xv.tolist() == postproc_ref.expand_array(pred.tolist(), skip, full_n)
    assert N * skip >= full_n, "expand_array truncates, it never pads"
    assert yv.tolist() == list(range(full_n))
    xs, ys = R.align(pred, np.arange(full_n, dtype=np.float32), 1, skip, N)                          # frames="sampled"
    assert xs.tolist() == pred.tolist() and ys.tolist() == list(range(0, full_n, skip))


def test_python_side_value_errors():
    from cvml_goalnet_amd import RankEvaluator, rank_correlation
    scores = np.ones((3, 10), dtype=np.float32)
    for args, kw in ((((scores, 0)), {}), ((scores, 2), dict(frames="every")), ((scores[0], 2), {}), ((np.ones((129, 10)), 2), {}),
                     ((np.ones((2, 65537)), 1), dict(frames="full")), ((np.ones((3, 0)), 2), {})):
        with pytest.raises(ValueError):
            RankEvaluator(*args, **kw)
    for x, y in ((np.ones(4), np.ones(5)), (np.ones((2, 4)), np.ones((3, 5))), (np.ones((2, 2, 2)), np.ones(2)), (np.ones(0), np.ones(0)),
                 (np.ones(4), np.ones((129, 4))), (np.ones(65537), np.ones(65537))):
        with pytest.raises(ValueError):
            rank_correlation(x, y)
    ok = rankcorr._prediction_rows
    t = torch.zeros
    assert ok(t(5), 5, False, "").shape == ok(t(5, 1), 5, False, "").shape == (1, 5)
    assert ok(t(3, 5), 5, True, "").shape == ok(t(3, 5, 1), 5, True, "").shape == (3, 5)
    for bad, batched in ((t(4), False), (t(6, 1), False), (t(5, 2), False), (t(1, 5), False), (t(3, 4), True), (t(5), True), (t(0, 5), True),
                         (t(3, 5, 2), True)):
        with pytest.raises(ValueError):
            ok(bad, 5, batched, "")


def test_packed_buffer_layout():
    """one buffer, one read-back: every float64 / int64 section starts on 8 bytes, and there is no padding that a call would
    leave unwritten"""
    for B, A in ((1, 1), (1, 20), (3, 20), (2, 3), (65535, 1)):
        assert rankcorr._packed_bytes(B, A) == 8 * (8 * B * A) + 8 * (B * A) * 2 + 8 * 2 * B + 4 * 2 * B + 4 * B
    words = torch.arange(66, dtype=torch.int64)
    host = torch.cat([words.view(torch.uint8), torch.tensor([66, 67], dtype=torch.int32).view(torch.uint8)])
    assert host.numel() == rankcorr._packed_bytes(2, 3)
    counts, tau, rho, mean, n_valid, status = rankcorr._unpack(host, 2, 3)
    assert counts.shape == (2, 3, 8) and counts.dtype == np.int64 and counts[1, 2, 7] == 47
    assert tau.shape == rho.shape == (2, 3) and mean.shape == (2, 2) and tau.dtype == np.float64
    assert tau.view(np.int64)[0, 0] == 48 and rho.view(np.int64)[0, 0] == 54 and mean.view(np.int64)[0, 0] == 60
    assert n_valid.shape == (2, 2) and n_valid.dtype == np.int32 and n_valid.tolist() == [[64, 0], [65, 0]]      # low, high halves
    assert status.dtype == np.int32 and status.tolist() == [66, 67]


def test_fails_loudly_without_a_gpu(monkeypatch):
    from cvml_goalnet_amd import GoalnetError, RankEvaluator, rank_correlation
    monkeypatch.setattr(torch.cuda, "is_available", lambda: False)
    with pytest.raises(GoalnetError):
        RankEvaluator(np.ones((3, 10), dtype=np.float32), 2)
    with pytest.raises(GoalnetError):
        RankEvaluator.from_annotations(np.ones((3, 10), dtype=np.float32), 2, frames="full")
    with pytest.raises(GoalnetError):
        rank_correlation(np.arange(4.0), np.arange(4.0))
