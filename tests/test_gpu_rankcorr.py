"""GPU: rank correlation (csrc/rankcorr.hip, cvml_goalnet_amd/rankcorr.py) against the numpy restatement tests/rankcorr_ref.py and
SciPy's stored values (tests/golden/rankcorr_*.npz). EXTENSION, PARITY UNPINNED (no reference code).

The eight int64 counts must be EQUAL to the restatement's: they are exact integer sums, whatever the grid. tau, rho and their means
are compared to 1e-12 absolute, NaN in identical places: device and restatement evaluate the same two float64 formulas (two
multiplications, a square root, a division, all correctly rounded) on those equal integers, and the mean adds at most 128 values of
magnitude <= 1 in the same order; SciPy's own values differed from the restatement by at most 1.1e-16 where measured
(tests/test_rankcorr_host.py), and one miscounted pair in n0 = 2e8 would move tau by 5e-9.

Shapes: the kernel gives one i to each of 256 threads and stages 1024 j per tile, so n runs one below, at and one above 64 (the
wavefront), 256 and 1024; n = 5000 is the one case where several blocks (20) add into one count over several tiles (5)."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import rankcorr_ref as R  # noqa: E402
from _abi_guard import Bands, ptr  # noqa: E402
from cvml_goalnet_amd import AVM, RankEvaluator, _lib, rank_correlation, synth  # noqa: E402
from cvml_goalnet_amd.loop import VideoTrainer  # noqa: E402

TOL = 1e-12


def _close(name, got, want):
    got, want = np.asarray(got, dtype=np.float64), np.asarray(want, dtype=np.float64)
    assert got.shape == want.shape, f"{name}: shape {got.shape} != {want.shape}"
    assert np.array_equal(np.isnan(got), np.isnan(want)), f"{name}: NaN in other places\n{got}\n{want}"
    fin = ~np.isnan(want)
    err = float(np.max(np.abs(got[fin] - want[fin]))) if fin.any() else 0.0
    print(f"{name}: max |device - oracle| = {err:.3e}")
    assert err <= TOL, f"{name}: {err} > {TOL}"


def _same(name, res, ref):
    """a batched RankCorrelation against rankcorr_ref.rank_corr's dict"""
    assert res.counts.dtype == np.int64 and np.array_equal(res.counts, ref["counts"]), \
        f"{name}: counts differ at {np.argwhere(res.counts != ref['counts'])[:8].tolist()}\n{res.counts[res.counts != ref['counts']][:8]}"
    _close(f"{name}: tau", res.kendall_per_annotator, ref["tau"])
    _close(f"{name}: rho", res.spearman_per_annotator, ref["rho"])
    _close(f"{name}: mean tau", res.kendall, ref["mean"][:, 0])
    _close(f"{name}: mean rho", res.spearman, ref["mean"][:, 1])
    assert res.n_valid.dtype == np.int32 and np.array_equal(res.n_valid, ref["n_valid"])
    assert np.array_equal(res.nonfinite, ref["status"] != 0)


def _inputs(n, A, B, seed):
    """TVSum-like: integer scores 1..5 constant over shots of 7; predictions continuous (row 0), in steps of 0.25 (row 1), constant
    (row 2). With A = 20 annotator 4 is constant."""
    rng = np.random.default_rng(seed)
    scores = np.repeat(rng.integers(1, 6, size=(A, -(-n // 7))), 7, axis=1)[:, :n].astype(np.float32)
    if A == 20:
        scores[4] = 2.0
    pred = rng.normal(3.0, 1.0, size=(B, n)).astype(np.float32)
    if B > 1:
        pred[1] = np.round(pred[1] * 4) / 4
    if B > 2:
        pred[2] = 1.5
    return scores, pred


@pytest.mark.parametrize("frames", ["sampled", "full"])
@pytest.mark.parametrize("name", R.CASES)
def test_fixtures_match_scipy_and_the_restatement(name, frames):
    """full_n = 1003, skip = 30 ("typical", frames="full"): runs of 30 tied predictions, the last group 13 long; skip = 1; n = 3 and 5"""
    d = R.load(name)
    ev = RankEvaluator(d["scores"], d["skip"], frames)
    ref = R.evaluator(d["scores"], d["skip"], frames, d["predictions"])
    res = ev(torch.from_numpy(d["predictions"]).cuda()[:, None])                # (N, 1), as the model gives it
    assert isinstance(res.kendall, float) and isinstance(res.spearman, float) and res.nonfinite is False
    assert res.kendall_per_annotator.shape == res.spearman_per_annotator.shape == (ev.n_annotators,)
    assert res.counts.shape == (ev.n_annotators, 8) and np.array_equal(res.counts, ref["counts"][0])
    _close(f"{name} {frames}: tau vs scipy", res.kendall_per_annotator, d[f"tau_{frames}"])
    _close(f"{name} {frames}: rho vs scipy", res.spearman_per_annotator, d[f"rho_{frames}"])
    _close(f"{name} {frames}: tau vs restatement", res.kendall_per_annotator, ref["tau"][0])
    _close(f"{name} {frames}: rho vs restatement", res.spearman_per_annotator, ref["rho"][0])
    _close(f"{name} {frames}: means", [res.kendall, res.spearman], ref["mean"][0])
    valid = [int((~np.isnan(d[f"tau_{frames}"])).sum()), int((~np.isnan(d[f"rho_{frames}"])).sum())]
    assert res.n_valid.tolist() == ref["n_valid"][0].tolist() == valid
    one = ev(d["predictions"])                                                  # (N,) from the host
    assert np.array_equal(one.counts, res.counts) and one.kendall == res.kendall and one.spearman == res.spearman


@pytest.mark.parametrize("n,A,B", [(1, 1, 1), (1, 20, 3), (2, 20, 3), (63, 1, 3), (64, 20, 1), (65, 20, 3), (255, 1, 3), (256, 20, 1), (257, 3, 3),
                                   (1023, 1, 1), (1024, 2, 1), (1025, 1, 3)])
def test_shapes_around_the_wavefront_the_block_and_the_tile(n, A, B):
    scores, pred = _inputs(n, A, B, 100 + n)
    ev = RankEvaluator(scores, 1)
    ref = R.rank_corr(pred, scores)
    res = ev.batch(torch.from_numpy(pred).cuda())
    _same(f"n={n} A={A} B={B}", res, ref)
    if A == 20 and n >= 2:
        assert np.isnan(res.kendall_per_annotator[:, 4]).all() and np.isnan(res.spearman_per_annotator[:, 4]).all()      # constant annotator
        varying = sum(len(set(row.tolist())) > 1 for row in scores)             # 19 once n exceeds a shot; none of them at n = 2
        assert res.n_valid[0].tolist() == [varying, varying] and varying == (19 if n >= 63 else 0) and not res.nonfinite.any()
    if B == 3:
        assert np.isnan(res.kendall_per_annotator[2]).all() and np.isnan(res.kendall[2]) and res.n_valid[2].tolist() == [0, 0]   # constant prediction
    if n == 1:
        assert np.isnan(res.kendall_per_annotator).all() and np.isnan(res.spearman_per_annotator).all() and not res.counts.any()
    # the free function on the same vectors: tau and rho only
    tau, rho = rank_correlation(pred, torch.from_numpy(scores).cuda())
    assert tau.dtype == rho.dtype == np.float64 and tau.shape == rho.shape == (B, A)
    assert np.array_equal(tau, res.kendall_per_annotator, equal_nan=True) and np.array_equal(rho, res.spearman_per_annotator, equal_nan=True)


def test_several_blocks_and_tiles_add_into_one_count():
    n = 5000
    scores, pred = _inputs(n, 2, 1, 7)
    ref = R.rank_corr(pred, scores)
    ev = RankEvaluator(scores, 1)
    _same("n=5000", ev.batch(pred), ref)
    assert abs(int(ref["counts"][0, 0, 0])) > 1000 and int(ref["counts"][0, 0, 2]) > n, "a case with something to count"
    tau, rho = rank_correlation(pred[0], scores[1])                             # (n,) and (n,): one pair
    assert tau.shape == (1, 1) and tau[0, 0] == ev(pred[0]).kendall_per_annotator[1] and abs(rho[0, 0] - ref["rho"][0, 1]) <= TOL


def test_nonfinite_predictions_give_nan_and_leave_the_other_rows_alone():
    n, A = 300, 20
    scores, pred = _inputs(n, A, 3, 11)
    pred[2] = pred[0][::-1]
    clean = pred.copy()
    pred[1, 257] = np.nan                                                       # in the second block of i
    pred[2, 5] = np.inf
    ev = RankEvaluator(scores, 1)
    res = ev.batch(pred)
    _same("non-finite", res, R.rank_corr(pred, scores))
    assert res.nonfinite.tolist() == [False, True, True]
    assert np.isnan(res.kendall_per_annotator[1:]).all() and np.isnan(res.spearman_per_annotator[1:]).all()
    assert np.isnan(res.kendall[1:]).all() and np.isnan(res.spearman[1:]).all() and not res.n_valid[1:].any()
    assert (res.counts[1:, :, 7] == 1).all() and not res.counts[0, :, 7].any()
    ok = ev.batch(clean)
    assert not ok.nonfinite.any()
    assert np.array_equal(ok.counts[0], res.counts[0]) and ok.kendall[0] == res.kendall[0] and ok.spearman[0] == res.spearman[0]
    one = ev(pred[1])                                                           # does not raise
    assert one.nonfinite is True and np.isnan(one.kendall) and np.isnan(one.spearman)
    # a non-finite SCORE is reported the same way
    bad_scores = scores.copy()
    bad_scores[3, 10] = -np.inf
    res = RankEvaluator(bad_scores, 1)(clean[0])
    assert res.nonfinite is True and np.isnan(res.kendall_per_annotator[3]) and res.n_valid.tolist() == [18, 18] and np.isfinite(res.kendall)


def test_two_calls_give_bit_identical_buffers():
    scores, pred = _inputs(1500, 20, 3, 13)
    ev = RankEvaluator(scores, 1)
    x = torch.from_numpy(pred).cuda()
    a = ev.launch(x)
    b = ev.launch(x)
    assert a.is_cuda and a.dtype == torch.uint8 and a.data_ptr() != b.data_ptr()
    assert torch.equal(a, b)
    res = ev.unpack(a.cpu(), 3)
    again = ev.batch(x)
    assert np.array_equal(res.counts, again.counts) and np.array_equal(res.kendall_per_annotator, again.kendall_per_annotator, equal_nan=True)
    single = ev.unpack(ev.launch(x[0]).cpu(), 1)
    assert np.array_equal(single.counts[0], res.counts[0]) and single.kendall[0] == res.kendall[0]


@pytest.mark.parametrize("name,frames", [("typical", "sampled"), ("skip1", "full"), ("tiny", "full")])
def test_human_consistency_leaves_the_diagonal_out(name, frames):
    d = R.load(name)
    ev = RankEvaluator.from_annotations(d["scores"], d["skip"], frames=frames)
    h = ev.human()
    ref = R.human(d["scores"], d["skip"], frames)
    A = ev.n_annotators
    for key, matrix, per, overall, k in (("tau", h.kendall_matrix, h.kendall_per_annotator, h.kendall, 0),
                                         ("rho", h.spearman_matrix, h.spearman_per_annotator, h.spearman, 1)):
        assert matrix.shape == (A, A) and np.isnan(np.diag(matrix)).all()
        _close(f"human {name} {frames} {key}: matrix", matrix, ref[key]["matrix"])
        _close(f"human {name} {frames} {key}: per annotator", per, ref[key]["per"])
        _close(f"human {name} {frames} {key}: overall", [overall], [ref[key]["overall"]])
        assert np.array_equal(h.n_valid[:, k], ref[key]["n_valid"]) and h.n_valid.max() <= A - 1
        off = ~np.eye(A, dtype=bool)
        assert np.array_equal(matrix[off], matrix.T[off], equal_nan=True), "x against y and y against x are the same integers"
        # an annotator against itself would be exactly 1 and is NOT in the mean: every defined mean stays below 1 here
        assert np.all(per[~np.isnan(per)] < 1.0)
    if name == "typical":
        assert np.isnan(h.kendall_per_annotator[7]) and h.n_valid[7].tolist() == [0, 0] and h.n_valid[0].tolist() == [18, 18]


def test_rank_corr_guarded():
    """the raw C ABI with ldx > n, strided y and every output a view between guard bands (tests/_abi_guard.py): nothing is written
    outside the extents; a read past a row of x or y would meet the NaN bands and show up as bad > 0"""
    lib = _lib.load()
    B, A, n, ldx, stride = 2, 3, 65, 70, 3
    cols = (n - 1) * stride + 1
    ldy = cols + 5
    scores, pred = _inputs(cols, A, B, 17)
    ref = R.rank_corr(pred[:, :n], scores, 1, stride, n)
    bands = Bands()
    x = bands.place_rows(torch.from_numpy(pred[:, :n].copy()), ldx, "x")
    y = bands.place_rows(torch.from_numpy(scores), ldy, "y")
    counts = bands.guarded((B, A, 8), torch.int64, name="counts")
    tau = bands.guarded((B, A), torch.float64, name="tau")
    rho = bands.guarded((B, A), torch.float64, name="rho")
    mean = bands.guarded((B, 2), torch.float64, name="mean")
    n_valid = bands.guarded((B, 2), torch.int32, name="n_valid")
    status = bands.guarded(B, torch.int32, name="status")
    rc = lib.goalnet_rank_corr(ptr(x), ldx, 1, ptr(y), ldy, stride, B, A, n, ptr(counts), ptr(tau), ptr(rho), ptr(mean), ptr(n_valid),
                               ptr(status), torch.cuda.current_stream().cuda_stream)
    assert rc == 0, lib.goalnet_last_error()
    bands.assert_bands_intact()
    assert np.array_equal(counts.cpu().numpy(), ref["counts"])
    _close("guarded: tau", tau.cpu().numpy(), ref["tau"])
    _close("guarded: rho", rho.cpu().numpy(), ref["rho"])
    _close("guarded: mean", mean.cpu().numpy(), ref["mean"])
    assert np.array_equal(n_valid.cpu().numpy(), ref["n_valid"]) and status.cpu().tolist() == [0, 0]
    # x_repeat > 1 with a short last group: 65 = 4 * 16 + 1, ldx = 17 + 3
    xr = bands.place_rows(torch.from_numpy(pred[:, :17].copy()), 20, "x_repeat")
    ref4 = R.rank_corr(pred[:, :17], scores, 4, stride, n)
    rc = lib.goalnet_rank_corr(ptr(xr), 20, 4, ptr(y), ldy, stride, B, A, n, ptr(counts), ptr(tau), ptr(rho), ptr(mean), ptr(n_valid),
                               ptr(status), torch.cuda.current_stream().cuda_stream)
    assert rc == 0, lib.goalnet_last_error()
    bands.assert_bands_intact()
    assert np.array_equal(counts.cpu().numpy(), ref4["counts"]), "the second call starts from zero: counts is an output"
    _close("guarded, x_repeat = 4: tau", tau.cpu().numpy(), ref4["tau"])


def test_wrong_prediction_shapes_are_value_errors():
    ev = RankEvaluator(np.ones((3, 100), dtype=np.float32), 30)                 # N = 4
    for bad in (np.zeros(3), np.zeros((5, 1)), np.zeros((4, 2)), np.zeros((1, 4))):
        with pytest.raises(ValueError):
            ev(bad)
    for bad in (np.zeros(4), np.zeros((2, 5)), np.zeros((0, 4))):
        with pytest.raises(ValueError):
            ev.batch(bad)
    with pytest.raises(ValueError):
        ev.launch(np.zeros((2, 3)))


def test_eval_video_predictions_go_straight_into_the_evaluator(monkeypatch):
    """VideoTrainer.eval_video -> RankEvaluator without leaving the device: finite figures in [-1, 1] for a small default-initialised
    model (no quality level is asserted), and ONE device-to-host copy per evaluation"""
    n, h, skip = 12, 40, 15
    full_n = n * skip - 4
    model = AVM(audio_included=False, device="cuda:0", seed=synth.BASE_SEED)
    vis = torch.from_numpy(synth.make_visual(n, h, h))
    lab = torch.from_numpy(synth.make_labels(n))
    loss, pred = VideoTrainer(model).eval_video([None] * n, vis, lab)
    assert pred.is_cuda and pred.numel() == n
    rng = np.random.default_rng(3)
    scores = np.repeat(rng.integers(1, 6, size=(20, -(-full_n // 60))), 60, axis=1)[:, :full_n].astype(np.uint8)
    evs = {frames: RankEvaluator.from_annotations(scores, skip, frames=frames) for frames in ("sampled", "full")}
    torch.cuda.synchronize()
    copies = []
    real_cpu, real_to = torch.Tensor.cpu, torch.Tensor.to

    def counting_cpu(self, *a, **kw):
        if self.is_cuda:
            copies.append(tuple(self.shape))
        return real_cpu(self, *a, **kw)

    def counting_to(self, *a, **kw):
        out = real_to(self, *a, **kw)
        if self.is_cuda and not out.is_cuda:
            copies.append(tuple(self.shape))
        return out

    monkeypatch.setattr(torch.Tensor, "cpu", counting_cpu)
    monkeypatch.setattr(torch.Tensor, "to", counting_to)
    for item in ("item", "tolist", "numpy"):
        real = getattr(torch.Tensor, item)
        monkeypatch.setattr(torch.Tensor, item, lambda self, *a, _real=real, **kw: (copies.append("sync") if self.is_cuda else None, _real(self, *a, **kw))[1])
    results = {frames: ev(pred) for frames, ev in evs.items()}
    packed = evs["sampled"].launch(pred)                                        # no copy at all
    monkeypatch.undo()
    assert len(copies) == 2, f"one read-back per evaluation, got {copies}"
    assert packed.is_cuda
    p = pred.detach().float().cpu().numpy().reshape(-1)
    for frames, res in results.items():
        ref = R.evaluator(scores, skip, frames, p)
        assert np.array_equal(res.counts, ref["counts"][0])
        vals = np.concatenate([res.kendall_per_annotator, res.spearman_per_annotator, [res.kendall, res.spearman]])
        assert np.isfinite(vals).all() and np.all(np.abs(vals) <= 1.0), vals
        assert res.n_valid.tolist() == [20, 20] and res.nonfinite is False
