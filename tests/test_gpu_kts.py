"""GPU: temporal segmentation (csrc/kts.hip, cvml_goalnet_amd/segment.py) against the numpy float64 restatement tests/kts_ref.py.
EXTENSION, PARITY UNPINNED (no reference code): the reference holds no segmentation code, the restatement is the oracle.

Tolerance. Costs and objectives are compared to 1e-9 RELATIVE, plus a floor for values that are themselves rounding noise: a
segment of one sample has J = (D[t+1] - D[t]) - ||S[t+1] - S[t]||^2, which is 0 in exact arithmetic and a few ulps of D[n] in
float64 — in the restatement as on the device, with a different sign pattern (I[4][5] of the five-sample case and I[0][1] of the
one-sample case are such sums). The floor is worked out from the number format, not from what the kernels give: every prefix
quantity that enters a J is a left-to-right sum of at most n terms, each the result of a d-term sum, so it carries at most
(n + d) u of its magnitude <= D[n] (u = 2^-53); a J combines four of them, and device and restatement each carry that much:
floor = 8 (n + d) u D[n]. That is 1.2e-11 at n = 97, d = 37 (where 1e-9 of the optimum is 2.7e-10) and 8e-15 at n = 1, d = 8."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import kts_ref as R  # noqa: E402
from _abi_guard import Bands, ptr  # noqa: E402
from cvml_goalnet_amd import AVM, GoalnetError, TemporalSegmenter, VideoSummarizer, _lib, synth  # noqa: E402
from cvml_goalnet_amd import postprocess as pp  # noqa: E402
from cvml_goalnet_amd.preprocess import frames_to_tensor  # noqa: E402
from oracle import avm_ref  # noqa: E402

U = 2.0 ** -53
SKIP = 7                                               # full_n = 7 n - 3: not a multiple of skip_frames


def _floor(n, d, ref):
    return 8.0 * (n + d) * U * float(ref["D"][n])


def _close(name, got, want, floor):
    got, want = np.asarray(got, dtype=np.float64), np.asarray(want, dtype=np.float64)
    assert got.shape == want.shape, f"{name}: shape {got.shape} != {want.shape}"
    assert np.array_equal(np.isinf(got), np.isinf(want)) and not np.isnan(got).any(), f"{name}: +inf in other places\n{got}\n{want}"
    fin = np.isfinite(want)
    err = np.abs(got[fin] - want[fin])
    tol = 1e-9 * np.abs(want[fin]) + floor
    worst = float(np.max(err / tol)) if err.size else 0.0
    print(f"{name}: max |device - restatement| = {float(err.max()) if err.size else 0.0:.3e}, {worst:.3e} of the tolerance")
    assert np.all(err <= tol), f"{name}: {err} > {tol}"


def _segmenter(name):
    n, d, bounds, lmin, lmax, max_cp, _ = R.CASES[name]
    return TemporalSegmenter(max_change_points=max_cp, lmin=lmin, lmax=lmax)


@pytest.mark.parametrize("name", sorted(R.CASES))
def test_segmentation_matches_the_restatement(name):
    n, d, bounds, lmin, lmax, max_cp, returns = R.CASES[name]
    X, ref = R.case(name)
    full_n = SKIP * n - 3
    seg = _segmenter(name).segment(torch.from_numpy(X).cuda(), full_n, SKIP)
    floor = _floor(n, d, ref)
    # 1. the number of change points and the change points themselves
    assert seg.n_change_points == ref["m"] == len(returns)
    assert seg.samples.dtype == np.int32 and seg.samples.tolist() == ref["samples"] == returns
    # 2. the restatement's scatter of the DEVICE's change points is the restatement's optimum (the criterion that survives a tie)
    total = R.total_scatter(ref["S"], ref["D"], seg.samples.tolist(), lmin, n if lmax is None else lmax)
    _close(f"{name}: scatter of the device's change points", [total], [ref["cost"][ref["m"]]], floor)
    # 3. I[m][n] and obj(m) for every m
    assert seg.cost.shape == seg.objective.shape == (max_cp + 1,) and seg.cost.dtype == np.float64
    _close(f"{name}: cost", seg.cost, ref["cost"], floor)
    _close(f"{name}: objective", seg.objective, ref["objective"], floor / n)
    # 4. frame units: step 7, a tiling of [0, full_n - 1], and what SummaryEvaluator takes
    cps = seg.change_points
    assert cps.dtype == np.int32 and cps.shape == (seg.n_change_points + 1, 2)
    assert np.array_equal(cps, R.to_frames(ref["samples"], SKIP, full_n))
    assert cps[0, 0] == 0 and cps[-1, 1] == full_n - 1 and np.array_equal(cps[1:, 0], cps[:-1, 1] + 1) and np.all(cps[:, 1] >= cps[:, 0])
    assert np.array_equal(cps[1:, 0], seg.samples * SKIP)
    ev = pp.SummaryEvaluator(cps, full_n, SKIP)
    pred = torch.from_numpy(np.random.default_rng(n).uniform(1.0, 5.0, size=n).astype(np.float32)).cuda()
    selected, mask = ev.postprocess(pred)
    assert mask.shape == (full_n,) and set(selected) <= set(range(len(cps)))
    assert int(mask.sum()) == sum(int(cps[c, 1] - cps[c, 0] + 1) for c in selected)


def test_host_descriptors_and_unnormalised_input():
    """numpy input is uploaded; normalize=False segments the raw rows (a scaled copy of a unit-norm input: costs scale by 9)"""
    name = "off_tile_n97_d37"
    n, d, bounds, lmin, lmax, max_cp, returns = R.CASES[name]
    X, ref = R.case(name)
    full_n = SKIP * n - 3
    seg = _segmenter(name).segment(np.asarray(X), full_n, SKIP)
    assert seg.samples.tolist() == returns
    X3 = (3.0 * X).astype(np.float32)
    ref3 = R.kts(X3, max_cp, lmin, lmax, normalize=False)
    seg3 = TemporalSegmenter(max_change_points=max_cp, normalize=False).segment(torch.from_numpy(X3).cuda(), full_n, SKIP)
    _close("normalize=False: cost", seg3.cost, ref3["cost"], _floor(n, d, ref3))
    assert seg3.n_change_points == ref3["m"] and seg3.samples.tolist() == ref3["samples"]
    # a row of zeros stays zero under normalisation
    Xz = np.array(X)
    Xz[40:44] = 0.0
    refz = R.kts(Xz, max_cp, lmin, lmax)
    segz = _segmenter(name).segment(torch.from_numpy(Xz).cuda(), full_n, SKIP)
    _close("zero rows: cost", segz.cost, refz["cost"], _floor(n, d, refz))
    assert segz.samples.tolist() == refz["samples"]


def test_default_max_change_points():
    """min(n - 1, ceil(full_n_frames / 60)): this project's choice"""
    X, ref = R.case("multiples_n96_d64")
    seg = TemporalSegmenter().segment(torch.from_numpy(X).cuda(), 96 * 10, 10)
    assert seg.cost.shape == (17,)                                      # ceil(960 / 60) = 16 change points at most
    assert seg.samples.tolist() == ref["samples"]
    seg = TemporalSegmenter().segment(torch.from_numpy(X[:5].copy()).cuda(), 5 * 100, 100)
    assert seg.cost.shape == (5,)                                       # n - 1 = 4 < ceil(500 / 60)


def test_no_feasible_segmentation_raises():
    X = torch.from_numpy(R.planted(10, 4, [5], R.SIGMA)).cuda()
    with pytest.raises(GoalnetError, match="no feasible"):
        TemporalSegmenter(max_change_points=9, lmin=4, lmax=4).segment(X, 10 * SKIP - 3, SKIP)
    # lmin = lmax = 5 leaves exactly one: two segments of five
    seg = TemporalSegmenter(max_change_points=9, lmin=5, lmax=5).segment(X, 10 * SKIP - 3, SKIP)
    assert seg.samples.tolist() == [5] and np.isinf(seg.cost[[0, 2, 3, 4, 5, 6, 7, 8, 9]]).all() and np.isfinite(seg.cost[1])


@pytest.mark.parametrize("name", ["off_tile_n97_d37", "tiny_n5_d8"])
def test_kts_guarded(name):
    """the raw C ABI with every buffer between guard bands (tests/_abi_guard.py): outputs and the workspace are written inside
    their extents only; rows past the chosen m hold -1; the workspace is exactly goalnet_kts_ws_bytes long"""
    lib = _lib.load()
    n, d, bounds, lmin, lmax, max_cp, returns = R.CASES[name]
    X, ref = R.case(name)
    full_n = SKIP * n - 3
    m = ref["m"]
    bands = Bands()
    x = bands.place(torch.from_numpy(np.asarray(X)), "x")
    cps = bands.guarded((max_cp + 1, 2), torch.int32, name="change_points")
    n_clips = bands.guarded(1, torch.int32, name="n_clips")
    samples = bands.guarded(max_cp, torch.int32, name="cps_samples")
    cost = bands.guarded(max_cp + 1, torch.float64, name="cost")
    objective = bands.guarded(max_cp + 1, torch.float64, name="objective")
    status = bands.guarded(1, torch.int32, name="status")
    nbytes = lib.goalnet_kts_ws_bytes(n, d, max_cp)
    assert nbytes > 0 and nbytes % 8 == 0
    ws = bands.guarded(nbytes // 8, torch.float64, name="ws")
    rc = lib.goalnet_kts(ptr(x), n, d, 1, max_cp, lmin, n if lmax is None else lmax, 1.0, SKIP, full_n, ptr(cps), ptr(n_clips), ptr(samples),
                         ptr(cost), ptr(objective), ptr(status), ptr(ws), nbytes, torch.cuda.current_stream().cuda_stream)
    assert rc == 0, lib.goalnet_last_error()
    bands.assert_bands_intact()
    assert status.item() == 0 and n_clips.item() == m + 1
    assert samples.cpu().tolist() == returns + [-1] * (max_cp - m)
    want = np.full((max_cp + 1, 2), -1, dtype=np.int32)
    want[:m + 1] = R.to_frames(returns, SKIP, full_n)
    assert np.array_equal(cps.cpu().numpy(), want)
    floor = _floor(n, d, ref)
    _close(f"{name} guarded: cost", cost.cpu().numpy(), ref["cost"], floor)
    _close(f"{name} guarded: objective", objective.cpu().numpy(), ref["objective"], floor / n)


def _scene_video():
    """600 frames of 24 x 32 in six planted scenes of 50, 80, 170, 60, 160 and 80 frames: a pattern per scene, noise per frame"""
    rng = np.random.default_rng(31)
    bounds = [0, 50, 130, 300, 360, 520, 600]
    yy, xx = np.mgrid[0:24, 0:32]
    dark = np.zeros((24, 32))
    dark[3, 5] = 255
    light = np.full((24, 32), 255.0)
    light[20, 25] = 0
    patterns = [dark, light, (xx < 16) * 255.0, dark, ((xx // 4 + yy // 4) % 2) * 255.0, light]
    frames = np.zeros((600, 24, 32, 3), np.uint8)
    for a, b, pat in zip(bounds[:-1], bounds[1:], patterns):
        frames[a:b] = np.clip(pat[None, :, :, None] + rng.normal(0, 6, size=(b - a, 24, 32, 3)), 0, 255).astype(np.uint8)
    return frames


def test_video_summarizer_segments_the_video_itself():
    """VideoSummarizer(model, None, segmenter=...) end to end. Whether a randomly initialised model separates the scenes is NOT
    asserted (with torch's default initialisation it does not: the descriptors of all frames point the same way, KTS returns no
    change point and the knapsack cannot take a clip of the whole video). So that a summary exists at all, the bias of the layer that
    produces the descriptor is set to minus the video's mean pre-activation: two forward passes of the seeded model, no training."""
    torch.manual_seed(33)
    skip, full_n = 10, 600
    frames = torch.from_numpy(_scene_video()).cuda()
    sd = {k: torch.from_numpy(v) for k, v in synth.make_params(40, 40, audio_included=False, bn_affine="default").items()}
    sd.update(avm_ref.init_buffers())
    model = AVM(audio_included=False, device="cuda:0", seed=synth.BASE_SEED).eval()
    sd["visbl.linear5.bias"] = torch.full((512,), 64.0)                # ReLU passes everything: last_features - 64 = the pre-activation
    model.load_state_dict(sd)
    with torch.no_grad():
        model.forward_device(None, frames_to_tensor(frames, (40, 40), stride=skip), save=False)
    sd["visbl.linear5.bias"] = -(model.last_features - 64.0).mean(0).cpu()
    model.load_state_dict(sd)

    res = VideoSummarizer(model, None, skip_frames=skip, segmenter=TemporalSegmenter())(frames)
    feats = model.last_features.cpu().numpy()
    assert feats.shape == (60, 512)
    ref = R.kts(feats, 10)                                              # the default: min(59, ceil(600 / 60)) change points at most
    obj = np.sort(ref["objective"][np.isfinite(ref["objective"])])
    print(f"end to end: m = {ref['m']}, change points {ref['samples']}, model-selection margin {obj[1] - obj[0]:.3e}")
    assert res.change_points is not None and res.change_points.dtype == np.int32
    assert np.array_equal(res.change_points, R.to_frames(ref["samples"], skip, full_n))
    given = VideoSummarizer(model, res.change_points, skip_frames=skip)(frames)
    assert torch.equal(given.predictions, res.predictions)
    assert torch.equal(given.frames, res.frames) and np.array_equal(given.frame_indices, res.frame_indices) and given.selected == res.selected
    assert torch.equal(given.src_index, res.src_index) and np.array_equal(given.change_points, res.change_points)
    assert res.frames.shape[0] >= 1 and len(res.selected) >= 1
