"""GPU: AudBl and the whole step at every audio bin-length class, against float64 and the oracle.

The audio input is (N, 30, B); every other whole-model test runs at B = 30. B selects code (tests/_bin_classes.py restates the rules and
holds the rows, tests/test_bin_classes_host.py checks both on the CPU): whether a Conv1d layer's one-launch backward fits LDS, which
skinny kernel runs audbl.linear3, how the last window of a stride-2, pad-1 Conv1d is cut. Here every row runs:

  * both Conv1d layers chained through test_gpu_ops.audbl_conv1d_case: float64 F.conv1d with autograd, 3e-6 (forward) and 1e-5 (weight,
    bias and data gradients, d_audio among them) of the tensor's max; the one-launch backward where the library's query serves the
    layer — AVM's dispatch — equal to the multi-launch form;
  * audbl.linear3's three contractions called the way AVM calls them (output and saved multiplier into columns 0 .. 127 of 640-column
    buffers, the gradient read from such a slice), float64 at 3e-6, J = 128, K = 128 * l2;
  * six fused steps at B != 30 through the runner of the mode matrix (tests/_mode_case.py), its tolerances and decision checks;
  * one input-gradient cell at B = 60 through tests/_inputgrad_case.py;
  * the graph-captured loop at B = 60, then B = 59 through the same trainer: tables and graphs rebuilt, equal to eager bit for bit.

No tolerance is new. Every output buffer of the op-level rows starts as NaN, so an element that a class forgets fails."""
import time

import pytest
import torch

pytestmark = pytest.mark.gpu

import _bin_classes as BC  # noqa: E402
import _inputgrad_case as IC  # noqa: E402
from _mode_case import BIN_CELLS, Cell, cell_id, compare, fixture_of, run_device  # noqa: E402
from cvml_goalnet_amd import ops  # noqa: E402
from test_gpu_loop import _graph_loop_vs_eager  # noqa: E402
from test_gpu_ops import DEV, audbl_conv1d_case, close, rnd  # noqa: E402


@pytest.mark.parametrize("n,bins", BC.CONV1D_ROWS)
def test_audbl_conv1d_at_every_bin_class(n, bins):
    print(f"[bins] conv1d n = {n}, B = {bins}: l1 = {BC.l1(bins)}, l2 = {BC.l2(bins)}, one launch serves conv1: {BC.conv1_fits(n, bins)}, "
          f"conv2: {BC.conv2_fits(n, bins)}")
    launches = audbl_conv1d_case(n, bins)
    # the library's query is the rule restated in _bin_classes.py (the host test walks every (N, B); here the rows that ran)
    want = int(BC.conv1_fits(n, bins)) + int(BC.conv2_fits(n, bins))
    assert launches == (want, 2 - want), "(conv1d_bwd_small, conv1d_bwd) calls of AVM's dispatch for this row"


@pytest.mark.parametrize("m,l2", BC.LINEAR3_ROWS)
def test_linear3_contractions_at_every_k_class(m, l2):
    """audbl.linear3 as AVM.forward_device / backward_device call it: y = relu(a2 W^T + b) into cat[:, :128] with the multiplier
    (pre > 0) saved into mcat[:, :128]; dW, db from dz[:, :128] and a2; da2 = dz[:, :128] W"""
    k, j, fw = 128 * l2, 128, 640
    print(f"[bins] linear3 m = {m}, K = {k}: {BC.linear3_engine(m)}, forward KS = {BC.skinny_fwd_splits(k)} ({BC.skinny_fwd_class(k)}), "
          f"dx / dw {BC.skinny_bwd_class(k)}")
    x = rnd(m, k, seed=61, lo=0.0, hi=1.0)                 # a2 is a ReLU output
    w = rnd(j, k, seed=62, lo=-0.05, hi=0.05)
    b = rnd(j, seed=63)
    dz = rnd(m, fw, seed=64)
    xg, wg, bg = x.to(DEV), w.to(DEV), b.to(DEV)
    # ---- forward
    pre = x.double() @ w.double().t() + b.double()
    cat = torch.full((m, fw), float("nan"), device=DEV)
    mcat = torch.full((m, fw), float("nan"), device=DEV)
    ops.linear_fwd(xg, wg, bg, cat[:, :j], relu=True, mult_out=mcat[:, :j])
    close(f"linear3.fwd[{m}x{k}]", cat[:, :j], torch.relu(pre), rtol=3e-6)
    assert torch.isnan(cat[:, j:]).all() and torch.isnan(mcat[:, j:]).all(), "wrote outside columns 0 .. 127"
    safe = pre.abs() > 1e-4                                # pre-activations within fp32 noise of 0 may legitimately differ
    assert torch.equal(mcat[:, :j].cpu().double()[safe], (pre > 0).double()[safe])
    assert bool(((mcat[:, :j] == 0) | (mcat[:, :j] == 1)).all())
    # ---- weight and bias gradient
    dzg = dz.to(DEV)
    dza, dzd = dzg[:, :j], dz[:, :j].double()
    dw = torch.full((j, k), float("nan"), device=DEV)
    db = torch.full((j,), float("nan"), device=DEV)
    ops.linear_bwd_dw(dza, xg, dw, db=db)
    close(f"linear3.dw[{m}: {j}x{k}]", dw, dzd.t() @ x.double(), rtol=3e-6)
    close("linear3.db", db, dzd.sum(0), rtol=3e-6)
    # ---- data gradient
    dx = torch.full((m, k), float("nan"), device=DEV)
    ops.linear_bwd_dx(dza, wg, dx, mult=None)
    close(f"linear3.dx[{m}x{j}->{k}]", dx, dzd @ w.double(), rtol=3e-6)
    assert torch.equal(dzg.cpu(), dz), "the gradient buffer is read only"


@pytest.mark.parametrize("cell", BIN_CELLS, ids=cell_id)
def test_step_vs_oracle_at_other_bin_lengths(cell, monkeypatch):
    classes = BC.STEP_CELLS[BIN_CELLS.index(cell)][1]
    t0 = time.perf_counter()
    fx = fixture_of(cell)
    assert fx["aud"].shape == (cell.n, 30, cell.bins) and fx["p"]["audbl.linear3.weight"].shape == (128, 128 * classes["l2"])
    dev = run_device(cell, fx, monkeypatch)
    t1 = time.perf_counter()
    # non-vacuity: each Conv1d layer's backward took the form the cell is here for
    small = int(classes["conv1_fits"]) + int(classes["conv2_fits"])
    assert dev["conv1d_launches"] == (small, 2 - small), "(conv1d_bwd_small, conv1d_bwd) launches"
    fig = compare(cell, fx, dev)
    print(f"[bins] {cell_id(cell)} | conv1d launches {dev['conv1d_launches']} | logit {fig['logit']:.2e} | worst gradient {fig['grad']:.2e} "
          f"({fig['grad_name']}) | {fig['disagree']} decisions disagree, worst {fig['worst']:.2e} of max|y| | device {t1 - t0:.2f} s, "
          f"oracle {time.perf_counter() - t1:.2f} s")


def test_input_gradients_at_60_bins():
    precision, n, bins = BC.INPUTGRAD_CELL
    cell = Cell(precision, "regression", True, "train", n, (40, 40), bins)
    fx = fixture_of(cell)
    w = IC.weights_of(cell)
    dev, _ = IC.run_device(cell, fx, w)
    assert dev["d_aud"].shape == (n, 30, bins) and dev["d_vis"].shape == (n, 3, 40, 40)
    fig = IC.compare(cell, fx, dev, w)
    assert set(fig) == {"d_audio", "d_visual"}


def test_graph_loop_equals_eager_at_60_bins_and_after_a_change_to_59():
    """two videos of 23 frames in sub-batches of 10, the first at 60 bins, the second at 59 through the same trainer and model (l1 = 30
    and l2 = 15 for both, so audbl.linear3 takes either). The staging tables are (cap, 30, B): the second video rebuilds them and drops
    the graphs captured for the first, whose launches have the old table's address and B baked in. Sizes 10 and 3 run eagerly once
    (video 1), size 10 is captured in video 1 and again in video 2, size 3 in video 2: 2 eager steps, 4 replays."""
    frames, sb, bins = BC.LOOP_ROW
    tr = _graph_loop_vs_eager(True, "fp32", "regression", sb, (40, 40), (frames, frames), (2, 4), [3, 10], bins=bins)
    assert tr._key == ((40, 40), bins[1]) and tr._aud.shape[1:] == (30, bins[1])
