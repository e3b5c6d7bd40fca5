"""GPU: the conv1 and max-pool / BatchNorm kernels at every frame-width class, against float64.

The kernels of block 1 (csrc/conv1.hip) and of the three pool / BatchNorm rounds (csrc/pool_bn.hip) are compiled once per class of row
width: staging slots per thread, passes of 32 pixels per pooled and per conv row. The frames of the other tests select a few of those
classes; tests/_width_classes.py restates the dispatch rules and holds rows for all of them, on both sides of every boundary between two
classes (tests/test_width_classes_host.py checks the tables against the rules on the CPU). Here every row runs:

  * conv1 forward and weight gradient through test_gpu_ops.conv1_case: F.conv2d in float64 with autograd, 2e-6 (forward) and 2e-5 (dW,
    db) of the tensor's scale, and bit for bit against the first-generation kernels;
  * max-pool, argmax taps, BatchNorm statistics / apply and the fused backward through test_gpu_ops.pool_bn_case: float64 autograd at
    that test's tolerances, on relu(uniform) inputs whose exact zeros tie in most windows;
  * one fused step on 40 x 300 frames in fp32 and in bf16 through the runner of the mode matrix (tests/_mode_case.py), its tolerances
    and its decision checks: conv1 v3<12>, blocks 2 and 3 at four forward passes and (4, 4) / (3, 4) backward passes.

No tolerance is new. Every output buffer of the two op-level helpers starts as NaN, so an element that a class forgets fails."""
import time

import pytest
import torch

pytestmark = pytest.mark.gpu

import _width_classes as WC  # noqa: E402
from _mode_case import Cell, cell_id, compare, fixture_of, h16_of, is_fp32, run_device  # noqa: E402
from test_gpu_ops import conv1_case, pool_bn_case  # noqa: E402


@pytest.mark.parametrize("n,h,w", WC.CONV1_ROWS)
def test_conv1_fwd_and_wgrad_at_every_width_class(n, h, w, monkeypatch):
    print(f"[width] conv1 {n}x{h}x{w}: forward {WC.conv1_fwd_class(w)}, weight gradient {WC.conv1_wgrad_class(w)}, "
          f"rows per block {WC.rows_per_block(n, h, WC.CONV1_FWD_GRID)} / {WC.rows_per_block(n, h, WC.CONV1_WGRAD_GRID)}")
    conv1_case(n, h, w, monkeypatch)


@pytest.mark.parametrize("n,hc,wc,c,parts", WC.POOL_ROWS + WC.POOL_BAND_ROWS)
def test_pool_bn_forward_and_backward_at_every_width_class(n, hc, wc, c, parts):
    print(f"[width] pool {n}x{hc}x{wc}x{c}, {parts or n} partial rows: forward {WC.pool_fwd_class(wc)}, backward {WC.pool_bwd_class(wc)}, "
          f"bands {WC.row_bands(parts or n, n, hc - 2)} / {WC.row_bands(parts or n, n, hc)}")
    pool_bn_case(n, hc, wc, c, parts)


@pytest.mark.parametrize("cell", [Cell(*c) for c in WC.STEP_CELLS], ids=cell_id)
def test_step_vs_oracle_on_40x300_frames(cell, monkeypatch):
    t0 = time.perf_counter()
    fx = fixture_of(cell)
    dev = run_device(cell, fx, monkeypatch)
    t1 = time.perf_counter()
    # non-vacuity: block 1 on the one-launch kernel, blocks 2 and 3 on the width-class kernels (counts derived by hand in _width_classes)
    assert dev["launches"] == WC.STEP_LAUNCHES, "(pool_bn_fwd_small, pool_bnstats_fwd, pool_bn_eval_fwd) launches"
    n, saved = cell.n, dev["saved"]
    (h1, w1), (h2, w2), (h3, w3), (hp3, wp3) = WC.STEP_GEOMETRY
    assert fx["vis"].shape == (n, 3, *cell.hw) and fx["p"]["visbl.linear5.weight"].shape == (512, 512 * hp3 * wp3)
    assert [saved[k][0] for k in ("p1", "p2", "p3")] == [(n, h2, w2, 64), (n, h3, w3, 256), (n, hp3, wp3, 512)]
    if is_fp32(cell):
        assert all(saved[k][1] == torch.float32 for k in ("p1", "p2", "p3"))
    else:
        # conv rows of 100 pixels fit the 16-bit kernels' LDS budgets: block 2's pooled activation is 16-bit; block 3's is not at
        # n <= 16, where linear5 runs on fp32 operands (tests/test_gpu_mode_matrix.py states both rules)
        assert saved["p1"][1] == torch.float32 and saved["p2"][1] == h16_of(cell) and saved["p3"][1] == torch.float32
    fig = compare(cell, fx, dev)
    print(f"[width] {cell_id(cell)} | launches {dev['launches']} | logit {fig['logit']:.2e} | worst gradient {fig['grad']:.2e} "
          f"({fig['grad_name']}) | {fig['disagree']} decisions disagree, worst {fig['worst']:.2e} of max|y| | device {t1 - t0:.2f} s, "
          f"oracle {time.perf_counter() - t1:.2f} s")
