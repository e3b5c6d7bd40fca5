"""GPU: one fused step per cell of the mode matrix — precision {fp32, bf16, fp16} x head x audio x train / eval x {10, 32} rows, at
40 x 40 frames — against the CPU oracle under the device's decisions (tests/_mode_case.py holds the cells, the runner and every
tolerance; tests/test_mode_matrix_host.py checks on the CPU that the cells cover every three-way combination, that each cell's inputs
make its criterion reject a row mix-up, and that the comparison turns red when the oracle side is broken).

tests/test_gpu_bench_shapes.py::_run_case pins the regression head with audio in train mode; the kernels and buffer layouts that the
other switches select (voff = 0 and K0 = 512 without audio, cls_head_* / cross_entropy and its loss-scaled gradient under the 16-bit
modes, the BatchNorm-eval backward under adopted routing and gates, the classifier beyond 16 rows) meet the oracle here.

The second test runs five of the cells on four frames with H != W (_mode_case.SHAPE_CELLS) through the same runner and comparison:
every whole-model test besides runs on square frames, where an (h, w) mix-up in the host code computes the same numbers."""
import time

import pytest
import torch

pytestmark = pytest.mark.gpu

from _mode_case import (CELLS, SHAPE_CELLS, SHAPE_GEOMETRY, SHAPE_LAUNCHES, cell_id, compare, fixture_of, h16_of, is_fp32,  # noqa: E402
                        run_device)


@pytest.mark.parametrize("cell", CELLS, ids=cell_id)
def test_mode_matrix_step_vs_oracle(cell, monkeypatch):
    t0 = time.perf_counter()
    fx = fixture_of(cell)
    dev = run_device(cell, fx, monkeypatch)
    t1 = time.perf_counter()
    fig = compare(cell, fx, dev)
    print(f"[matrix] {cell_id(cell)} | logit {fig['logit']:.2e} | worst gradient {fig['grad']:.2e} ({fig['grad_name']}) | "
          f"{fig['disagree']} decisions disagree, worst {fig['worst']:.2e} of max|y| | device {t1 - t0:.2f} s, oracle {time.perf_counter() - t1:.2f} s")


def _width_fits_16bit(wc):
    """the width rule of the 16-bit pooled activations and of the fused 16-bit backward, restated from their LDS budgets (three conv rows
    of a 32-channel slice in fp32; three ring rows of wc + 2 pixels with a value and an argmax byte) and not by calling the model"""
    return 3 * wc * 32 * 4 <= 65536 and 3 * (wc + 2) * 32 * 5 <= 65536


@pytest.mark.parametrize("cell", SHAPE_CELLS, ids=cell_id)
def test_mode_matrix_step_vs_oracle_on_non_square_frames(cell, monkeypatch):
    t0 = time.perf_counter()
    fx = fixture_of(cell)
    dev = run_device(cell, fx, monkeypatch)
    t1 = time.perf_counter()
    # non-vacuity: the BatchNorm kernel of every block is the one the hand-written count next to the cell expects
    assert dev["launches"] == SHAPE_LAUNCHES[cell], "(pool_bn_fwd_small, pool_bnstats_fwd, pool_bn_eval_fwd) launches"
    n, saved = cell.n, dev["saved"]
    (h1, w1), (h2, w2), (h3, w3), (hp3, wp3) = SHAPE_GEOMETRY[cell.hw]
    assert fx["vis"].shape == (n, 3, *cell.hw) and fx["p"]["visbl.linear5.weight"].shape == (512, 512 * hp3 * wp3)
    assert [saved[k][0] for k in ("p1", "p2", "p3")] == [(n, h2, w2, 64), (n, h3, w3, 256), (n, hp3, wp3, 512)]
    if is_fp32(cell):
        assert all(saved[k][1] == torch.float32 for k in ("p1", "p2", "p3")) and not {"xh1", "xh2", "xh3"} & set(saved)
    else:
        # Block 2's pooled activation is stored in 16 bits where conv2's output width fits the rule, block 3's where conv3's does AND
        # linear5 runs on 16-bit operands (n > 16); block 1's never. EVERY block of these four shapes qualifies (the widest, 21, needs
        # 8 064 and 11 040 of the 65 536 bytes) — the rule fails first at a conv output 135 pixels wide, and a cell that wide has to
        # expect fp32 tensors from exactly the blocks whose WIDTH is over, whatever their height.
        assert all(_width_fits_16bit(w) for w in (w2, w3))
        h16 = h16_of(cell)
        assert saved["p1"][1] == torch.float32
        assert saved["p2"][1] == (h16 if _width_fits_16bit(w2) else torch.float32)
        assert saved["p3"][1] == (h16 if n > 16 and _width_fits_16bit(w3) else torch.float32)
        assert saved["xh1"][1] == h16 and saved["xh2"][1] == h16, "the padded 16-bit operands of conv2 and conv3"
        assert saved["xh3"] == ((n, hp3, wp3, 512), h16), "linear5's 16-bit operand"
    fig = compare(cell, fx, dev)
    print(f"[matrix] {cell_id(cell)} | launches {dev['launches']} | logit {fig['logit']:.2e} | worst gradient {fig['grad']:.2e} "
          f"({fig['grad_name']}) | {fig['disagree']} decisions disagree, worst {fig['worst']:.2e} of max|y| | device {t1 - t0:.2f} s, "
          f"oracle {time.perf_counter() - t1:.2f} s")
