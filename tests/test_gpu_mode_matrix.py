"""GPU: one fused step per cell of the mode matrix — precision {fp32, bf16, fp16} x head x audio x train / eval x {10, 32} rows, at
40 x 40 frames — against the CPU oracle under the device's decisions (tests/_mode_case.py holds the cells, the runner and every
tolerance; tests/test_mode_matrix_host.py checks on the CPU that the cells cover every three-way combination, that each cell's inputs
make its criterion reject a row mix-up, and that the comparison turns red when the oracle side is broken).

tests/test_gpu_bench_shapes.py::_run_case pins the regression head with audio in train mode; the kernels and buffer layouts that the
other switches select (voff = 0 and K0 = 512 without audio, cls_head_* / cross_entropy and its loss-scaled gradient under the 16-bit
modes, the BatchNorm-eval backward under adopted routing and gates, the classifier beyond 16 rows) meet the oracle here."""
import time

import pytest
import torch

pytestmark = pytest.mark.gpu

from _mode_case import CELLS, cell_id, compare, fixture_of, run_device  # noqa: E402


@pytest.mark.parametrize("cell", CELLS, ids=cell_id)
def test_mode_matrix_step_vs_oracle(cell, monkeypatch):
    t0 = time.perf_counter()
    fx = fixture_of(cell)
    dev = run_device(cell, fx, monkeypatch)
    t1 = time.perf_counter()
    fig = compare(cell, fx, dev)
    print(f"[matrix] {cell_id(cell)} | logit {fig['logit']:.2e} | worst gradient {fig['grad']:.2e} ({fig['grad_name']}) | "
          f"{fig['disagree']} decisions disagree, worst {fig['worst']:.2e} of max|y| | device {t1 - t0:.2f} s, oracle {time.perf_counter() - t1:.2f} s")
