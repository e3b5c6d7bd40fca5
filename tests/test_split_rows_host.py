"""CPU: per-row accuracy of the split-operand arithmetic over mixed magnitudes (tests/_split_emul.py): what "fp32-grade" means for
"bf16x6" and "fp16x3" when one tensor holds rows of very different size. No kernel runs here: this is the arithmetic of the ideal
split product alone, and it pins the dynamic-range limit that README.md, DESIGN.md §3 / §4.2.1 and csrc/split3.hip state."""
import pytest
import torch

from _split_emul import FP16X3_KNEE, ROW_EXPONENTS, ROW_TOL, ideal_split_product, per_row_error, rows_at_exponents


def _case(rows_per_r=3, k=2304, cols=64):
    g = torch.Generator().manual_seed(500)
    a = (torch.rand(rows_per_r * len(ROW_EXPONENTS), k, generator=g, dtype=torch.float64) * 2 - 1).float()
    b = ((torch.rand(cols, k, generator=g, dtype=torch.float64) * 2 - 1) * 0.05).float()
    a, r = rows_at_exponents(a, 0)
    return a, b, r


def _worst_by_r(err, r):
    return {rv: err[r == rv].max().item() for rv in ROW_EXPONENTS}


def test_bf16x6_keeps_every_row_at_fp32_grade_whatever_its_magnitude():
    """bf16 triples are the fp32 value exactly and bf16 has fp32's exponent range: a row 2^40 below the tensor's maximum is as
    accurate, relative to ITSELF, as the largest one (the six products miss a b by < 2^-23 |a b|)."""
    a, b, r = _case()
    ref = a.double() @ b.double().t()
    err = _worst_by_r(per_row_error(ideal_split_product(lambda x, y: x @ y.t(), a, b, 3), ref), r)
    print("[parity] ideal bf16x6 product, per-row error by r:", {k: f"{v:.2e}" for k, v in err.items()})
    assert all(v <= ROW_TOL for v in err.values()), err


def test_fp16x3_per_row_accuracy_ends_2_to_the_20_below_the_tensor_maximum():
    """ONE power-of-two scale per tensor puts the maximum into [2^14, 2^15). A row at 2^-r of it has its `mid` part in binary16's
    subnormals from r = 18 (absolute quantum 2^-24 of the scaled value): relative error 2^(r - 39) per element. Measured here, per row
    (max over the row / the row's own max, K = 2 304): r = 0, 8, 16: ~1e-7 (22 bits); r = 20: 1.4e-6, still inside 6e-6; r = 24: 1.8e-5;
    r = 32: 7e-3; r = 40: the scaled values are <= 2^-25, half the smallest subnormal, and the whole row is EXACTLY zero. The knee
    is at r = 20. Consequence: under fp16x3 a channel or frame of a gradient more than ~2^20 (1e6) below its
    tensor's largest entry is not fp32-grade relative to itself, and one 2^40 (1e12) below is dropped."""
    a, b, r = _case()
    ref = a.double() @ b.double().t()
    emul = ideal_split_product(lambda x, y: x @ y.t(), a, b, 2)
    err = _worst_by_r(per_row_error(emul, ref), r)
    print("[parity] ideal fp16x3 product, per-row error by r:", {k: f"{v:.2e}" for k, v in err.items()})
    assert FP16X3_KNEE == 20
    for rv in ROW_EXPONENTS:
        if rv <= FP16X3_KNEE:
            assert err[rv] <= ROW_TOL, (rv, err[rv])
    assert ROW_TOL < err[24] < err[32] < err[40], "beyond the knee the per-row error must grow with r"
    assert not emul[r == 40].any() and err[40] == 1.0, "rows 2^40 below the tensor's maximum must come out exactly zero"
    assert emul[r == 32].any(), "rows 2^32 below the maximum are coarse, not dropped"


@pytest.mark.parametrize("parts", [3, 2])
def test_the_tensor_wide_criterion_does_not_see_the_small_rows(parts):
    """why the per-row tests exist: divided by the TENSOR's maximum, as `close()` does, the same products pass at 6e-6 for both forms —
    fp16x3's zeroed and coarse rows included"""
    a, b, _ = _case()
    ref = a.double() @ b.double().t()
    emul = ideal_split_product(lambda x, y: x @ y.t(), a, b, parts)
    assert (emul - ref).abs().max().item() <= ROW_TOL * ref.abs().max().item()
