"""CPU: the value an IDEAL split-operand GEMM computes (csrc/split3.hip: precision = "bf16x6" / "fp16x3"), from torch's own 16-bit
roundings with every product and sum in fp64. What separates a device result from this is the fp32 accumulation alone; what separates
this from the fp64 product of the unsplit operands is the representation: exact for bf16 triples, 22 bits of the SCALED value for fp16
pairs — with one power-of-two scale per tensor, so an element 2^r below its tensor's largest magnitude keeps those 22 bits only while
its `mid` part is a normal binary16 (r <= 17), loses them at 2^(r - 39) relative beyond and is exactly zero from r = 40.

Used by tests/test_split_rows_host.py (the arithmetic alone, no GPU) and tests/test_gpu_ops.py (the kernels against it, row by row)."""
import math

import torch

# rows of the scaled operand sit at 2^-r of the tensor's largest magnitude
ROW_EXPONENTS = (0, 8, 16, 20, 24, 32, 40)
ROW_TOL = 6e-6            # the split engine's existing criterion (tests/test_gpu_ops.py), here per output row
FP16X3_KNEE = 20          # largest r of ROW_EXPONENTS at which fp16x3 still meets ROW_TOL per row (test_split_rows_host.py pins it)


def split_host(x, parts, s=1.0):
    """the parts computed by torch on the host (round to nearest even): bf16 (hi, mid, lo) of x, or fp16 (hi, mid) of x * s"""
    dt = torch.bfloat16 if parts == 3 else torch.float16
    v = x * s
    hi = v.to(dt)
    r1 = v - hi.float()
    mid = r1.to(dt)
    return (hi, mid, (r1 - mid.float()).to(dt)) if parts == 3 else (hi, mid)


def host_scale(x):
    """scale_of_amax (csrc/split3.hip) of an fp32 tensor: the power of two that puts its largest magnitude into [2^14, 2^15); 1 for an
    all-zero tensor; clamped for magnitudes below 2^-113"""
    a = x.abs().max().item()
    if a == 0.0:
        return 1.0
    e = max(int(torch.tensor([a], dtype=torch.float32).view(torch.int32).item()) >> 23, 14)
    return 2.0 ** (141 - e)


def ideal_split_product(op, a, b, parts):
    """op(A, B) for a bilinear fp64 function `op` (a matrix product, a convolution's weight gradient) as the split engine forms it:
    parts = 3: the six bf16 products hi hi, hi mid, mid hi, hi lo, lo hi, mid mid; parts = 2: hi hi + hi mid + mid hi of the fp16
    roundings of the scaled operands, unscaled afterwards. Grouped by the first operand's part (the sums of parts are exact in fp64)."""
    sa, sb = (1.0, 1.0) if parts == 3 else (host_scale(a), host_scale(b))
    pa = [t.double() for t in split_host(a, parts, sa)]
    pb = [t.double() for t in split_host(b, parts, sb)]
    if parts == 3:
        out = op(pa[0], pb[0] + pb[1] + pb[2]) + op(pa[1], pb[0] + pb[1]) + op(pa[2], pb[0])
    else:
        out = op(pa[0], pb[0] + pb[1]) + op(pa[1], pb[0])
    return out / sa / sb                                   # powers of two: exact


def rows_at_exponents(x, dim):
    """x with slice i along `dim` multiplied by 2^-ROW_EXPONENTS[i % 7] (exact), and the exponent of every slice"""
    n = x.shape[dim]
    r = torch.tensor([ROW_EXPONENTS[i % len(ROW_EXPONENTS)] for i in range(n)])
    shape = [1] * x.dim()
    shape[dim] = n
    return x * torch.pow(2.0, -r.double()).float().view(shape), r


def per_row_error(got, want):
    """max |got - want| of every row (first axis) over that row's max |want|; 0 where both rows are all zero"""
    got = got.detach().cpu().double().reshape(got.shape[0], -1)
    want = want.detach().cpu().double().reshape(want.shape[0], -1)
    err = (got - want).abs().amax(dim=1)
    scale = want.abs().amax(dim=1)
    return torch.where(scale > 0, err / scale.clamp_min(1e-300), torch.where(err > 0, torch.full_like(err, math.inf), torch.zeros_like(err)))


def check_rows(name, got, emul, ref, r, parts):
    """the per-row contract of a split GEMM whose output rows are fed by operand rows at 2^-r of their tensor's maximum:
    device vs the ideal split product within ROW_TOL of the row's max |emulation| (fp32 accumulation only) and exactly zero where the
    emulation is; device vs fp64 within ROW_TOL per row for every r (bf16x6) or r <= FP16X3_KNEE (fp16x3)"""
    got = got.detach().cpu()
    e_emul, e_ref = per_row_error(got, emul), per_row_error(got, ref)
    for rv in ROW_EXPONENTS:
        sel = r == rv
        if sel.any():
            print(f"[parity] {name} parts={parts} rows at 2^-{rv}: vs ideal split product {e_emul[sel].max().item():.3e}, vs fp64 {e_ref[sel].max().item():.3e} (per-row)")
    dead = emul.reshape(emul.shape[0], -1).abs().amax(dim=1) == 0
    assert not got.reshape(got.shape[0], -1)[dead].any(), f"{name}: non-zero output where the ideal split product is exactly zero"
    assert (e_emul <= ROW_TOL).all(), f"{name}: rows {torch.nonzero(e_emul > ROW_TOL).flatten().tolist()[:8]} are {e_emul.max().item():.3e} from the ideal split product"
    held = torch.ones_like(r, dtype=torch.bool) if parts == 3 else r <= FP16X3_KNEE
    assert (e_ref[held] <= ROW_TOL).all(), f"{name}: a row inside the format's range is {e_ref[held].max().item():.3e} of its own scale from fp64"
