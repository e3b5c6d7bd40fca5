"""Thin torch-tensor wrappers over the C ABI (include/goalnet_hip.h).

PyTorch is plumbing here: device memory (caching allocator), the current HIP stream and
torch.distributed. Every arithmetic operation of the hot path runs in libgoalnet_hip.so.
Tensors are fp32, on the GPU, in the device layouts named in the header (NHWC / OHWI).
"""
from __future__ import annotations

import ctypes
import os

import torch

from . import _lib
from ._lib import STAT_PARTS, check

F32 = torch.float32


def _s():
    return torch.cuda.current_stream().cuda_stream


def _p(t):
    return 0 if t is None else t.data_ptr()


def _chk(*ts, f64=True):
    """f64=False: the wrapper takes no float64 tensor (no fp64 partial sums, no workspace of the caller's): one that arrives is an fp32
    tensor that was never converted, and its bytes would be read as twice as many floats"""
    for t in ts:
        if t is None:
            continue
        if not t.is_cuda:
            raise _lib.GoalnetError("expected a GPU tensor")
        if t.dtype not in (F32, torch.float64, torch.uint8, torch.bfloat16, torch.float16, torch.int32) or (t.dtype == torch.float64 and not f64):
            raise _lib.GoalnetError(f"unexpected dtype {t.dtype}")


def _f32c(who, **ts):
    """every tensor given is fp32 and contiguous: the kernels behind `who` take a bare pointer and an element count"""
    for name, t in ts.items():
        _req(t is None or (t.dtype == F32 and t.is_contiguous()), f"{who}: {name} must be a contiguous float32 tensor")


def _req(cond, msg):
    """argument / shape checks raise RuntimeError (what ATen raises for a shape mismatch in the reference, SURVEY.md §8(b)
    "Ownership / errors"); unlike `assert` they survive `python -O`"""
    if not cond:
        raise RuntimeError(msg)


def _ld(t):
    """leading dimension (row stride) of a 2-D view with unit column stride"""
    _req(t.dim() == 2 and (t.shape[1] == 1 or t.stride(1) == 1), "_ld: argument check failed: t.dim() == 2 and (t.shape[1] == 1 or t.stride(1) == 1)")
    return t.stride(0)


def lib():
    return _lib.load()


# ---------------------------------------------------------------------------------------------
def fill_uniform(dst, seed, tensor_id, lo, hi):
    _chk(dst)
    _req(dst.is_contiguous() and dst.dtype == F32, "fill_uniform: argument check failed: dst.is_contiguous() and dst.dtype == F32")
    check(lib().goalnet_fill_uniform(dst.data_ptr(), dst.numel(), seed, tensor_id, lo, hi, _s()), "fill_uniform")
    return dst


def dropout_mask(dst, seed, tensor_id, p):
    _chk(dst)
    _req(dst.is_contiguous() and dst.dtype == F32, "dropout_mask: argument check failed: dst.is_contiguous() and dst.dtype == F32")
    check(lib().goalnet_dropout_mask(dst.data_ptr(), dst.numel(), seed, tensor_id, p, _s()), "dropout_mask")
    return dst


def transpose_inner(src, dst, B, R, C):
    """[B][R][C] -> [B][C][R] on contiguous buffers"""
    _chk(src, dst)
    _req(src.is_contiguous() and dst.is_contiguous() and src.numel() == dst.numel() == B * R * C, "transpose_inner: argument check failed: src.is_contiguous() and dst.is_contiguous() and src.numel() == dst.numel() == B * R * C")
    check(lib().goalnet_transpose_inner(src.data_ptr(), dst.data_ptr(), B, R, C, _s()), "transpose_inner")
    return dst


def conv3x3_weight_flip(w, wt, cout, cin):
    _chk(w, wt)
    _req(w.numel() == wt.numel() == cout * cin * 9, "conv3x3_weight_flip: argument check failed: w.numel() == wt.numel() == cout * cin * 9")
    check(lib().goalnet_conv3x3_weight_flip(w.data_ptr(), wt.data_ptr(), cout, cin, _s()), "conv3x3_weight_flip")
    return wt


def conv3x3_weight_flip2(wa, wta, couta, cina, wb, wtb, coutb, cinb):
    _chk(wa, wta, wb, wtb)
    _req(wa.numel() == wta.numel() == couta * cina * 9 and wb.numel() == wtb.numel() == coutb * cinb * 9, "conv3x3_weight_flip2: sizes")
    check(lib().goalnet_conv3x3_weight_flip2(wa.data_ptr(), wta.data_ptr(), couta, cina, wb.data_ptr(), wtb.data_ptr(), coutb, cinb, _s()),
          "conv3x3_weight_flip2")


def conv1_fwd(x_nchw, w, b, y, N, H, W):
    _chk(x_nchw, w, b, y, f64=False)
    _f32c("conv1_fwd", x_nchw=x_nchw, w=w, b=b, y=y)
    _req(x_nchw.is_contiguous() and x_nchw.numel() == N * 3 * H * W, "conv1_fwd: argument check failed: x_nchw.is_contiguous() and x_nchw.numel() == N * 3 * H * W")
    Ho, Wo = (H + 3) // 3 + 1, (W + 3) // 3 + 1
    _req(y.numel() == N * Ho * Wo * 64 and w.numel() == 64 * 27 and b.numel() == 64, "conv1_fwd: argument check failed: y.numel() == N * Ho * Wo * 64 and w.numel() == 64 * 27 and b.numel() == 64")
    check(lib().goalnet_conv1_fwd(x_nchw.data_ptr(), w.data_ptr(), b.data_ptr(), y.data_ptr(), N, H, W, _s()), "conv1_fwd")
    return y


def conv1_wgrad(x_nchw, dy, dw, db, N, H, W):
    _chk(x_nchw, dy, dw, db, f64=False)
    _f32c("conv1_wgrad", x_nchw=x_nchw, dy=dy, dw=dw, db=db)
    Ho, Wo = (H + 3) // 3 + 1, (W + 3) // 3 + 1
    _req(x_nchw.numel() == N * 3 * H * W, "conv1_wgrad: argument check failed: x_nchw.numel() == N * 3 * H * W")
    _req(dy.numel() == N * Ho * Wo * 64 and dw.numel() == 64 * 27 and db.numel() == 64, "conv1_wgrad: argument check failed: dy.numel() == N * Ho * Wo * 64 and dw.numel() == 64 * 27 and db.numel() == 64")
    nbytes = lib().goalnet_conv1_wgrad_ws_bytes(N, H, W)
    ws = torch.empty(nbytes // 4, dtype=F32, device=dy.device)
    check(lib().goalnet_conv1_wgrad(x_nchw.data_ptr(), dy.data_ptr(), dw.data_ptr(), db.data_ptr(), ws.data_ptr(), nbytes,
                                    N, H, W, _s()), "conv1_wgrad")


def conv1_dgrad(dy, w, out, reduce, N, H, W):
    """conv1's data gradient from dy (N,Ho,Wo,64): out = dx (N,3,H,W), or with reduce=1 max_ci |dx| (N,H,W); bit-equal arithmetic"""
    _chk(dy, w, out)
    Ho, Wo = (H + 3) // 3 + 1, (W + 3) // 3 + 1
    _req(dy.dtype == F32 and out.dtype == F32 and dy.is_contiguous() and out.is_contiguous(), "conv1_dgrad: contiguous fp32 tensors")
    _req(dy.numel() == N * Ho * Wo * 64 and w.numel() == 64 * 27 and out.numel() == N * (1 if reduce else 3) * H * W,
         "conv1_dgrad: dy (N,Ho,Wo,64), w (64,3,3,3), out (N,3,H,W) or (N,H,W)")
    check(lib().goalnet_conv1_dgrad(dy.data_ptr(), w.data_ptr(), out.data_ptr(), int(reduce), N, H, W, _s()), "conv1_dgrad")
    return out


def stat_parts(units):
    """rows of a partial-sum buffer for `units` independent work items (frames): min(units, STAT_PARTS)"""
    return max(1, min(int(units), STAT_PARTS))


def _rows(partials, width):
    """the partial-sum kernels take the row count from the buffer the caller allocated: [nparts][width] doubles"""
    _req(partials.dtype == torch.float64 and partials.is_contiguous() and partials.numel() % width == 0, "_rows: argument check failed: partials.dtype == torch.float64 and partials.is_contiguous() and partials.numel() % width == 0")
    n = partials.numel() // width
    _req(1 <= n <= STAT_PARTS, "_rows: argument check failed: 1 <= n <= STAT_PARTS")
    return n


def idx_to_nhwc(idx, N, Hp, Wp, C):
    """argmax bytes as the kernels store them ([N][C/S][Hp][Wp][S], S = 32 or C; include/goalnet_hip.h) -> (N, Hp, Wp, C)"""
    S = 32 if C % 32 == 0 else C
    return idx.reshape(N, C // S, Hp, Wp, S).permute(0, 2, 3, 1, 4).reshape(N, Hp, Wp, C)


def pool_bnstats_fwd(y, p, idx, partials, N, Hc, Wc, C):
    _chk(y, p, idx, partials)
    _req(y.numel() == N * Hc * Wc * C and p.numel() == N * (Hc - 2) * (Wc - 2) * C, "pool_bnstats_fwd: argument check failed: y.numel() == N * Hc * Wc * C and p.numel() == N * (Hc - 2) * (Wc - 2) * C")
    _req(idx is None or (idx.dtype == torch.uint8 and idx.numel() == p.numel()), "pool_bnstats_fwd: argument check failed: idx is None or (idx.dtype == torch.uint8 and idx.numel() == p.numel())")
    if p.dtype in H16:                              # pooled activation stored in 16 bits (statistics of the stored values)
        check(lib().goalnet_pool_bnstats_fwd_p16(y.data_ptr(), int(y.dtype in H16), p.data_ptr(), _p(idx), partials.data_ptr(),
                                                 _rows(partials, 2 * C), N, Hc, Wc, C, _f16(y, p), _s()), "pool_bnstats_fwd_p16")
        return
    _req(y.dtype == F32, "pool_bnstats_fwd: argument check failed: y.dtype == F32")
    check(lib().goalnet_pool_bnstats_fwd(y.data_ptr(), p.data_ptr(), _p(idx), partials.data_ptr(), _rows(partials, 2 * C),
                                         N, Hc, Wc, C, _s()), "pool_bnstats_fwd")


def bn_finalize(partials, gamma, beta, rmean, rvar, momentum, eps, count, C, mean, invstd, scale, shift):
    _chk(partials, gamma, beta, rmean, rvar, mean, invstd, scale, shift)
    for t in (gamma, beta, mean, invstd, scale, shift):
        _req(t.numel() == C and t.is_contiguous(), "bn_finalize: argument check failed: t.numel() == C and t.is_contiguous()")
    check(lib().goalnet_bn_finalize(partials.data_ptr(), _rows(partials, 2 * C), gamma.data_ptr(), beta.data_ptr(), _p(rmean), _p(rvar), momentum, eps,
                                    count, C, mean.data_ptr(), invstd.data_ptr(), scale.data_ptr(), shift.data_ptr(), _s()),
          "bn_finalize")


def bn_bwd_reduce(dz, p, mean, invstd, partials, npix, C):
    """dz: fp32, or bf16 as the *_o16 GEMMs write it; p: fp32, or bf16 as pool_bnstats_fwd stores it into a bf16 tensor"""
    _chk(dz, p, mean, invstd, partials)
    _req(dz.numel() == p.numel() == npix * C, "bn_bwd_reduce: argument check failed: dz.numel() == p.numel() == npix * C")
    if dz.dtype in H16 or p.dtype in H16:
        check(lib().goalnet_bn_bwd_reduce_t(dz.data_ptr(), int(dz.dtype in H16), p.data_ptr(), int(p.dtype in H16),
                                            mean.data_ptr(), invstd.data_ptr(), partials.data_ptr(), _rows(partials, 2 * C), npix, C,
                                            _f16(dz, p), _s()), "bn_bwd_reduce_t")
        return
    check(lib().goalnet_bn_bwd_reduce(dz.data_ptr(), p.data_ptr(), mean.data_ptr(), invstd.data_ptr(), partials.data_ptr(),
                                      _rows(partials, 2 * C), npix, C, _s()), "bn_bwd_reduce")


def bn_bwd_finalize(partials, gamma, mean, invstd, count, C, dgamma, dbeta, coef3):
    _chk(partials, gamma, mean, invstd, dgamma, dbeta, coef3)
    _req(coef3.numel() == 3 * C and dgamma.numel() == C and dbeta.numel() == C, "bn_bwd_finalize: argument check failed: coef3.numel() == 3 * C and dgamma.numel() == C and dbeta.numel() == C")
    check(lib().goalnet_bn_bwd_finalize(partials.data_ptr(), _rows(partials, 2 * C), gamma.data_ptr(), mean.data_ptr(), invstd.data_ptr(), count, C,
                                        dgamma.data_ptr(), dbeta.data_ptr(), coef3.data_ptr(), _s()), "bn_bwd_finalize")


def bnpool_bwd(dz, p, idx, coef3, dy, dbias_partials, N, Hc, Wc, C):
    _chk(dz, p, idx, coef3, dy, dbias_partials)
    npool = N * (Hc - 2) * (Wc - 2) * C
    _req(dz.numel() == p.numel() == idx.numel() == npool and dy.numel() == N * Hc * Wc * C, "bnpool_bwd: argument check failed: dz.numel() == p.numel() == idx.numel() == npool and dy.numel() == N * Hc * Wc * C")
    if dz.dtype in H16 or p.dtype in H16:
        check(lib().goalnet_bnpool_bwd_bf16p_t(dz.data_ptr(), int(dz.dtype in H16), p.data_ptr(), int(p.dtype in H16),
                                               idx.data_ptr(), coef3.data_ptr(), dy.data_ptr(), None, dbias_partials.data_ptr(),
                                               _rows(dbias_partials, C), N, Hc, Wc, C, _f16(dz, p), _s()), "bnpool_bwd_bf16p_t")
        return
    check(lib().goalnet_bnpool_bwd(dz.data_ptr(), p.data_ptr(), idx.data_ptr(), coef3.data_ptr(), dy.data_ptr(),
                                   dbias_partials.data_ptr(), _rows(dbias_partials, C), N, Hc, Wc, C, _s()), "bnpool_bwd")


def bnpool_bwd_bf16p(dz, p, idx, coef3, dy, dypad, dbias_partials, N, Hc, Wc, C):
    _chk(dz, p, idx, coef3, dy, dypad, dbias_partials)
    _req(dypad.dtype in H16 and dypad.numel() >= N * (Hc + 2) * (Wc + 2) * C, "bnpool_bwd_bf16p: argument check failed: dypad.dtype in H16 and dypad.numel() >= N * (Hc + 2) * (Wc + 2) * C")
    if dz.dtype in H16 or p.dtype in H16:
        check(lib().goalnet_bnpool_bwd_bf16p_t(dz.data_ptr(), int(dz.dtype in H16), p.data_ptr(), int(p.dtype in H16),
                                               idx.data_ptr(), coef3.data_ptr(), _p(dy), dypad.data_ptr(), dbias_partials.data_ptr(),
                                               _rows(dbias_partials, C), N, Hc, Wc, C, _f16(dz, p, dypad), _s()), "bnpool_bwd_bf16p_t")
        return
    check(lib().goalnet_bnpool_bwd_bf16p(dz.data_ptr(), p.data_ptr(), idx.data_ptr(), coef3.data_ptr(), _p(dy),
                                         dypad.data_ptr(), dbias_partials.data_ptr(), _rows(dbias_partials, C), N, Hc, Wc, C,
                                         _f16(dypad), _s()), "bnpool_bwd_bf16p")


SMALL_BN_ELEMS = 1 << 20       # conv outputs of up to this many elements (C <= 512) take the small-shape pool / BatchNorm kernels


def pool_bn_fwd_small(y, p, idx, gamma, beta, rmean, rvar, momentum, eps, st, N, Hc, Wc, C):
    """pool_bnstats_fwd + bn_finalize in one launch (small fp32 shapes); st = (4, C): mean, invstd, scale, shift"""
    _chk(y, p, idx, gamma, beta, rmean, rvar, st)
    _req(y.dtype == F32 and p.dtype == F32 and y.numel() == N * Hc * Wc * C and p.numel() == N * (Hc - 2) * (Wc - 2) * C,
         "pool_bn_fwd_small: fp32 y (N,Hc,Wc,C) and p (N,Hc-2,Wc-2,C)")
    _req(idx is None or (idx.dtype == torch.uint8 and idx.numel() == p.numel()), "pool_bn_fwd_small: idx must be uint8, one per pooled element")
    _req(st.numel() == 4 * C and st.is_contiguous(), "pool_bn_fwd_small: st must be (4, C)")
    nbytes = lib().goalnet_bn_small_ws_bytes(C)
    ws = torch.empty(nbytes // 8, dtype=torch.float64, device=y.device)
    ctr = _tile_counters(("pool_bn_fwd", N, Hc, Wc, C), y.device)
    check(lib().goalnet_pool_bn_fwd_small(y.data_ptr(), p.data_ptr(), _p(idx), gamma.data_ptr(), beta.data_ptr(), _p(rmean), _p(rvar),
                                          momentum, eps, st[0].data_ptr(), st[1].data_ptr(), st[2].data_ptr(), st[3].data_ptr(),
                                          ws.data_ptr(), nbytes, ctr.data_ptr(), N, Hc, Wc, C, _s()), "pool_bn_fwd_small")


def bn_bwd_reduce_small(dz, p, mean, invstd, gamma, dgamma, dbeta, coef3, N, Hc, Wc, C):
    """bn_bwd_reduce + bn_bwd_finalize in one launch (small fp32 shapes)"""
    _chk(dz, p, mean, invstd, gamma, dgamma, dbeta, coef3)
    npool = N * (Hc - 2) * (Wc - 2) * C
    _req(dz.dtype == F32 and p.dtype == F32 and dz.numel() == p.numel() == npool, "bn_bwd_reduce_small: fp32 dz / p of the pooled shape")
    _req(dgamma.numel() == C and dbeta.numel() == C and coef3.numel() == 3 * C, "bn_bwd_reduce_small: dgamma, dbeta (C), coef3 (3 C)")
    nbytes = lib().goalnet_bn_small_ws_bytes(C)
    ws = torch.empty(nbytes // 8, dtype=torch.float64, device=dz.device)
    ctr = _tile_counters(("bn_bwd_reduce", N, Hc, Wc, C), dz.device)
    check(lib().goalnet_bn_bwd_reduce_small(dz.data_ptr(), p.data_ptr(), mean.data_ptr(), invstd.data_ptr(), gamma.data_ptr(), dgamma.data_ptr(),
                                            dbeta.data_ptr(), coef3.data_ptr(), ws.data_ptr(), nbytes, ctr.data_ptr(), N, Hc, Wc, C, _s()),
          "bn_bwd_reduce_small")


def pool_bn_eval_fwd(y, p, idx, gamma, beta, rmean, rvar, eps, st, N, Hc, Wc, C):
    """eval mode, one launch: max-pool (+ argmax when idx is given) as pool_bnstats_fwd stores it, and st = (4, C) = (running_mean,
    invstd, scale, shift) from the running buffers (read only). y / p: fp32, or 16-bit as the 16-bit paths store them."""
    _chk(y, p, idx, gamma, beta, rmean, rvar, st)
    _req(y.numel() == N * Hc * Wc * C and p.numel() == N * (Hc - 2) * (Wc - 2) * C, "pool_bn_eval_fwd: y (N,Hc,Wc,C) and p (N,Hc-2,Wc-2,C)")
    _req(idx is None or (idx.dtype == torch.uint8 and idx.numel() == p.numel()), "pool_bn_eval_fwd: idx must be uint8, one per pooled element")
    _req(p.dtype in H16 or y.dtype == F32, "pool_bn_eval_fwd: a 16-bit y needs a 16-bit p")
    for t in (gamma, beta, rmean, rvar):
        _req(t.dtype == F32 and t.numel() == C and t.is_contiguous(), "pool_bn_eval_fwd: gamma, beta, running stats must be fp32 (C)")
    _req(st.dtype == F32 and st.numel() == 4 * C and st.is_contiguous(), "pool_bn_eval_fwd: st must be fp32 (4, C)")
    check(lib().goalnet_pool_bn_eval_fwd(y.data_ptr(), int(y.dtype in H16), p.data_ptr(), int(p.dtype in H16), _p(idx), gamma.data_ptr(),
                                         beta.data_ptr(), rmean.data_ptr(), rvar.data_ptr(), eps, st.data_ptr(), stat_parts(8 * N),
                                         N, Hc, Wc, C, _f16(y, p), _s()), "pool_bn_eval_fwd")
    return p, idx, st


def bn_bwd_finalize_eval(partials, gamma, invstd, C, dgamma, dbeta, coef3):
    """eval mode: dgamma, dbeta from bn_bwd_reduce's partials (taken with the running mean / invstd), coef3 = (gamma invstd, 0, 0)"""
    _chk(partials, gamma, invstd, dgamma, dbeta, coef3)
    _req(coef3.numel() == 3 * C and dgamma.numel() == C and dbeta.numel() == C and gamma.numel() == C and invstd.numel() == C,
         "bn_bwd_finalize_eval: gamma, invstd, dgamma, dbeta (C), coef3 (3 C)")
    check(lib().goalnet_bn_bwd_finalize_eval(partials.data_ptr(), _rows(partials, 2 * C), gamma.data_ptr(), invstd.data_ptr(), C,
                                             dgamma.data_ptr(), dbeta.data_ptr(), coef3.data_ptr(), _s()), "bn_bwd_finalize_eval")


def bn_bwd_reduce_small_eval(dz, p, mean, invstd, gamma, dgamma, dbeta, coef3, N, Hc, Wc, C):
    """eval-mode bn_bwd_reduce_small: mean / invstd are the running statistics; coef3 = (gamma invstd, 0, 0)"""
    _chk(dz, p, mean, invstd, gamma, dgamma, dbeta, coef3)
    npool = N * (Hc - 2) * (Wc - 2) * C
    _req(dz.dtype == F32 and p.dtype == F32 and dz.numel() == p.numel() == npool, "bn_bwd_reduce_small_eval: fp32 dz / p of the pooled shape")
    _req(dgamma.numel() == C and dbeta.numel() == C and coef3.numel() == 3 * C, "bn_bwd_reduce_small_eval: dgamma, dbeta (C), coef3 (3 C)")
    nbytes = lib().goalnet_bn_small_ws_bytes(C)
    ws = torch.empty(nbytes // 8, dtype=torch.float64, device=dz.device)
    ctr = _tile_counters(("bn_bwd_reduce_eval", N, Hc, Wc, C), dz.device)
    check(lib().goalnet_bn_bwd_reduce_small_eval(dz.data_ptr(), p.data_ptr(), mean.data_ptr(), invstd.data_ptr(), gamma.data_ptr(),
                                                 dgamma.data_ptr(), dbeta.data_ptr(), coef3.data_ptr(), ws.data_ptr(), nbytes,
                                                 ctr.data_ptr(), N, Hc, Wc, C, _s()), "bn_bwd_reduce_small_eval")


def bnpool_bwd_small(dz, p, idx, coef3, dy, dbias, N, Hc, Wc, C):
    """bnpool_bwd + the conv bias gradient in one launch (small fp32 shapes; a direct 9-window gather)"""
    _chk(dz, p, idx, coef3, dy, dbias)
    npool = N * (Hc - 2) * (Wc - 2) * C
    _req(dz.dtype == F32 and p.dtype == F32 and dz.numel() == p.numel() == idx.numel() == npool and dy.numel() == N * Hc * Wc * C and dbias.numel() == C,
         "bnpool_bwd_small: fp32 dz / p / idx of the pooled shape, dy of the conv shape, dbias (C)")
    nbytes = lib().goalnet_bn_small_ws_bytes(C)
    ws = torch.empty(nbytes // 8, dtype=torch.float64, device=dz.device)
    ctr = _tile_counters(("bnpool_bwd", N, Hc, Wc, C), dz.device)
    check(lib().goalnet_bnpool_bwd_small(dz.data_ptr(), p.data_ptr(), idx.data_ptr(), coef3.data_ptr(), dy.data_ptr(), dbias.data_ptr(),
                                         ws.data_ptr(), nbytes, ctr.data_ptr(), N, Hc, Wc, C, _s()), "bnpool_bwd_small")


def partials_sum(partials, nparts, stride, C, out):
    _chk(partials, out)
    _req(partials.dtype == torch.float64 and out.numel() == C, "partials_sum: argument check failed: partials.dtype == torch.float64 and out.numel() == C")
    check(lib().goalnet_partials_sum(partials.data_ptr(), nparts, stride, C, out.data_ptr(), _s()), "partials_sum")


def partials_sum2(pa, Ca, oa, pb, Cb, ob):
    """partials_sum of two [rows][C] arrays in one launch"""
    _chk(pa, oa, pb, ob)
    _req(oa.numel() == Ca and ob.numel() == Cb, "partials_sum2: out sizes")
    check(lib().goalnet_partials_sum2(pa.data_ptr(), _rows(pa, Ca), Ca, oa.data_ptr(), pb.data_ptr(), _rows(pb, Cb), Cb, ob.data_ptr(), _s()),
          "partials_sum2")


def partials_sum_f64(partials, C, out):
    """out[c] (double) = sum over the rows of partials[rows][C]"""
    _chk(partials, out)
    _req(partials.dtype == torch.float64 and out.dtype == torch.float64 and out.numel() == C, "partials_sum_f64: argument check failed: partials.dtype == torch.float64 and out.dtype == torch.float64 and out.numel() == C")
    check(lib().goalnet_partials_sum_f64(partials.data_ptr(), _rows(partials, C), C, C, out.data_ptr(), _s()), "partials_sum_f64")


N_TILE_CTR = 1024
# The fused split-K reduction (the last block of a tile sums its slabs) is built and tested, and OFF by default: one block summing
# 13 slabs x 64 KB is a chain of ~50 dependent memory round trips (measured on the 10-frame step: +450 us per step against the
# separate reduce launch, which spreads the same bytes over every CU and costs 1.6 us of launch gap inside a graph)
FUSED_SPLITK = os.environ.get("GOALNET_FUSED_SPLITK", "0") == "1"
_TILE_CTR = {}
_WGRAD_CODES = {}


def _tile_counters(key, device):
    """zeroed int32 ticket counters lent to the fused split-K reduction of one call site (include/goalnet_hip.h: zero on entry,
    zero again on exit). One tensor per (call site, shape): calls that may overlap on two streams — a weight gradient on the
    side stream under a data gradient on the main one — never share counters."""
    k = (key, device.index)
    t = _TILE_CTR.get(k)
    if t is None:
        t = _TILE_CTR[k] = torch.zeros(N_TILE_CTR, dtype=torch.int32, device=device)
    return t


def conv3x3_fwd(x, scale, shift, w, bias, relu, y, N, H, W, Cin, Cout):
    _chk(x, scale, shift, w, bias, y)
    _req(x.numel() == N * H * W * Cin and y.numel() == N * H * W * Cout and w.numel() == Cout * 9 * Cin, "conv3x3_fwd: argument check failed: x.numel() == N * H * W * Cin and y.numel() == N * H * W * Cout and w.numel() == Cout * 9 * Cin")
    _req(scale is None or (scale.numel() == Cin and shift.numel() == Cin), "conv3x3_fwd: argument check failed: scale is None or (scale.numel() == Cin and shift.numel() == Cin)")
    _req(bias is None or bias.numel() == Cout, "conv3x3_fwd: argument check failed: bias is None or bias.numel() == Cout")
    nbytes = lib().goalnet_conv3x3_fwd_ws_bytes(N, H, W, Cin, Cout)       # > 0 only for small N (split-K slabs)
    ws = torch.empty(nbytes // 4, dtype=F32, device=x.device) if nbytes else None
    ctr = _tile_counters(("conv3x3_fwd", N, H, W, Cin, Cout, scale is None), x.device) if (nbytes and FUSED_SPLITK) else None
    check(lib().goalnet_conv3x3_fwd(x.data_ptr(), _p(scale), _p(shift), w.data_ptr(), _p(bias), int(relu), y.data_ptr(),
                                    N, H, W, Cin, Cout, _p(ws), nbytes, _p(ctr), N_TILE_CTR if ctr is not None else 0, _s()), "conv3x3_fwd")
    return y


def conv3x3_wgrad(x, scale, shift, dy, dw, N, H, W, Cin, Cout):
    _chk(x, scale, shift, dy, dw)
    _req(x.numel() == N * H * W * Cin and dy.numel() == N * H * W * Cout and dw.numel() == Cout * 9 * Cin, "conv3x3_wgrad: argument check failed: x.numel() == N * H * W * Cin and dy.numel() == N * H * W * Cout and dw.numel() == Cout * 9 * Cin")
    nbytes = lib().goalnet_conv3x3_wgrad_ws_bytes(N, H, W, Cin, Cout)
    ws = torch.empty(nbytes // 4, dtype=F32, device=x.device)
    # the border-code table depends on (N, H, W) only: built once per shape and device, not once per call
    ck = (N, H, W, x.device.index)
    codes = _WGRAD_CODES.get(ck)
    if codes is None:
        codes = torch.empty(lib().goalnet_conv3x3_wgrad_codes_bytes(N, H, W) // 4, dtype=torch.int32, device=x.device)
        check(lib().goalnet_conv3x3_wgrad_codes(codes.data_ptr(), N, H, W, _s()), "conv3x3_wgrad_codes")
        if len(_WGRAD_CODES) < 64 and N * H * W <= (1 << 22):
            _WGRAD_CODES[ck] = codes
    ctr = _tile_counters(("conv3x3_wgrad", N, H, W, Cin, Cout), x.device) if FUSED_SPLITK else None
    check(lib().goalnet_conv3x3_wgrad(x.data_ptr(), _p(scale), _p(shift), dy.data_ptr(), dw.data_ptr(), ws.data_ptr(), nbytes,
                                      codes.data_ptr(), _p(ctr), N_TILE_CTR if ctr is not None else 0, N, H, W, Cin, Cout, _s()), "conv3x3_wgrad")
    return dw


BF16 = torch.bfloat16
F16 = torch.float16
H16 = (BF16, F16)          # the 16-bit storage formats of the reduced-precision engine; the C ABI's `f16` flag = (dtype == float16)
ADAM_RANGES_MAX = _lib.ADAM_RANGES_MAX     # ranges one adam_step_dev_ranges launch takes


def _f16(*ts):
    """the `f16` flag of a call: 1 when its 16-bit tensors are torch.float16, 0 for bfloat16 (they must agree)"""
    kinds = {t.dtype for t in ts if t is not None and t.dtype in H16}
    _req(len(kinds) <= 1, "_f16: 16-bit operands of one call must share a format")
    return int(F16 in kinds)


def cast_bf16(x, y):
    _chk(x, y)
    _req(x.dtype == F32 and y.dtype in H16 and x.is_contiguous() and y.is_contiguous() and x.numel() == y.numel(), "cast_bf16: argument check failed: x.dtype == F32 and y.dtype in H16 and x.is_contiguous() and y.is_contiguous() and x.numel() == y.numel()")
    check(lib().goalnet_cast_bf16(x.data_ptr(), y.data_ptr(), x.numel(), _f16(y), _s()), "cast_bf16")
    return y


def cast_f32(x, y):
    _chk(x, y)
    _req(x.dtype in H16 and y.dtype == F32 and x.is_contiguous() and y.is_contiguous() and x.numel() == y.numel(), "cast_f32: argument check failed: x.dtype in H16 and y.dtype == F32 and x.is_contiguous() and y.is_contiguous() and x.numel() == y.numel()")
    check(lib().goalnet_cast_f32(x.data_ptr(), y.data_ptr(), x.numel(), _f16(x), _s()), "cast_f32")
    return y


def bn_apply_bf16(x, scale, shift, y, C):
    _chk(x, scale, shift, y)
    _req(x.dtype in (F32,) + H16 and y.dtype in H16 and x.numel() == y.numel() and scale.numel() == C, "bn_apply_bf16: argument check failed: x.dtype in (F32,) + H16 and y.dtype in H16 and x.numel() == y.numel() and scale.numel() == C")
    if x.dtype in H16:
        check(lib().goalnet_bn_apply_bf16_p16(x.data_ptr(), scale.data_ptr(), shift.data_ptr(), y.data_ptr(), x.numel(), C, _f16(x, y), _s()), "bn_apply_bf16_p16")
        return y
    check(lib().goalnet_bn_apply_bf16(x.data_ptr(), scale.data_ptr(), shift.data_ptr(), y.data_ptr(), x.numel(), C, _f16(y), _s()), "bn_apply_bf16")
    return y


def conv3x3_fwd_bf16(x, w, bias, relu, y, N, H, W, Cin, Cout):
    _chk(x, w, bias, y)
    _req(x.dtype in H16 and w.dtype == x.dtype and y.dtype == F32, "conv3x3_fwd_bf16: argument check failed: x.dtype in H16 and w.dtype == x.dtype and y.dtype == F32")
    _req(x.numel() == N * H * W * Cin and y.numel() == N * H * W * Cout and w.numel() == Cout * 9 * Cin, "conv3x3_fwd_bf16: argument check failed: x.numel() == N * H * W * Cin and y.numel() == N * H * W * Cout and w.numel() == Cout * 9 * Cin")
    check(lib().goalnet_conv3x3_fwd_bf16(x.data_ptr(), w.data_ptr(), _p(bias), int(relu), y.data_ptr(), N, H, W, Cin, Cout, _f16(x, w), _s()),
          "conv3x3_fwd_bf16")
    return y


def padded_bf16_alloc(N, H, W, C, device, dtype=torch.bfloat16):
    """Zeroed 16-bit buffer for a padded [N][H+2][W+2][C] tensor with its guard bands; returns (buffer, view at padded pixel 0)."""
    import ctypes as _ct
    tot, off = _ct.c_int64(), _ct.c_int64()
    check(lib().goalnet_bf16_padded_layout(N, H, W, C, _ct.byref(tot), _ct.byref(off)), "bf16_padded_layout")
    buf = torch.zeros(tot.value, dtype=dtype, device=device)
    return buf, buf[off.value:]


def to_bf16_padded(x, scale, shift, ypad, N, H, W, C):
    _chk(x, scale, shift, ypad)
    _req(x.dtype in (F32,) + H16 and ypad.dtype in H16 and x.numel() == N * H * W * C and ypad.numel() >= N * (H + 2) * (W + 2) * C, "to_bf16_padded: argument check failed: x.dtype in (F32,) + H16 and ypad.dtype in H16 and x.numel() == N * H * W * C and ypad.numel() >= N * (H + 2) * (W + 2) * C")
    if x.dtype in H16:
        check(lib().goalnet_to_bf16_padded_p16(x.data_ptr(), _p(scale), _p(shift), ypad.data_ptr(), N, H, W, C, _f16(x, ypad), _s()), "to_bf16_padded_p16")
        return ypad
    check(lib().goalnet_to_bf16_padded(x.data_ptr(), _p(scale), _p(shift), ypad.data_ptr(), N, H, W, C, _f16(ypad), _s()), "to_bf16_padded")
    return ypad


def conv3x3_fwd_bf16p(xpad, w, bias, relu, y, N, H, W, Cin, Cout):
    _chk(xpad, w, bias, y)
    _req(xpad.dtype in H16 and w.dtype == xpad.dtype and y.dtype == F32, "conv3x3_fwd_bf16p: argument check failed: xpad.dtype in H16 and w.dtype == xpad.dtype and y.dtype == F32")
    _req(y.numel() == N * H * W * Cout and w.numel() == Cout * 9 * Cin, "conv3x3_fwd_bf16p: argument check failed: y.numel() == N * H * W * Cout and w.numel() == Cout * 9 * Cin")
    nbytes = lib().goalnet_conv3x3_fwd_bf16p_ws_bytes(N, H, W, Cin, Cout)
    ws = torch.empty(nbytes // 4, dtype=F32, device=y.device) if nbytes else None
    check(lib().goalnet_conv3x3_fwd_bf16p(xpad.data_ptr(), w.data_ptr(), _p(bias), int(relu), y.data_ptr(), N, H, W, Cin, Cout,
                                          _p(ws), nbytes, _f16(xpad, w), _s()), "conv3x3_fwd_bf16p")
    return y


def conv3x3_fwd_bf16p_o16_ok(N, H, W, Cin, Cout) -> bool:
    return bool(lib().goalnet_conv3x3_fwd_bf16p_o16_ok(N, H, W, Cin, Cout))


def conv3x3_fwd_bf16p_o16(xpad, w, bias, relu, y, N, H, W, Cin, Cout):
    """bf16 result (bias None, relu False: the data gradient); only for dims conv3x3_fwd_bf16p_o16_ok accepts"""
    _chk(xpad, w, bias, y)
    _req(xpad.dtype in H16 and w.dtype == xpad.dtype and y.dtype == xpad.dtype, "conv3x3_fwd_bf16p_o16: argument check failed: xpad.dtype in H16 and w.dtype == xpad.dtype and y.dtype == xpad.dtype")
    _req(y.numel() == N * H * W * Cout and w.numel() == Cout * 9 * Cin, "conv3x3_fwd_bf16p_o16: argument check failed: y.numel() == N * H * W * Cout and w.numel() == Cout * 9 * Cin")
    check(lib().goalnet_conv3x3_fwd_bf16p_o16(xpad.data_ptr(), w.data_ptr(), _p(bias), int(relu), y.data_ptr(), N, H, W, Cin, Cout,
                                              _f16(xpad, w, y), _s()),
          "conv3x3_fwd_bf16p_o16")
    return y


def conv3x3_wgrad_bf16(xpad, dypad, dw, N, H, W, Cin, Cout):
    _chk(xpad, dypad, dw)
    _req(xpad.dtype in H16 and dypad.dtype == xpad.dtype and dw.dtype == F32 and dw.numel() == Cout * 9 * Cin, "conv3x3_wgrad_bf16: argument check failed: xpad.dtype in H16 and dypad.dtype == xpad.dtype and dw.dtype == F32 and dw.numel() == Cout * 9 * Cin")
    nbytes = lib().goalnet_conv3x3_wgrad_bf16_ws_bytes(N, H, W, Cin, Cout)
    ws = torch.empty(nbytes // 4, dtype=F32, device=dw.device)
    check(lib().goalnet_conv3x3_wgrad_bf16(xpad.data_ptr(), dypad.data_ptr(), dw.data_ptr(), ws.data_ptr(), nbytes,
                                           N, H, W, Cin, Cout, _f16(xpad, dypad), _s()), "conv3x3_wgrad_bf16")
    return dw


# ---- precision = "bf16x6" / "fp16x3" (csrc/split3.hip): fp32 operands as bf16 triples (parts = 3, six partial products per product) or
# as fp16 pairs of the power-of-two-scaled value (parts = 2, three partial products; `amax` = the tensor's magnitude word, `oscale` =
# the two operands' combined scale and its inverse for the GEMM epilogue)
def _part_dtype(parts):
    _req(parts in (2, 3), "parts must be 3 (bf16 triples) or 2 (scaled fp16 pairs)")
    return torch.bfloat16 if parts == 3 else torch.float16


def absmax(x, amax, rows, C, scale=None, shift=None, bnC=0):
    """atomic max of the bit pattern of |x * scale + shift| over a (rows, C) fp32 matrix into the int32 word `amax` (zeroed by the caller)"""
    _chk(x, amax, scale, shift)
    _req(x.dtype == F32 and amax.dtype == torch.int32 and amax.numel() == 1 and x.numel() >= rows * C, "absmax: sizes / dtypes")
    ldx = _ld(x) if x.dim() == 2 else C
    check(lib().goalnet_absmax(x.data_ptr(), ldx, _p(scale), _p(shift), bnC, rows, C, amax.data_ptr(), _s()), "absmax")
    return amax


def split_scales(amax_a, amax_b, oscale=None):
    """oscale = the exponent (int32 word on the device) the GEMM epilogue adds to undo the two operands' power-of-two scales"""
    oscale = torch.empty(1, dtype=torch.int32, device=amax_a.device) if oscale is None else oscale
    _chk(amax_a, amax_b, oscale)
    check(lib().goalnet_split_scales(amax_a.data_ptr(), amax_b.data_ptr(), oscale.data_ptr(), _s()), "split_scales")
    return oscale


def split_padded(parts, x, scale, shift, ypads, N, H, W, C, amax=None):
    """x fp32 (N,H,W,C) [* scale + shift per channel] -> interior of the zero-padded (N,H+2,W+2,parts C) 16-bit view `ypads`"""
    _chk(x, scale, shift, ypads, amax)
    _req(x.dtype == F32 and ypads.dtype == _part_dtype(parts) and x.numel() == N * H * W * C and ypads.numel() >= N * (H + 2) * (W + 2) * parts * C
         and (parts == 3 or amax is not None), "split_padded: x fp32 (N,H,W,C), ypads 16-bit (N,H+2,W+2,parts C); parts = 2 needs amax")
    check(lib().goalnet_split_padded(parts, x.data_ptr(), _p(scale), _p(shift), _p(amax), ypads.data_ptr(), N, H, W, C, _s()), "split_padded")
    return ypads


def split_rows(parts, x, ys, rows, C, scale=None, shift=None, bnC=0, amax=None):
    """x fp32 (rows, C) (row stride = x's leading dim when 2-D) [* scale + shift with channel = column % bnC] -> ys 16-bit [rows][parts C]"""
    _chk(x, ys, scale, shift, amax)
    _req(x.dtype == F32 and ys.dtype == _part_dtype(parts) and ys.numel() == parts * rows * C and (parts == 3 or amax is not None),
         "split_rows: sizes / dtypes; parts = 2 needs amax")
    ldx = _ld(x) if x.dim() == 2 else C
    _req(x.dim() == 2 and tuple(x.shape) == (rows, C) or x.numel() == rows * C, "split_rows: x must hold rows x C values")
    check(lib().goalnet_split_rows(parts, x.data_ptr(), ldx, _p(scale), _p(shift), bnC, _p(amax), ys.data_ptr(), rows, C, _s()), "split_rows")
    return ys


def linear_split_ok(parts, M, K, J) -> bool:
    return bool(lib().goalnet_linear_split_ok(parts, M, K, J))


def conv3x3_fwd_split(parts, xpads, ws, bias, relu, y, N, H, W, Cin, Cout, oscale=None):
    _chk(xpads, ws, bias, y, oscale)
    dt = _part_dtype(parts)
    _req(xpads.dtype == dt and ws.dtype == dt and y.dtype == F32 and ws.numel() == Cout * 9 * parts * Cin and y.numel() == N * H * W * Cout
         and xpads.numel() >= N * (H + 2) * (W + 2) * parts * Cin and (parts == 3 or oscale is not None), "conv3x3_fwd_split: sizes / dtypes")
    check(lib().goalnet_conv3x3_fwd_split(parts, xpads.data_ptr(), ws.data_ptr(), _p(bias), int(relu), y.data_ptr(), N, H, W, Cin, Cout, _p(oscale), _s()),
          "conv3x3_fwd_split")
    return y


def conv3x3_wgrad_split(parts, xpads, dypads, dw, N, H, W, Cin, Cout, oscale=None):
    _chk(xpads, dypads, dw, oscale)
    dt = _part_dtype(parts)
    _req(xpads.dtype == dt and dypads.dtype == dt and dw.dtype == F32 and dw.numel() == Cout * 9 * Cin and (parts == 3 or oscale is not None),
         "conv3x3_wgrad_split: sizes / dtypes")
    nbytes = lib().goalnet_conv3x3_wgrad_split_ws_bytes(parts, N, H, W, Cin, Cout)
    ws = torch.empty(nbytes // 4, dtype=F32, device=dw.device)
    check(lib().goalnet_conv3x3_wgrad_split(parts, xpads.data_ptr(), dypads.data_ptr(), dw.data_ptr(), ws.data_ptr(), nbytes, N, H, W, Cin, Cout,
                                            _p(oscale), _s()), "conv3x3_wgrad_split")
    return dw


def linear_fwd_split(parts, xs, wsp, bias, y, M, K, J, *, relu=False, dropmask=None, mult_out=None, oscale=None):
    """y (M,J view, fp32) from the split operands xs [M][parts K], wsp [J][parts K]"""
    _chk(xs, wsp, bias, y, dropmask, mult_out, oscale)
    dt = _part_dtype(parts)
    _req(xs.dtype == dt and wsp.dtype == dt and xs.numel() == parts * M * K and wsp.numel() == parts * J * K and tuple(y.shape) == (M, J)
         and (parts == 3 or oscale is not None), "linear_fwd_split: sizes / dtypes")
    nbytes = lib().goalnet_linear_fwd_split_ws_bytes(parts, M, K, J)
    _req(nbytes > 0, "linear_fwd_split: dims not served (linear_split_ok)")
    ws = torch.empty(nbytes // 4, dtype=F32, device=y.device)
    check(lib().goalnet_linear_fwd_split(parts, xs.data_ptr(), wsp.data_ptr(), _p(bias), int(relu), _p(dropmask), 0 if dropmask is None else _ld(dropmask),
                                         y.data_ptr(), _ld(y), _p(mult_out), 0 if mult_out is None else _ld(mult_out), M, K, J, ws.data_ptr(), nbytes,
                                         _p(oscale), _s()), "linear_fwd_split")
    return y


def linear_bwd_dx_split(parts, dys, wsp, dx, M, K, J, oscale=None):
    _chk(dys, wsp, dx, oscale)
    dt = _part_dtype(parts)
    _req(dys.dtype == dt and wsp.dtype == dt and dx.dtype == F32 and dys.numel() == parts * M * J and wsp.numel() == parts * J * K
         and tuple(dx.shape) == (M, K) and (parts == 3 or oscale is not None), "linear_bwd_dx_split: sizes / dtypes")
    check(lib().goalnet_linear_bwd_dx_split(parts, dys.data_ptr(), wsp.data_ptr(), dx.data_ptr(), _ld(dx), M, K, J, _p(oscale), _s()), "linear_bwd_dx_split")
    return dx


def linear_bwd_dw_split(parts, dys, xs, dw, M, K, J, oscale=None):
    _chk(dys, xs, dw, oscale)
    dt = _part_dtype(parts)
    _req(dys.dtype == dt and xs.dtype == dt and dw.dtype == F32 and dys.numel() == parts * M * J and xs.numel() == parts * M * K
         and dw.numel() == J * K and (parts == 3 or oscale is not None), "linear_bwd_dw_split: sizes / dtypes")
    check(lib().goalnet_linear_bwd_dw_split(parts, dys.data_ptr(), xs.data_ptr(), dw.data_ptr(), M, K, J, _p(oscale), _s()), "linear_bwd_dw_split")
    return dw


def linear_bwd_dx_bf16(dy, w, dx, mult=None):
    _chk(dy, w, dx, mult)
    _req(dy.dtype in H16 and w.dtype == dy.dtype and dx.dtype == F32, "linear_bwd_dx_bf16: argument check failed: dy.dtype in H16 and w.dtype == dy.dtype and dx.dtype == F32")
    M, J = dy.shape
    K = dx.shape[1]
    _req(w.numel() == J * K and dx.shape[0] == M, "linear_bwd_dx_bf16: argument check failed: w.numel() == J * K and dx.shape[0] == M")
    check(lib().goalnet_linear_bwd_dx_bf16(dy.data_ptr(), _ld(dy), w.data_ptr(), _p(mult), 0 if mult is None else _ld(mult),
                                           dx.data_ptr(), _ld(dx), M, K, J, _f16(dy, w), _s()), "linear_bwd_dx_bf16")
    return dx


def linear_bwd_dx_bf16_o16_ok(M, K, J) -> bool:
    return bool(lib().goalnet_linear_bwd_dx_bf16_o16_ok(M, K, J))


def linear_bwd_dx_bf16_o16(dy, w, dx):
    """bf16 result; only for dims linear_bwd_dx_bf16_o16_ok accepts"""
    _chk(dy, w, dx)
    _req(dy.dtype in H16 and w.dtype == dy.dtype and dx.dtype == dy.dtype, "linear_bwd_dx_bf16_o16: argument check failed: dy.dtype in H16 and w.dtype == dy.dtype and dx.dtype == dy.dtype")
    M, J = dy.shape
    K = dx.shape[1]
    _req(w.numel() == J * K and dx.shape[0] == M, "linear_bwd_dx_bf16_o16: argument check failed: w.numel() == J * K and dx.shape[0] == M")
    check(lib().goalnet_linear_bwd_dx_bf16_o16(dy.data_ptr(), _ld(dy), w.data_ptr(), dx.data_ptr(), _ld(dx), M, K, J, _f16(dy, w, dx), _s()),
          "linear_bwd_dx_bf16_o16")
    return dx


def linear_bwd_dw_bf16(dy, x, dw):
    _chk(dy, x, dw)
    _req(dy.dtype in H16 and x.dtype == dy.dtype and dw.dtype == F32, "linear_bwd_dw_bf16: argument check failed: dy.dtype in H16 and x.dtype == dy.dtype and dw.dtype == F32")
    M, J = dy.shape
    K = x.shape[1]
    _req(dw.numel() == J * K and x.shape[0] == M, "linear_bwd_dw_bf16: argument check failed: dw.numel() == J * K and x.shape[0] == M")
    check(lib().goalnet_linear_bwd_dw_bf16(dy.data_ptr(), _ld(dy), x.data_ptr(), _ld(x), dw.data_ptr(), M, K, J, _f16(dy, x), _s()), "linear_bwd_dw_bf16")
    return dw


def linear_fwd_bf16(x, w, bias, y, *, relu=False, dropmask=None, mult_out=None):
    _chk(x, w, bias, y, dropmask, mult_out)
    _req(x.dtype in H16 and w.dtype == x.dtype, "linear_fwd_bf16: argument check failed: x.dtype in H16 and w.dtype == x.dtype")
    M, K = x.shape
    J = y.shape[1]
    _req(w.numel() == J * K and y.shape[0] == M, "linear_fwd_bf16: argument check failed: w.numel() == J * K and y.shape[0] == M")
    nbytes = lib().goalnet_linear_fwd_bf16_ws_bytes(M, K, J)
    ws = torch.empty(max(nbytes // 4, 1), dtype=F32, device=x.device) if nbytes else None
    check(lib().goalnet_linear_fwd_bf16(x.data_ptr(), _ld(x), w.data_ptr(), _p(bias), int(relu), _p(dropmask),
                                        0 if dropmask is None else _ld(dropmask), y.data_ptr(), _ld(y), _p(mult_out),
                                        0 if mult_out is None else _ld(mult_out), M, K, J, _p(ws), nbytes, _f16(x, w), _s()), "linear_fwd_bf16")
    return y


def linear_fwd(x, w, bias, y, *, relu=False, scale=None, shift=None, bnC=0, dropmask=None, mult_out=None, K=None):
    """y (M,J view) = act(x (M,K view) @ w(J,K)^T + bias) * dropmask. x/y/dropmask/mult_out may be column
    slices of wider buffers (row stride = leading dim)."""
    _chk(x, w, bias, y, scale, shift, dropmask, mult_out)
    M = x.shape[0]
    K = x.shape[1] if K is None else K
    J = y.shape[1]
    _req(w.numel() == J * K and y.shape[0] == M, "linear_fwd: argument check failed: w.numel() == J * K and y.shape[0] == M")
    nbytes = lib().goalnet_linear_fwd_ws_bytes(M, K, J)
    ws = torch.empty(max(nbytes // 4, 1), dtype=F32, device=x.device) if nbytes else None
    check(lib().goalnet_linear_fwd(x.data_ptr(), _ld(x), _p(scale), _p(shift), bnC, w.data_ptr(), _p(bias), int(relu),
                                   _p(dropmask), 0 if dropmask is None else _ld(dropmask), y.data_ptr(), _ld(y),
                                   _p(mult_out), 0 if mult_out is None else _ld(mult_out), M, K, J, _p(ws), nbytes, _s()),
          "linear_fwd")
    return y


def linear_bwd_dx(dy, w, dx, mult=None):
    _chk(dy, w, dx, mult)
    M, J = dy.shape
    K = dx.shape[1]
    _req(w.numel() == J * K and dx.shape[0] == M, "linear_bwd_dx: argument check failed: w.numel() == J * K and dx.shape[0] == M")
    check(lib().goalnet_linear_bwd_dx(dy.data_ptr(), _ld(dy), w.data_ptr(), _p(mult), 0 if mult is None else _ld(mult),
                                      dx.data_ptr(), _ld(dx), M, K, J, _s()), "linear_bwd_dx")
    return dx


def linear_bwd_dw(dy, x, dw, *, scale=None, shift=None, bnC=0, db=None):
    """db (optional): bias gradient = column sums of dy, produced by the same call"""
    _chk(dy, x, dw, scale, shift, db)
    M, J = dy.shape
    K = x.shape[1]
    _req(dw.numel() == J * K and x.shape[0] == M and (db is None or db.numel() == J), "linear_bwd_dw: argument check failed: dw.numel() == J * K and x.shape[0] == M and (db is None or db.numel() == J)")
    check(lib().goalnet_linear_bwd_dw(dy.data_ptr(), _ld(dy), x.data_ptr(), _ld(x), _p(scale), _p(shift), bnC, dw.data_ptr(), _p(db),
                                      M, K, J, _s()), "linear_bwd_dw")
    return dw


def linear_bwd_dw_adam(dy, x, p, m, v, lr, beta1, beta2, eps, step, *, scale=None, shift=None, bnC=0, db=None, grad_scale=1.0, step_bias=0):
    """linear_bwd_dw + adam_step_dev on p / m / v (laid out like dw, [J][K]) in one launch, same bits; the gradient is not written.
    Rows above the weight-streaming kernels' limit only (M > 16): the C side refuses the rest."""
    _chk(dy, x, p, m, v, scale, shift, db)
    M, J = dy.shape
    K = x.shape[1]
    _req(p.numel() == J * K and m.numel() == J * K and v.numel() == J * K and x.shape[0] == M and (db is None or db.numel() == J),
         "linear_bwd_dw_adam: argument check failed: p.numel() == m.numel() == v.numel() == J * K and x.shape[0] == M and (db is None or db.numel() == J)")
    _req(p.is_contiguous() and m.is_contiguous() and v.is_contiguous(), "linear_bwd_dw_adam: p, m and v must be contiguous")
    check(lib().goalnet_linear_bwd_dw_adam(dy.data_ptr(), _ld(dy), x.data_ptr(), _ld(x), _p(scale), _p(shift), bnC, p.data_ptr(), m.data_ptr(),
                                           v.data_ptr(), _p(db), M, K, J, lr, beta1, beta2, eps, _ctr(step), int(step_bias), grad_scale, _s()),
          "linear_bwd_dw_adam")


def colsum(x, out):
    _chk(x, out)
    M, J = x.shape
    _req(out.numel() == J, "colsum: argument check failed: out.numel() == J")
    check(lib().goalnet_colsum(x.data_ptr(), _ld(x), M, J, out.data_ptr(), _s()), "colsum")
    return out


def mul(x, m, y):
    _chk(x, m, y)
    M, J = x.shape
    check(lib().goalnet_mul(x.data_ptr(), _ld(x), m.data_ptr(), _ld(m), y.data_ptr(), _ld(y), M, J, _s()), "mul")
    return y


def conv1d_fwd(x, w, b, y, relu, N, Cin, L, Cout, stride=2, pad=1):
    _chk(x, w, b, y, f64=False)
    _f32c("conv1d_fwd", x=x, w=w, b=b, y=y)
    Lo = (L + 2 * pad - 3) // stride + 1
    _req(x.numel() == N * Cin * L and y.numel() == N * Cout * Lo and w.numel() == Cout * Cin * 3, "conv1d_fwd: argument check failed: x.numel() == N * Cin * L and y.numel() == N * Cout * Lo and w.numel() == Cout * Cin * 3")
    check(lib().goalnet_conv1d_fwd(x.data_ptr(), w.data_ptr(), b.data_ptr(), int(relu), y.data_ptr(), N, Cin, L, Cout, stride, pad,
                                   _s()), "conv1d_fwd")
    return y


def conv1d_bwd(x, dz, w, dx, dw, db, N, Cin, L, Cout, stride=2, pad=1):
    _chk(x, dz, w, dx, dw, db, f64=False)
    _f32c("conv1d_bwd", x=x, dz=dz, w=w, dx=dx, dw=dw, db=db)
    Lo = (L + 2 * pad - 3) // stride + 1
    _req(x.numel() == N * Cin * L and dz.numel() == N * Cout * Lo, "conv1d_bwd: argument check failed: x.numel() == N * Cin * L and dz.numel() == N * Cout * Lo")
    _req(w.numel() == dw.numel() == Cout * Cin * 3 and db.numel() == Cout and (dx is None or dx.numel() == x.numel()), "conv1d_bwd: w / dw / db / dx shapes")
    nbytes = lib().goalnet_conv1d_bwd_ws_bytes(N, Cin, Cout)
    ws = torch.empty(nbytes // 8, dtype=torch.float64, device=x.device) if nbytes else None
    check(lib().goalnet_conv1d_bwd(x.data_ptr(), dz.data_ptr(), w.data_ptr(), _p(dx), dw.data_ptr(), db.data_ptr(), N, Cin, L, Cout,
                                   stride, pad, _p(ws), nbytes, _s()), "conv1d_bwd")


def conv1d_bwd_small_ok(N, Cin, L, Cout, stride=2, pad=1) -> bool:
    """whether conv1d_bwd_small serves the dims (N < 64, Cin <= 256, and the dz rows of a weight-gradient block fit LDS); where it
    does not, relu_bwd + conv1d_bwd compute the same layer backward in several launches"""
    return bool(lib().goalnet_conv1d_bwd_small_ok(N, Cin, L, Cout, stride, pad))


def conv1d_bwd_small(x, dz, y, w, dx, dw, db, N, Cin, L, Cout, stride=2, pad=1):
    """conv1d_bwd for N < 64 frames in one launch; y (the layer's ReLU output) gates dz when given; only for dims conv1d_bwd_small_ok accepts"""
    _chk(x, dz, y, w, dx, dw, db, f64=False)
    _f32c("conv1d_bwd_small", x=x, dz=dz, y=y, w=w, dx=dx, dw=dw, db=db)
    Lo = (L + 2 * pad - 3) // stride + 1
    _req(x.numel() == N * Cin * L and dz.numel() == N * Cout * Lo and (y is None or y.numel() == dz.numel()), "conv1d_bwd_small: x / dz / y shapes")
    _req(dw.numel() == Cout * Cin * 3 and db.numel() == Cout and (dx is None or dx.numel() == x.numel()), "conv1d_bwd_small: dw / db / dx shapes")
    check(lib().goalnet_conv1d_bwd_small(x.data_ptr(), dz.data_ptr(), _p(y), w.data_ptr(), _p(dx), dw.data_ptr(), db.data_ptr(),
                                         N, Cin, L, Cout, stride, pad, _s()), "conv1d_bwd_small")


def relu_bwd(dy, y, dz):
    _chk(dy, y, dz)
    _req(dy.is_contiguous() and y.is_contiguous() and dz.is_contiguous() and dy.numel() == y.numel() == dz.numel(), "relu_bwd: argument check failed: dy.is_contiguous() and y.is_contiguous() and dz.is_contiguous() and dy.numel() == y.numel() == dz.numel()")
    check(lib().goalnet_relu_bwd(dy.data_ptr(), y.data_ptr(), dz.data_ptr(), dy.numel(), _s()), "relu_bwd")
    return dz


MLP_WIDTHS = (512, 512, 256, 128)


def _ptrs(ts):
    return (ctypes.c_void_p * len(ts))(*[_p(t) for t in ts])


def loss_spec(kind="mse_bcast", param=None, weights_given=False, head="regression"):
    """Validate a loss selection (include/goalnet_loss.h) on the host, before any launch: -> (GOALNET_LOSS_* code, param as float).
    ValueError: an unknown name, smooth_l1's beta <= 0, weights with a loss that takes none, a non-default loss on the classifier head."""
    if kind not in _lib.LOSS_KINDS:
        raise ValueError(f"unknown loss {kind!r}: one of {', '.join(_lib.LOSS_KINDS)}")
    if kind != "mse_bcast" and head != "regression":
        raise ValueError(f"loss={kind!r} is defined for the regression head; head='classifier' trains with its cross-entropy")
    p = 0.0
    if kind == "smooth_l1":
        p = 1.0 if param is None else float(param)
        if not p > 0.0:
            raise ValueError(f"smooth_l1 needs beta > 0, got {param!r}")
    if weights_given and kind in ("mse_bcast", "rank"):
        raise ValueError(f"loss={kind!r} takes no per-frame weights")
    return _lib.LOSS_KINDS[kind], p


def _loss_weights_ok(weights, n, who):
    _req(weights is None or (torch.is_tensor(weights) and weights.dtype == F32 and weights.numel() == n and weights.is_contiguous()),
         f"{who}: weights must be a contiguous float32 tensor of {n} elements")


def frame_loss(pred, labels, loss, dpred, kind, param=None, weights=None):
    """loss (1) and dpred (n) — each optional, not both — of the named loss (loss_spec) for pred (n) against labels (n), fp32 GPU
    tensors; weights (n) for the pointwise kinds. The rank loss is O(n^2) and borrows a workspace of 24 n bytes."""
    code, p = loss_spec(kind, param, weights is not None)
    n = pred.numel()
    _req(1 <= n <= _lib.FRAME_LOSS_MAX_N, f"frame_loss: 1..{_lib.FRAME_LOSS_MAX_N} predictions")
    _loss_weights_ok(weights, n, "frame_loss")
    _req(loss is not None or dpred is not None, "frame_loss: neither loss nor dpred")
    _chk(pred, labels, loss, dpred, weights)
    _req(labels.numel() == n and pred.dtype == F32 and labels.dtype == F32 and pred.is_contiguous() and labels.is_contiguous(),
         "frame_loss: pred and labels must be contiguous float32 tensors of the same length")
    _req((loss is None or (loss.dtype == F32 and loss.numel() >= 1)) and (dpred is None or (dpred.dtype == F32 and dpred.numel() == n and dpred.is_contiguous())),
         "frame_loss: loss (1) / dpred (n) must be contiguous float32 tensors")
    nbytes = lib().goalnet_frame_loss_ws_bytes(code, n)
    ws = torch.empty(nbytes // 8, dtype=torch.float64, device=pred.device) if nbytes else None
    check(lib().goalnet_frame_loss(code, p, pred.data_ptr(), labels.data_ptr(), _p(weights), n, _p(loss), _p(dpred), _p(ws), nbytes, _s()),
          "frame_loss")


def mlp_fwd(cat, ws, bs, masks, hs, mults, logit, out, labels=None, loss=None, dout=None, *, loss_kind="mse_bcast", loss_param=None,
            weights=None):
    """fusion.0 .. fusion.12 + Sigmoid + 4y+1 on <= 16 rows in one launch. cat (n, K0) may be a view with a row stride;
    ws / bs: 5 weights / biases; masks: 4 dropout multipliers or None; hs: 4 outputs; mults: 4 saved multipliers or None.
    labels: the launch's tail evaluates the loss too — the broadcast MSE (goalnet_mlp_fwd) or the named one (goalnet_mlp_fwd_loss)."""
    code, lparam = loss_spec(loss_kind, loss_param, weights is not None)
    _chk(cat, logit, out, labels, loss, dout, weights, *ws, *bs, *masks, *hs, *mults)
    n, K0 = cat.shape
    _loss_weights_ok(weights, n, "mlp_fwd")
    _req(labels is None or (labels.numel() == n and labels.dtype == F32 and labels.is_contiguous() and loss is not None and dout is not None
                            and dout.numel() == n), "mlp_fwd: labels (n) need loss (1) and dout (n)")
    _req(len(ws) == 5 and len(bs) == 5 and len(masks) == 4 and len(hs) == 4 and len(mults) == 4, "mlp_fwd: 5 layers, 4 hidden outputs")
    for l, wd in enumerate(MLP_WIDTHS):
        kin = K0 if l == 0 else MLP_WIDTHS[l - 1]
        _req(ws[l].numel() == wd * kin and bs[l].numel() == wd and hs[l].shape == (n, wd) and hs[l].is_contiguous(), f"mlp_fwd: layer {l} shapes")
        _req(masks[l] is None or masks[l].shape == (n, wd), f"mlp_fwd: mask {l} shape")
        _req(mults[l] is None or (mults[l].shape == (n, wd) and mults[l].is_contiguous()), f"mlp_fwd: mult {l} shape")
    _req(ws[4].numel() == 128 and bs[4].numel() == 1 and logit.numel() == n and out.numel() == n, "mlp_fwd: head shapes")
    ldm = (ctypes.c_int64 * 4)(*[0 if m is None else _ld(m) for m in masks])
    sync = _tile_counters(("mlp_fwd", n, K0), cat.device)
    if loss_kind == "mse_bcast":
        check(lib().goalnet_mlp_fwd(cat.data_ptr(), _ld(cat), K0, _ptrs(ws), _ptrs(bs), _ptrs(masks), ldm, _ptrs(hs), _ptrs(mults),
                                    logit.data_ptr(), out.data_ptr(), _p(labels), _p(loss), _p(dout), n, sync.data_ptr(), _s()), "mlp_fwd")
        return
    check(lib().goalnet_mlp_fwd_loss(cat.data_ptr(), _ld(cat), K0, _ptrs(ws), _ptrs(bs), _ptrs(masks), ldm, _ptrs(hs), _ptrs(mults),
                                     logit.data_ptr(), out.data_ptr(), _p(labels), _p(loss), _p(dout), code, lparam, _p(weights), n,
                                     sync.data_ptr(), _s()), "mlp_fwd_loss")


def mlp_bwd(dout, out, xs, ms, ws, dws, dbs, dcat, db5, voff):
    """backward of mlp_fwd in one launch. xs: cat (view), h1..h4; ms: mcat (view), mult1..4; dws / dbs: 5 gradient slots;
    dcat (n, K0) contiguous; db5 (K0 - voff) or None."""
    _chk(dout, out, dcat, db5, *xs, *ms, *ws, *dws, *dbs)
    n, K0 = xs[0].shape
    _req(len(xs) == 5 and len(ms) == 5 and len(ws) == 5 and len(dws) == 5 and len(dbs) == 5, "mlp_bwd: 5 layers")
    _req(dout.numel() == n and out.numel() == n and dout.is_contiguous() and out.is_contiguous(), "mlp_bwd: dout / out (n)")
    _req(dcat.shape == (n, K0) and dcat.is_contiguous() and (db5 is None or db5.numel() == K0 - voff), "mlp_bwd: dcat (n, K0), db5 (K0 - voff)")
    for l in range(1, 5):
        _req(xs[l].shape == (n, MLP_WIDTHS[l - 1]) and xs[l].is_contiguous() and (ms[l] is None or (ms[l].shape == xs[l].shape and ms[l].is_contiguous())),
             f"mlp_bwd: layer {l} input / multiplier shapes")
    for l in range(5):
        _req(dws[l].numel() == ws[l].numel() and dws[l].is_contiguous() and dbs[l].is_contiguous(), f"mlp_bwd: layer {l} gradient slots")
    nbytes = lib().goalnet_mlp_bwd_ws_bytes(n)
    wsb = torch.empty(nbytes // 4, dtype=F32, device=dout.device)
    sync = _tile_counters(("mlp_bwd", n, K0), dout.device)
    check(lib().goalnet_mlp_bwd(dout.data_ptr(), out.data_ptr(), _ptrs(xs), _ld(xs[0]), _ptrs(ms), 0 if ms[0] is None else _ld(ms[0]),
                                _ptrs(ws), _ptrs(dws), _ptrs(dbs), dcat.data_ptr(), _ld(dcat), _p(db5), voff, n, K0, wsb.data_ptr(), nbytes,
                                sync.data_ptr(), _s()), "mlp_bwd")


def mlp_sync_error(device, n, K0) -> bool:
    """True when a grid barrier of the fused MLP kernels timed out on this device (one host read-back; tests)"""
    bad = False
    for name in ("mlp_fwd", "mlp_bwd"):
        t = _TILE_CTR.get(((name, n, K0), device.index))
        bad = bad or (t is not None and bool(t[2].item() != 0))
    return bad


def head_fwd(h, w, b, logit, out):
    _chk(h, w, b, logit, out)
    N, K = h.shape
    check(lib().goalnet_head_fwd(h.data_ptr(), _ld(h), w.data_ptr(), b.data_ptr(), _p(logit), out.data_ptr(), N, K, _s()), "head_fwd")


def head_bwd(dout, out, h, w, mult, dh, dw, db):
    _chk(dout, out, h, w, mult, dh, dw, db)
    N, K = h.shape
    _req(dout.numel() == N and out.numel() == N and dout.is_contiguous() and out.is_contiguous(), "head_bwd: argument check failed: dout.numel() == N and out.numel() == N and dout.is_contiguous() and out.is_contiguous()")
    check(lib().goalnet_head_bwd(dout.data_ptr(), out.data_ptr(), h.data_ptr(), _ld(h), w.data_ptr(), _p(mult),
                                 0 if mult is None else _ld(mult), dh.data_ptr(), _ld(dh), dw.data_ptr(), db.data_ptr(), N, K, _s()),
          "head_bwd")


def cls_head_fwd(h, w, b, logits, scores):
    """classifier-head extension: scores (N, C) = 4 softmax(h w^T + b) + 1"""
    _chk(h, w, b, logits, scores)
    N, K = h.shape
    C = scores.shape[1]
    _req(w.numel() == C * K and b.numel() == C and scores.is_contiguous() and (logits is None or logits.is_contiguous()), "cls_head_fwd: argument check failed: w.numel() == C * K and b.numel() == C and scores.is_contiguous() and (logits is None or logits.is_contiguous())")
    check(lib().goalnet_cls_head_fwd(h.data_ptr(), _ld(h), w.data_ptr(), b.data_ptr(), _p(logits), scores.data_ptr(), N, K, C, _s()), "cls_head_fwd")


def cross_entropy(scores, labels, loss, dscores):
    """nn.CrossEntropyLoss()(scores, (labels - 1).long()) and its gradient wrt scores"""
    _chk(scores, labels, loss, dscores, f64=False)
    _f32c("cross_entropy", scores=scores, labels=labels, loss=loss, dscores=dscores)
    N, C = scores.shape
    _req(labels.numel() == N and scores.is_contiguous() and (dscores is None or dscores.is_contiguous()), "cross_entropy: argument check failed: labels.numel() == N and scores.is_contiguous() and (dscores is None or dscores.is_contiguous())")
    check(lib().goalnet_cross_entropy(scores.data_ptr(), labels.data_ptr(), _p(loss), _p(dscores), N, C, _s()), "cross_entropy")


def cls_head_bwd(dscores, scores, h, w, mult, dh, dw, db):
    _chk(dscores, scores, h, w, mult, dh, dw, db)
    N, K = h.shape
    C = scores.shape[1]
    _req(dscores.is_contiguous() and scores.is_contiguous() and dw.numel() == C * K and db.numel() == C, "cls_head_bwd: argument check failed: dscores.is_contiguous() and scores.is_contiguous() and dw.numel() == C * K and db.numel() == C")
    check(lib().goalnet_cls_head_bwd(dscores.data_ptr(), scores.data_ptr(), h.data_ptr(), _ld(h), w.data_ptr(), _p(mult),
                                     0 if mult is None else _ld(mult), dh.data_ptr(), _ld(dh), dw.data_ptr(), db.data_ptr(), N, K, C, _s()),
          "cls_head_bwd")


def argmax_plus1(scores, classes):
    _chk(scores, classes)
    N, C = scores.shape
    _req(classes.numel() == N and scores.is_contiguous(), "argmax_plus1: argument check failed: classes.numel() == N and scores.is_contiguous()")
    check(lib().goalnet_argmax_plus1(scores.data_ptr(), classes.data_ptr(), N, C, _s()), "argmax_plus1")
    return classes


def mse_bcast(pred, labels, loss, dpred):
    _chk(pred, labels, loss, dpred, f64=False)
    _f32c("mse_bcast", pred=pred, labels=labels, loss=loss, dpred=dpred)
    N = pred.numel()
    _req(labels.numel() == N, "mse_bcast: argument check failed: labels.numel() == N")
    check(lib().goalnet_mse_bcast(pred.data_ptr(), labels.data_ptr(), N, _p(loss), _p(dpred), _s()), "mse_bcast")


def adam_step(p, g, m, v, lr, beta1, beta2, eps, step, grad_scale=1.0):
    _chk(p, g, m, v)
    n = p.numel()
    _req(g.numel() == n and m.numel() == n and v.numel() == n, "adam_step: argument check failed: g.numel() == n and m.numel() == n and v.numel() == n")
    check(lib().goalnet_adam_step(p.data_ptr(), g.data_ptr(), m.data_ptr(), v.data_ptr(), n, lr, beta1, beta2, eps, step, grad_scale,
                                  _s()), "adam_step")


# ---- device-resident step state (graph-capturable variants; include/goalnet_hip.h "device-resident step state") ----
I64 = torch.int64


def _ctr(t):
    _req(t.is_cuda and t.dtype == I64 and t.numel() == 1, "_ctr: argument check failed: t.is_cuda and t.dtype == I64 and t.numel() == 1")
    return t.data_ptr()


def counter_add(counter, delta):
    check(lib().goalnet_counter_add(_ctr(counter), int(delta), _s()), "counter_add")


def dropout_masks_dev(dst, n, widths, seed, tid_base, tid_stride, step, p, row_offset=0):
    """dst: flat fp32 buffer of n*sum(widths); returns the per-layer (n, width) views. row_offset: the masks are rows
    [row_offset, row_offset + n) of the (row_offset + n, width) masks the same stream yields (data-parallel shards)."""
    _chk(dst)
    total = n * sum(widths)
    _req(dst.is_contiguous() and dst.dtype == F32 and dst.numel() == total, "dropout_masks_dev: argument check failed: dst.is_contiguous() and dst.dtype == F32 and dst.numel() == total")
    arr = (ctypes.c_int * len(widths))(*widths)
    check(lib().goalnet_dropout_masks_dev(dst.data_ptr(), n, arr, len(widths), seed, tid_base, tid_stride, _ctr(step), p, int(row_offset), _s()),
          "dropout_masks_dev")
    out, off = [], 0
    for wdt in widths:
        out.append(dst[off:off + n * wdt].view(n, wdt))
        off += n * wdt
    return out


def counters_add4(counters, d0, d1, d2, d3):
    _req(counters.is_cuda and counters.dtype == I64 and counters.numel() == 4 and counters.is_contiguous(), "counters_add4: argument check failed: counters.is_cuda and counters.dtype == I64 and counters.numel() == 4 and counters.is_contiguous()")
    check(lib().goalnet_counters_add4(counters.data_ptr(), int(d0), int(d1), int(d2), int(d3), _s()), "counters_add4")


def counters_add4_guarded(counters, d0, d1, d2, d3, bad_step):
    """counters_add4 of a precision="fp16" step: the step count stays where it is when this step's Adam was skipped"""
    _req(counters.is_cuda and counters.dtype == I64 and counters.numel() == 4 and counters.is_contiguous(), "counters_add4_guarded: argument check failed: counters.is_cuda and counters.dtype == I64 and counters.numel() == 4 and counters.is_contiguous()")
    check(lib().goalnet_counters_add4_guarded(counters.data_ptr(), int(d0), int(d1), int(d2), int(d3), _ctr(bad_step), _s()), "counters_add4_guarded")


def adam_step_dev(p, g, m, v, lr, beta1, beta2, eps, step, grad_scale=1.0, step_bias=0):
    """Adam with the 1-based step count = *step + step_bias"""
    _chk(p, g, m, v)
    n = p.numel()
    _req(g.numel() == n and m.numel() == n and v.numel() == n, "adam_step_dev: argument check failed: g.numel() == n and m.numel() == n and v.numel() == n")
    check(lib().goalnet_adam_step_dev(p.data_ptr(), g.data_ptr(), m.data_ptr(), v.data_ptr(), n, lr, beta1, beta2, eps, _ctr(step),
                                      int(step_bias), grad_scale, _s()), "adam_step_dev")


def adam_step_dev_blocks(p, g, m, v, lr, beta1, beta2, eps, step, grad_scale=1.0, step_bias=0, max_blocks=128):
    """adam_step_dev as a background pass on at most max_blocks blocks"""
    _chk(p, g, m, v)
    n = p.numel()
    _req(g.numel() == n and m.numel() == n and v.numel() == n, "adam_step_dev_blocks: p, g, m, v must have the same size")
    check(lib().goalnet_adam_step_dev_blocks(p.data_ptr(), g.data_ptr(), m.data_ptr(), v.data_ptr(), n, lr, beta1, beta2, eps, _ctr(step),
                                             int(step_bias), grad_scale, int(max_blocks), _s()), "adam_step_dev_blocks")


def adam_step_dev_shadow(p, g, m, v, lr, beta1, beta2, eps, step, shadow, shadow_begin, grad_scale=1.0, step_bias=0):
    """adam_step_dev that also writes bf16(p_new) of arena[shadow_begin : shadow_begin + shadow.numel()] into `shadow`"""
    _chk(p, g, m, v, shadow)
    n = p.numel()
    _req(g.numel() == n and m.numel() == n and v.numel() == n and shadow.dtype in H16 and shadow.is_contiguous(), "adam_step_dev_shadow: argument check failed: g.numel() == n and m.numel() == n and v.numel() == n and shadow.dtype in H16 and shadow.is_contiguous()")
    check(lib().goalnet_adam_step_dev_shadow(p.data_ptr(), g.data_ptr(), m.data_ptr(), v.data_ptr(), n, lr, beta1, beta2, eps, _ctr(step),
                                             int(step_bias), grad_scale, shadow.data_ptr(), int(shadow_begin), shadow.numel(), _f16(shadow), _s()),
          "adam_step_dev_shadow")


def adam_step_dev_guarded(p, g, m, v, lr, beta1, beta2, eps, step, bad_step, shadow=None, shadow_begin=0, grad_scale=1.0, step_bias=0):
    """precision="fp16": adam_step_dev[_shadow] that leaves everything untouched when grad_finite_check stamped this step"""
    _chk(p, g, m, v, shadow)
    n = p.numel()
    _req(g.numel() == n and m.numel() == n and v.numel() == n and (shadow is None or (shadow.dtype in H16 and shadow.is_contiguous())), "adam_step_dev_guarded: argument check failed: g.numel() == n and m.numel() == n and v.numel() == n and (shadow is None or (shadow.dtype in H16 and shadow.is_contiguous()))")
    check(lib().goalnet_adam_step_dev_guarded(p.data_ptr(), g.data_ptr(), m.data_ptr(), v.data_ptr(), n, lr, beta1, beta2, eps, _ctr(step),
                                              int(step_bias), grad_scale, _p(shadow), int(shadow_begin), 0 if shadow is None else shadow.numel(),
                                              0 if shadow is None else _f16(shadow), _ctr(bad_step), _s()), "adam_step_dev_guarded")


def _ranges(who, ranges, n, struct):
    """[(begin, count[, skipped[, decay[, group]]])] inside an arena of n elements -> struct[]; the fields a tuple leaves out are 0"""
    _req(1 <= len(ranges) <= _lib.ADAM_RANGES_MAX, f"{who}: 1..{_lib.ADAM_RANGES_MAX} ranges")
    _req(all(r[0] >= 0 and r[1] > 0 and r[0] + r[1] <= n for r in ranges), f"{who}: a range leaves the arena")
    rows = [[int(bool(x)) if i == 3 else int(x) for i, x in enumerate(r)] for r in ranges]          # field 3, `decay`, is a flag
    return (struct * len(rows))(*[struct(*f) for f in rows])


def _shadow_tail(who, shadow, shadow_begin, n, bad_step):
    """the checked last arguments of the update launches over ranges: (shadow, begin, count, f16, bad_step, stream)"""
    _req(shadow is None or (shadow.dtype in H16 and shadow.is_contiguous() and shadow_begin + shadow.numel() <= n),
         f"{who}: shadow must be a contiguous 16-bit tensor for a slice inside the arena")
    return (_p(shadow), int(shadow_begin), 0 if shadow is None else shadow.numel(), 0 if shadow is None else _f16(shadow),
            0 if bad_step is None else _ctr(bad_step), _s())


def adam_step_dev_ranges(p, g, m, v, ranges, lr, beta1, beta2, eps, step, grad_scale=1.0, shadow=None, shadow_begin=0, bad_step=None):
    """adam_step_dev[_guarded] over `ranges` = [(begin, count, skipped)] of the arenas p, g, m, v in ONE launch; a range's 1-based step
    count is *step + 1 - skipped. `shadow` (16-bit) receives the updated arena[shadow_begin : shadow_begin + shadow.numel()]."""
    _chk(p, g, m, v, shadow)
    n = p.numel()
    _req(g.numel() == n and m.numel() == n and v.numel() == n, "adam_step_dev_ranges: p, g, m, v must have the same size")
    arr = _ranges("adam_step_dev_ranges", ranges, n, _lib.AdamRange)
    tail = _shadow_tail("adam_step_dev_ranges", shadow, shadow_begin, n, bad_step)
    check(lib().goalnet_adam_step_dev_ranges(p.data_ptr(), g.data_ptr(), m.data_ptr(), v.data_ptr(), arr, len(ranges), lr, beta1, beta2, eps,
                                             _ctr(step), grad_scale, *tail), "adam_step_dev_ranges")


# ---- optimizer options on the fused step (include/goalnet_optim.h) ----
def _optim_opts(lr, beta1, beta2, eps, optim):
    """the host structure of one launch: base rate and betas of the call, everything else from the OptimOptions"""
    return _lib.OptimOpts(float(lr), float(beta1), float(beta2), float(eps), float(optim.weight_decay),
                          0.0 if optim.max_grad_norm is None else float(optim.max_grad_norm), float(optim.min_lr), float(optim.gamma),
                          int(optim.warmup_steps), int(optim.total_steps or 0), int(optim.step_period or 0), int(optim.decoupled),
                          _lib.SCHEDULES[optim.schedule])


def grad_sumsq(g, ranges, out=None):
    """sum of g[i]^2 over `ranges` = [(begin, count, skipped, decay)] of the gradient arena, in fp64, into out (1,) float64: two launches,
    fixed shares and a fixed order, so the same data gives the same bits"""
    _chk(g, out)
    _req(g.dtype == F32 and g.is_contiguous(), "grad_sumsq: g must be a contiguous fp32 arena")
    arr = _ranges("grad_sumsq", ranges, g.numel(), _lib.OptimRange)
    if out is None:
        out = torch.empty(1, dtype=torch.float64, device=g.device)
    _req(out.dtype == torch.float64 and out.numel() == 1, "grad_sumsq: out must be one float64")
    nbytes = lib().goalnet_grad_sumsq_ws_bytes(arr, len(ranges))
    _req(nbytes > 0, "grad_sumsq: the ranges must be sorted, disjoint and begin at multiples of 4")
    ws = torch.empty(nbytes // 8, dtype=torch.float64, device=g.device)
    check(lib().goalnet_grad_sumsq(g.data_ptr(), arr, len(ranges), out.data_ptr(), ws.data_ptr(), nbytes, _s()), "grad_sumsq")
    return out


def optim_step_dev_ranges(p, g, m, v, ranges, lr, beta1, beta2, eps, optim, step, grad_scale=1.0, sumsq=None, shadow=None, shadow_begin=0,
                          bad_step=None):
    """adam_step_dev_ranges under `optim` (optim.OptimOptions) over `ranges` = [(begin, count, skipped, decay)] in ONE launch: the rate
    of the schedule at *step, the clip coefficient from `sumsq` (grad_sumsq; required iff optim.max_grad_norm is set), weight decay
    on the ranges flagged `decay`. Without any of them it is adam_step_dev_ranges, bit for bit."""
    _chk(p, g, m, v, shadow, sumsq)
    n = p.numel()
    _req(g.numel() == n and m.numel() == n and v.numel() == n, "optim_step_dev_ranges: p, g, m, v must have the same size")
    arr = _ranges("optim_step_dev_ranges", ranges, n, _lib.OptimRange)
    _req((sumsq is None) == (optim.max_grad_norm is None), "optim_step_dev_ranges: sumsq goes with max_grad_norm, and only with it")
    _req(sumsq is None or (sumsq.dtype == torch.float64 and sumsq.numel() == 1), "optim_step_dev_ranges: sumsq must be one float64")
    tail = _shadow_tail("optim_step_dev_ranges", shadow, shadow_begin, n, bad_step)
    opts = _optim_opts(lr, beta1, beta2, eps, optim)
    check(lib().goalnet_optim_step_dev_ranges(p.data_ptr(), g.data_ptr(), m.data_ptr(), v.data_ptr(), arr, len(ranges), ctypes.byref(opts),
                                              _ctr(step), grad_scale, _p(sumsq), *tail), "optim_step_dev_ranges")


def optim_lr(lr, optim, step, out=None):
    """the learning rate of the step that starts from *step completed steps, as the device evaluates it, into out (1,) float64"""
    _chk(out)
    if out is None:
        out = torch.empty(1, dtype=torch.float64, device=step.device)
    _req(out.dtype == torch.float64 and out.numel() == 1, "optim_lr: out must be one float64")
    opts = _optim_opts(lr, 0.9, 0.999, 1e-8, optim)
    check(lib().goalnet_optim_lr(ctypes.byref(opts), _ctr(step), out.data_ptr(), _s()), "optim_lr")
    return out


# ---- parameter groups and AMSGrad on the fused step (include/goalnet_groups.h) ----
GROUPS_MAX = _lib.GROUPS_MAX               # rows of one launch's hyper-parameter table, the default group included


def _group_table(who, table):
    """[(lr, beta1, beta2, eps, weight_decay, amsgrad)] -> goalnet_group_hyper[]"""
    _req(1 <= len(table) <= GROUPS_MAX, f"{who}: 1..{GROUPS_MAX} groups")
    return (_lib.GroupHyper * len(table))(*[_lib.GroupHyper(float(lr), float(b1), float(b2), float(eps), float(wd), int(bool(ams)), 0)
                                            for lr, b1, b2, eps, wd, ams in table])


def group_step_dev_ranges(p, g, m, v, vmax, ranges, table, optim, step, grad_scale=1.0, sumsq=None, shadow=None, shadow_begin=0,
                          bad_step=None):
    """optim_step_dev_ranges over `ranges` = [(begin, count, skipped, decay, group)] in ONE launch, every range under its row of `table` =
    [(lr, beta1, beta2, eps, weight_decay, amsgrad)] (optim.OptimOptions.hyper_table): schedule, clipping and `decoupled` come from
    `optim`, rate, betas, eps, decay value and AMSGrad from the row. `vmax`: the running maximum of v, required iff a referenced row
    has amsgrad. A row with the single-rate call's values and no AMSGrad gives optim_step_dev_ranges' bits."""
    _chk(p, g, m, v, vmax, shadow, sumsq)
    n = p.numel()
    _req(g.numel() == n and m.numel() == n and v.numel() == n, "group_step_dev_ranges: p, g, m, v must have the same size")
    _req(vmax is None or (vmax.dtype == F32 and vmax.is_contiguous() and vmax.numel() == n),
         "group_step_dev_ranges: vmax must be a contiguous fp32 arena of the size of v")
    arr = _ranges("group_step_dev_ranges", ranges, n, _lib.GroupRange)
    tab = _group_table("group_step_dev_ranges", table)
    _req((sumsq is None) == (optim.max_grad_norm is None), "group_step_dev_ranges: sumsq goes with max_grad_norm, and only with it")
    _req(sumsq is None or (sumsq.dtype == torch.float64 and sumsq.numel() == 1), "group_step_dev_ranges: sumsq must be one float64")
    tail = _shadow_tail("group_step_dev_ranges", shadow, shadow_begin, n, bad_step)
    opts = _optim_opts(table[0][0], table[0][1], table[0][2], table[0][3], optim)
    check(lib().goalnet_group_step_dev_ranges(p.data_ptr(), g.data_ptr(), m.data_ptr(), v.data_ptr(), _p(vmax), arr, len(ranges), tab,
                                              len(table), ctypes.byref(opts), _ctr(step), grad_scale, _p(sumsq), *tail), "group_step_dev_ranges")


def group_lr(table, group, optim, step, out=None):
    """the learning rate of row `group` of `table` for the step that starts from *step completed steps, as the device evaluates it,
    into out (1,) float64"""
    _chk(out)
    if out is None:
        out = torch.empty(1, dtype=torch.float64, device=step.device)
    _req(out.dtype == torch.float64 and out.numel() == 1, "group_lr: out must be one float64")
    tab = _group_table("group_lr", table)
    _req(0 <= int(group) < len(table), "group_lr: no such group")
    opts = _optim_opts(table[0][0], table[0][1], table[0][2], table[0][3], optim)
    check(lib().goalnet_group_lr(ctypes.byref(opts), tab, int(group), _ctr(step), out.data_ptr(), _s()), "group_lr")
    return out


# ---- the weight average behind the fused step (include/goalnet_ema.h) ----
# ranges = [(begin, count)] or [(begin, count, skipped)]: these passes do not read the count of sat-out steps, and it is not handed on
def ema_update_dev_ranges(p, e, ranges, ema, step, step_bias=1, bad_step=None):
    """the average `e` of the weights `p` over `ranges` in ONE launch, under `ema` (optim.EmaOptions) at the 1-based step count
    t = *step + step_bias: a copy up to ema.start_step, then every ema.every-th step e += w (p - e) with w = ema.weight_at(t); a step
    that `bad_step` stamps leaves e alone."""
    _chk(p, e)
    n = p.numel()
    _req(p.dtype == F32 and e.dtype == F32 and p.is_contiguous() and e.is_contiguous() and e.numel() == n,
         "ema_update_dev_ranges: p and e must be contiguous fp32 arenas of one size")
    arr = _ranges("ema_update_dev_ranges", [r[:2] for r in ranges], n, _lib.AdamRange)
    opts = _lib.EmaOpts(float(ema.decay), int(ema.every), int(ema.start_step), int(bool(ema.warmup)), 0)
    check(lib().goalnet_ema_update_dev_ranges(p.data_ptr(), e.data_ptr(), arr, len(ranges), ctypes.byref(opts), _ctr(step), int(step_bias),
                                              0 if bad_step is None else _ctr(bad_step), _s()), "ema_update_dev_ranges")


def swap_ranges(a, b, ranges):
    """a[i] <-> b[i] over `ranges` in ONE launch, bit for bit"""
    _chk(a, b)
    n = a.numel()
    _req(a.dtype == F32 and b.dtype == F32 and a.is_contiguous() and b.is_contiguous() and b.numel() == n,
         "swap_ranges: a and b must be contiguous fp32 arenas of one size")
    arr = _ranges("swap_ranges", [r[:2] for r in ranges], n, _lib.AdamRange)
    check(lib().goalnet_swap_ranges(a.data_ptr(), b.data_ptr(), arr, len(ranges), _s()), "swap_ranges")


# ---- gradient accumulation over a window of micro-steps (include/goalnet_accum.h) ----
def grad_accum_dev_ranges(acc, g, ranges, scale, first):
    """acc = g * scale (`first`: acc is not read) or acc = acc + g * scale over `ranges` in ONE launch; the product and the sum are
    rounded separately in fp32, as the two torch operations `t = g * scale; acc + t` are."""
    _chk(acc, g)
    n = g.numel()
    _req(acc.dtype == F32 and g.dtype == F32 and acc.is_contiguous() and g.is_contiguous() and acc.numel() == n,
         "grad_accum_dev_ranges: acc and g must be contiguous fp32 arenas of one size")
    arr = _ranges("grad_accum_dev_ranges", [r[:2] for r in ranges], n, _lib.AdamRange)
    check(lib().goalnet_grad_accum_dev_ranges(acc.data_ptr(), g.data_ptr(), arr, len(ranges), float(scale), int(bool(first)), _s()),
          "grad_accum_dev_ranges")


def scale_(x, s):
    _chk(x)
    _req(x.dtype == F32 and x.is_contiguous(), "scale_: argument check failed: x.dtype == F32 and x.is_contiguous()")
    check(lib().goalnet_scale(x.data_ptr(), x.numel(), float(s), _s()), "scale")
    return x


def grad_finite_check(g, step, bad_step, skipped, step_bias=1):
    _chk(g)
    _req(g.dtype == F32 and g.is_contiguous(), "grad_finite_check: argument check failed: g.dtype == F32 and g.is_contiguous()")
    check(lib().goalnet_grad_finite_check(g.data_ptr(), g.numel(), _ctr(step), int(step_bias), _ctr(bad_step), _ctr(skipped), _s()), "grad_finite_check")


def rows_copy_batch(segments):
    """segments: up to 4 of (table, block, nrows, cursor, cursor_bias, gather); rows [cursor + bias, +nrows) of `table`
    are read into (gather) or written from (scatter) `block`. One launch."""
    arr = (_lib.RowCopy * len(segments))()
    for k, (table, block, nrows, cursor, bias, gather) in enumerate(segments):
        _chk(table, block)
        _req(table.is_contiguous() and block.is_contiguous() and table.dtype == block.dtype, "rows_copy_batch: argument check failed: table.is_contiguous() and block.is_contiguous() and table.dtype == block.dtype")
        row_bytes = table[0].numel() * table.element_size() if table.dim() > 1 else table.element_size()
        _req(block.numel() * block.element_size() == row_bytes * nrows, "rows_copy_batch: argument check failed: block.numel() * block.element_size() == row_bytes * nrows")
        src, dst = (table, block) if gather else (block, table)
        arr[k] = _lib.RowCopy(src.data_ptr(), dst.data_ptr(), row_bytes, nrows, 1 if gather else 0, _ctr(cursor), int(bias))
    check(lib().goalnet_rows_copy_batch(arr, len(segments), _s()), "rows_copy_batch")


def rows_scatter_tick(segments, counters, d0, d1, d2, d3, bad_step=None):
    """rows_copy_batch(segments) followed by counters_add4[_guarded] in ONE launch (the segments are small)"""
    arr = (_lib.RowCopy * len(segments))()
    for k, (table, block, nrows, cursor, bias, gather) in enumerate(segments):
        _chk(table, block)
        _req(table.is_contiguous() and block.is_contiguous() and table.dtype == block.dtype, "rows_scatter_tick: contiguous tensors of one dtype")
        row_bytes = table[0].numel() * table.element_size() if table.dim() > 1 else table.element_size()
        _req(block.numel() * block.element_size() == row_bytes * nrows, "rows_scatter_tick: block size")
        src, dst = (table, block) if gather else (block, table)
        arr[k] = _lib.RowCopy(src.data_ptr(), dst.data_ptr(), row_bytes, nrows, 1 if gather else 0, _ctr(cursor), int(bias))
    _req(counters.is_cuda and counters.dtype == I64 and counters.numel() == 4 and counters.is_contiguous(), "rows_scatter_tick: int64[4] counters")
    check(lib().goalnet_rows_scatter_tick(arr, len(segments), counters.data_ptr(), int(d0), int(d1), int(d2), int(d3),
                                          0 if bad_step is None else _ctr(bad_step), _s()), "rows_scatter_tick")


def rows_gather(table, block, nrows, cursor):
    """block[0:nrows] = table[cursor : cursor + nrows]; rows are the leading dimension of contiguous tensors."""
    _chk(table, block)
    _req(table.is_contiguous() and block.is_contiguous() and table.dtype == block.dtype, "rows_gather: argument check failed: table.is_contiguous() and block.is_contiguous() and table.dtype == block.dtype")
    row_bytes = table[0].numel() * table.element_size() if table.dim() > 1 else table.element_size()
    _req(block.numel() * block.element_size() == row_bytes * nrows, "rows_gather: argument check failed: block.numel() * block.element_size() == row_bytes * nrows")
    check(lib().goalnet_rows_gather(table.data_ptr(), block.data_ptr(), row_bytes, nrows, _ctr(cursor), _s()), "rows_gather")


def rows_scatter(block, table, nrows, cursor):
    """table[cursor : cursor + nrows] = block[0:nrows]"""
    _chk(table, block)
    _req(table.is_contiguous() and block.is_contiguous() and table.dtype == block.dtype, "rows_scatter: argument check failed: table.is_contiguous() and block.is_contiguous() and table.dtype == block.dtype")
    row_bytes = table[0].numel() * table.element_size() if table.dim() > 1 else table.element_size()
    _req(block.numel() * block.element_size() == row_bytes * nrows, "rows_scatter: argument check failed: block.numel() * block.element_size() == row_bytes * nrows")
    check(lib().goalnet_rows_scatter(block.data_ptr(), table.data_ptr(), row_bytes, nrows, _ctr(cursor), _s()), "rows_scatter")


# ---- shuffled, augmented passes over a resident video (include/goalnet_epoch.h, csrc/epoch.hip) ----------
I32 = torch.int32


def augment_spec(flip_p=0.0, max_shift=0, contrast=0.0, brightness=0.0):
    """(flip_p, max_shift, contrast, brightness) as goalnet_epoch_plan takes them — ValueError on a value outside its range, before
    any launch and without a GPU. The three floats are rounded to fp32 here: that is what the draws are defined on."""
    if isinstance(max_shift, bool) or not isinstance(max_shift, int) or not 0 <= max_shift <= _lib.MAX_SHIFT:
        raise ValueError(f"max_shift must be an integer in [0, {_lib.MAX_SHIFT}], got {max_shift!r}")
    out = []
    for name, v, ok in (("flip_p", flip_p, lambda f: 0.0 <= f <= 1.0), ("contrast", contrast, lambda f: 0.0 <= f < 1.0),
                        ("brightness", brightness, lambda f: 0.0 <= f < float("inf"))):
        try:
            f = ctypes.c_float(float(v)).value
        except (TypeError, ValueError):
            raise ValueError(f"{name} must be a number, got {v!r}") from None
        if not ok(f):                                   # NaN fails every comparison
            raise ValueError(f"{name} = {v!r} is outside its range")
        out.append(f)
    return out[0], max_shift, out[1], out[2]


def _plan_ok(plan, who):
    _req(torch.is_tensor(plan) and plan.is_cuda and plan.dtype == I32 and plan.dim() == 2 and plan.shape[1] == _lib.PLAN_WORDS
         and plan.is_contiguous() and plan.shape[0] >= 1, f"{who}: the plan must be a contiguous int32 (n, {_lib.PLAN_WORDS}) GPU tensor")


def epoch_plan(plan, n, seed, index, shuffle=False, flip_p=0.0, max_shift=0, contrast=0.0, brightness=0.0):
    """rows [0, n) of `plan` (int32 (>= n, 8)) = the plan of pass `index`: {src, flip, dx, dy, gain, bias, 0, 0} per consumed frame"""
    flip_p, max_shift, contrast, brightness = augment_spec(flip_p, max_shift, contrast, brightness)
    if not 1 <= n <= _lib.EPOCH_MAX_N:
        raise ValueError(f"a pass takes 1..{_lib.EPOCH_MAX_N} frames, got {n}")
    if not 0 <= index < (1 << 28):
        raise ValueError(f"pass index must be in [0, 2^28), got {index}")
    _plan_ok(plan, "epoch_plan")
    _req(plan.shape[0] >= n, "epoch_plan: the plan table is shorter than the pass")
    check(lib().goalnet_epoch_plan(plan.data_ptr(), n, int(seed) & 0xFFFFFFFFFFFFFFFF, index, 1 if shuffle else 0, flip_p, max_shift, contrast,
                                   brightness, _s()), "epoch_plan")
    return plan


def frames_gather_aug(table, out, plan, nrows, cursor, cursor_bias=0, colour=False):
    """out[i] = the frame plan[cursor + cursor_bias + i] names, flipped / shifted (edge-replicate) and, with `colour`, gain / bias /
    clamp to [0, 1]; table (rows, C, H, W), out (nrows, C, H, W), fp32. One launch."""
    _chk(table, out)
    _plan_ok(plan, "frames_gather_aug")
    _req(table.dtype == F32 and out.dtype == F32 and table.dim() == 4 and table.is_contiguous() and out.is_contiguous()
         and tuple(out.shape) == (nrows,) + tuple(table.shape[1:]), "frames_gather_aug: fp32 (rows, C, H, W) table and (nrows, C, H, W) block")
    _, C, H, W = table.shape
    check(lib().goalnet_frames_gather_aug(table.data_ptr(), table.shape[0], out.data_ptr(), plan.data_ptr(), plan.shape[0], C, H, W, nrows,
                                          _ctr(cursor), int(cursor_bias), 1 if colour else 0, _s()), "frames_gather_aug")
    return out


def rows_copy_indexed(segments, plan):
    """rows_copy_batch through the plan's order: segments of (table, block, nrows, cursor, cursor_bias, gather, indexed). Indexed
    gather: block[i] = table[plan[c + i].src]; indexed scatter: table[plan[c + i].src] = block[i]; not indexed: rows [c, c + nrows)
    as rows_copy_batch. One launch for up to 4 segments."""
    _plan_ok(plan, "rows_copy_indexed")
    _req(1 <= len(segments) <= _lib.ROWCOPY_MAX, f"rows_copy_indexed: 1..{_lib.ROWCOPY_MAX} segments")
    arr = (_lib.RowCopyIndexed * len(segments))()
    for k, (table, block, nrows, cursor, bias, gather, indexed) in enumerate(segments):
        _chk(table, block)
        _req(table.is_contiguous() and block.is_contiguous() and table.dtype == block.dtype, "rows_copy_indexed: contiguous tensors of one dtype")
        row_bytes = table[0].numel() * table.element_size() if table.dim() > 1 else table.element_size()
        _req(block.numel() * block.element_size() == row_bytes * nrows, "rows_copy_indexed: block size")
        src, dst = (table, block) if gather else (block, table)
        arr[k] = _lib.RowCopyIndexed(src.data_ptr(), dst.data_ptr(), row_bytes, nrows, 1 if gather else 0, _ctr(cursor), int(bias),
                                     1 if indexed else 0, table.shape[0])
    check(lib().goalnet_rows_copy_indexed(arr, len(segments), plan.data_ptr(), plan.shape[0], _s()), "rows_copy_indexed")


# ---- audio augmentation and mixup on such a pass (include/goalnet_mix.h, csrc/mix.hip) -------------------------
AUDIO_COEFFS = 30         # MFCC coefficients per frame: rows of the (N, 30, B) audio tables


def _int_option(name, v, hi):
    if isinstance(v, bool) or not isinstance(v, int) or v < 0 or (hi is not None and v > hi):
        raise ValueError(f"{name} must be an integer " + (">= 0" if hi is None else f"in [0, {hi}]") + f", got {v!r}")
    return v


def _f32_option(name, v, ok):
    try:
        f = ctypes.c_float(float(v)).value
    except (TypeError, ValueError):
        raise ValueError(f"{name} must be a number, got {v!r}") from None
    if isinstance(v, bool) or not ok(f):                # NaN fails every comparison
        raise ValueError(f"{name} = {v!r} is outside its range")
    return f


def audio_augment_spec(max_shift=0, time_mask=0, coeff_mask=0, gain=0.0, noise=0.0):
    """(max_shift, time_mask, coeff_mask, gain, noise) as goalnet_epoch_plan2 takes them — ValueError on a value outside its range,
    before any launch and without a GPU. The two floats are rounded to fp32 here: that is what the draws are defined on.
    (time_mask <= bins can only be checked against a video: goalnet_epoch_plan2's wrapper and train_video do that.)"""
    return (_int_option("max_shift", max_shift, _lib.MAX_SHIFT), _int_option("time_mask", time_mask, None),
            _int_option("coeff_mask", coeff_mask, AUDIO_COEFFS - 1), _f32_option("gain", gain, lambda f: 0.0 <= f < 1.0),
            _f32_option("noise", noise, lambda f: 0.0 <= f < float("inf")))


def mixup_spec(strength=0.0, p=0.0):
    """(strength, p) as goalnet_epoch_plan2 takes them, rounded to fp32 — ValueError outside [0, 1], without a GPU"""
    return _f32_option("strength", strength, lambda f: 0.0 <= f <= 1.0), _f32_option("p", p, lambda f: 0.0 <= f <= 1.0)


def _plan2_ok(plan2, plan, who):
    _plan_ok(plan, who)
    _req(torch.is_tensor(plan2) and plan2.is_cuda and plan2.dtype == I32 and plan2.dim() == 2 and plan2.shape[1] == _lib.PLAN2_WORDS
         and plan2.is_contiguous() and plan2.shape[0] >= plan.shape[0] and plan2.device == plan.device,
         f"{who}: plan2 must be a contiguous int32 (>= {plan.shape[0]}, {_lib.PLAN2_WORDS}) GPU tensor beside the plan")


def epoch_plan2(plan2, plan, n, seed, index, C, B, max_shift=0, time_mask=0, coeff_mask=0, gain=0.0, noise=0.0, strength=0.0, p=0.0):
    """rows [0, n) of `plan2` (int32 (>= n, 12)) = the audio / mixup draws of pass `index` for the frames rows [0, n) of the finished
    `plan` name: {a_shift, t0, tw, c0, cw, gain, partner, lambda, nkey lo, nkey hi, 0, 0}; the audio table is (rows, C, B)"""
    max_shift, time_mask, coeff_mask, gain, noise = audio_augment_spec(max_shift, time_mask, coeff_mask, gain, noise)
    strength, p = mixup_spec(strength, p)
    if not 1 <= n <= _lib.EPOCH_MAX_N:
        raise ValueError(f"a pass takes 1..{_lib.EPOCH_MAX_N} frames, got {n}")
    if not 0 <= index < _lib.PLAN2_MAX_INDEX:
        raise ValueError(f"pass index must be in [0, 2^26), got {index}")
    if C < 1 or B < 1 or time_mask > B or coeff_mask > C - 1:
        raise ValueError(f"time_mask = {time_mask} / coeff_mask = {coeff_mask} do not fit a ({C}, {B}) audio row")
    _plan2_ok(plan2, plan, "epoch_plan2")
    _req(plan.shape[0] >= n, "epoch_plan2: the plan tables are shorter than the pass")
    check(lib().goalnet_epoch_plan2(plan2.data_ptr(), plan.data_ptr(), n, int(seed) & 0xFFFFFFFFFFFFFFFF, index, C, B, max_shift, time_mask,
                                    coeff_mask, gain, noise, strength, p, _s()), "epoch_plan2")
    return plan2


def audio_gather_aug(table, out, plan, plan2, nrows, cursor, cursor_bias=0, gain=False, noise=0.0, mix=False):
    """out[i] = the audio row plan[cursor + cursor_bias + i] names, shifted in time (edge-replicate), with `gain` scaled, with
    `noise` > 0 plus uniform noise of that amplitude, time / coefficient masked (never coefficient 0) and, with `mix`, mixed with
    its partner's as plan2 says; table (rows, C, B), out (nrows, C, B), fp32. No flag: values are moved as words. One launch."""
    _chk(table, out)
    _plan2_ok(plan2, plan, "audio_gather_aug")
    _req(table.dtype == F32 and out.dtype == F32 and table.dim() == 3 and table.is_contiguous() and out.is_contiguous()
         and tuple(out.shape) == (nrows,) + tuple(table.shape[1:]), "audio_gather_aug: fp32 (rows, C, B) table and (nrows, C, B) block")
    noise = _f32_option("noise", noise, lambda f: 0.0 <= f < float("inf"))
    flags = (_lib.AUDIO_GAIN if gain else 0) | (_lib.AUDIO_NOISE if noise > 0 else 0) | (_lib.AUDIO_MIX if mix else 0)
    _, C, B = table.shape
    check(lib().goalnet_audio_gather_aug(table.data_ptr(), table.shape[0], out.data_ptr(), plan.data_ptr(), plan2.data_ptr(), plan.shape[0], C, B,
                                         nrows, _ctr(cursor), int(cursor_bias), flags, noise, _s()), "audio_gather_aug")
    return out


def frames_gather_mix(table, out, plan, plan2, nrows, cursor, cursor_bias=0, colour=False):
    """frames_gather_aug with the mix: a row plan2 marks as mixed is lambda * its own augmented frame + (1 - lambda) * its partner's"""
    _chk(table, out)
    _plan2_ok(plan2, plan, "frames_gather_mix")
    _req(table.dtype == F32 and out.dtype == F32 and table.dim() == 4 and table.is_contiguous() and out.is_contiguous()
         and tuple(out.shape) == (nrows,) + tuple(table.shape[1:]), "frames_gather_mix: fp32 (rows, C, H, W) table and (nrows, C, H, W) block")
    _, C, H, W = table.shape
    check(lib().goalnet_frames_gather_mix(table.data_ptr(), table.shape[0], out.data_ptr(), plan.data_ptr(), plan2.data_ptr(), plan.shape[0], C, H,
                                          W, nrows, _ctr(cursor), int(cursor_bias), 1 if colour else 0, _s()), "frames_gather_mix")
    return out


def rows_mix_indexed(segments, plan, plan2):
    """fp32 row tables through the plan with the mix: segments of (table, block, nrows, cursor, cursor_bias);
    block[i] = mix(table[plan[c + i].src], table[plan[partner].src]). One launch for up to 4 segments."""
    _plan2_ok(plan2, plan, "rows_mix_indexed")
    _req(1 <= len(segments) <= _lib.ROWCOPY_MAX, f"rows_mix_indexed: 1..{_lib.ROWCOPY_MAX} segments")
    arr = (_lib.RowMix * len(segments))()
    for k, (table, block, nrows, cursor, bias) in enumerate(segments):
        _chk(table, block)
        _req(table.is_contiguous() and block.is_contiguous() and table.dtype == F32 and block.dtype == F32, "rows_mix_indexed: contiguous fp32 tensors")
        row_elems = table[0].numel() if table.dim() > 1 else 1
        _req(block.numel() == row_elems * nrows, "rows_mix_indexed: block size")
        arr[k] = _lib.RowMix(table.data_ptr(), block.data_ptr(), row_elems, nrows, _ctr(cursor), int(bias), table.shape[0])
    check(lib().goalnet_rows_mix_indexed(arr, len(segments), plan.data_ptr(), plan2.data_ptr(), plan.shape[0], _s()), "rows_mix_indexed")


# ---- inference mode around the model (csrc/summary.hip) ---------------------------------------------------------------------
def frames_preprocess_strided(frames, stride, out, minmax):
    """out (n, 3, H, W) fp32 = frames_preprocess of frames[::stride], n = ceil(n_total / stride), read in place from the whole
    video `frames` (n_total, H0, W0, 3) uint8; minmax: int32 scratch (n, 2)"""
    _chk(frames, out, minmax)
    _req(frames.dtype == torch.uint8 and frames.dim() == 4 and frames.shape[3] == 3 and frames.is_contiguous(),
         "frames_preprocess_strided: frames must be contiguous uint8 (n_total, H0, W0, 3)")
    n_total, h0, w0, _ = frames.shape
    _req(stride >= 1 and n_total >= 1, "frames_preprocess_strided: stride and n_total must be >= 1")
    n = (n_total + stride - 1) // stride
    _req(out.dtype == F32 and out.dim() == 4 and out.shape[0] == n and out.shape[1] == 3 and out.is_contiguous(),
         "frames_preprocess_strided: out must be contiguous fp32 (ceil(n_total / stride), 3, H, W)")
    _req(minmax.dtype == torch.int32 and minmax.numel() == 2 * n and minmax.is_contiguous(), "frames_preprocess_strided: minmax must be int32 (n, 2)")
    check(lib().goalnet_frames_preprocess_strided(frames.data_ptr(), n_total, int(stride), h0, w0, out.data_ptr(), out.shape[2], out.shape[3],
                                                  minmax.data_ptr(), _s()), "frames_preprocess_strided")
    return out


def gather_clips(frames, change_points, selected, out, capacity, src_index, count, status):
    """out[k] = the k-th frame of concatenate([frames[a:b] for the clips with selected != 0]) (end-exclusive slices); src_index[k] = its
    source frame; count (int64[1]) = the number of frames, status (int32[1]) != 0 when it exceeds `capacity` (then nothing is written
    past out[:capacity]). frames (full_n, ...) and out (>= capacity, ...) are contiguous uint8 with the same frame shape."""
    _chk(frames, change_points, selected, out, src_index, status)
    _req(frames.dtype == torch.uint8 and out.dtype == torch.uint8 and frames.is_contiguous() and out.is_contiguous() and frames.dim() >= 1
         and frames.shape[0] >= 1 and tuple(frames.shape[1:]) == tuple(out.shape[1:]), "gather_clips: frames / out must be contiguous uint8 with one frame shape")
    n_clips = selected.numel()
    _req(change_points.dtype == torch.int32 and selected.dtype == torch.int32 and change_points.numel() == 2 * n_clips
         and change_points.is_contiguous() and selected.is_contiguous(), "gather_clips: change_points int32 (n_clips, 2), selected int32 (n_clips)")
    _req(0 <= capacity <= out.shape[0] and src_index.dtype == torch.int32 and src_index.numel() >= capacity and src_index.is_contiguous(),
         "gather_clips: out and src_index must hold `capacity` frames")
    _req(status.dtype == torch.int32 and status.numel() == 1, "gather_clips: status must be int32[1]")
    frame_bytes = frames[0].numel()
    nbytes = lib().goalnet_gather_clips_ws_bytes(n_clips)
    ws = torch.empty(nbytes // 8, dtype=I64, device=frames.device)
    check(lib().goalnet_gather_clips(frames.data_ptr(), frames.shape[0], frame_bytes, change_points.data_ptr(), selected.data_ptr(), n_clips,
                                     out.data_ptr(), int(capacity), src_index.data_ptr(), _ctr(count), status.data_ptr(), ws.data_ptr(), nbytes, _s()),
          "gather_clips")
    return out
