"""Gradient accumulation: the CPU side of tests/test_gpu_accum_step.py — the restatement of the accumulation pass and
the oracle runs of the independent check, kept apart from the device so that the check's precondition can be run without a GPU.

restate(acc, g, k, first)      the two torch operations the header names, on CPU tensors: t = g * (float)(1 / k); acc + t
oracle_large / oracle_window   the gradient of ONE step on all 18 frames, and of a window of k = 3 micro-steps of 6 frames accumulated
                               as the device accumulates, by oracle.avm_ref in fp32 or fp64: model.eval() (running-statistics
                               BatchNorm, no dropout) and loss = "mse", the mean of the per-frame squared errors, where
                               mean over 18 = (1 / 3) * sum of the three means over 6 holds mathematically.
verdicts(...)                  tests/_mode_case.py's grad_verdict for every tensor: at most F32_FACTOR["fp32"] x the oracle's own fp32
                               distance from the fp64 large-batch gradient, or within 2e-6 of the tensor's scale.

The data is tests/_mode_case.py's eval fixture at n = 18 (default seeds, converged BatchNorm statistics). The oracle alone passes on
it with its accumulated fp32 gradient in place of the device's: run on the CPU when the seed was adopted, the worst tensor
(visbl.bnorm2.bias) sits at 0.29 x its allowance and the fp64 window is within 2.2e-15 relative of the fp64 large batch; the GPU test
asserts that precondition again before it judges the device."""
import ctypes

import torch

from _mode_case import Cell, fixture, grad_verdict
from oracle import avm_ref

K, ROWS, N = 3, 6, 18
CELL = Cell("fp32", "regression", True, "eval", N)


def scale_of(k):
    return ctypes.c_float(1.0 / k).value              # c = (float)(1.0 / k)


def restate(acc, g, k, first):
    t = g * scale_of(k)
    return t if first else acc + t


def eval_fixture():
    return fixture("regression", True, "eval", N)


def _grads(fx, lo, hi, dtype):
    p = {k: v.to(dtype, copy=True).requires_grad_(True) for k, v in fx["p"].items()}
    b = {k: (v.to(dtype) if v.is_floating_point() else v.clone()) for k, v in fx["b"].items()}
    pred = avm_ref.forward(p, b, fx["aud"][lo:hi].to(dtype), fx["vis"][lo:hi].to(dtype), None, True, None, training=False)
    ((pred.view(-1) - fx["lab"][lo:hi].to(dtype)) ** 2).mean().backward()
    return {k: v.grad for k, v in p.items()}


def oracle_large(fx, dtype):
    return _grads(fx, 0, N, dtype)


def oracle_window(fx, dtype):
    """fp32: accumulated as the device does, c = (float)(1 / 3), product and sum rounded separately; fp64: with c = 1 / 3 in double"""
    acc = None
    for i in range(K):
        g = _grads(fx, i * ROWS, (i + 1) * ROWS, dtype)
        if dtype == torch.float32:
            acc = {k: restate(None if acc is None else acc[k], v, K, acc is None) for k, v in g.items()}
        else:
            acc = {k: v / K if acc is None else acc[k] + v / K for k, v in g.items()}
    return acc


def verdicts(mine, og, g64):
    """{name: (distance from the fp64 truth / the tensor's allowance, failure message or None)}"""
    from test_gpu_bench_shapes import F32_FACTOR
    out = {}
    for k, o in og.items():
        m = mine[k].reshape(o.shape)
        _, msg = grad_verdict(CELL, k, m, o, g64[k])
        scale = max(o.abs().max().item(), 1e-30)
        allow = max(F32_FACTOR["fp32"] * (o.double() - g64[k]).abs().max().item(), 2e-6 * scale)
        out[k] = ((m.double() - g64[k]).abs().max().item() / allow, msg)
    return out
