"""Shuffled, augmented passes over a video that is resident on the GPU (EXTENSION — the reference feeds every video in time order
with the same pixels every epoch; DESIGN.md §4.13, include/goalnet_epoch.h).

A *plan* is drawn on the device once per pass: row i names the i-th frame the pass consumes and that frame's horizontal flip,
integer shift (edge-replicate), contrast gain and brightness bias. `loop.VideoTrainer(shuffle=..., augment=...)` consumes it inside
its captured graphs; the two functions here are the same kernels for the drop-in path (`model(a, v)` with a stock optimizer):

    plan = epoch_plan(len(frames), seed, epoch, shuffle=True, flip_p=0.5, max_shift=2, device="cuda:0")
    for a in range(0, len(frames), 10):
        x = gather_augmented(frames, plan, a, min(10, len(frames) - a))          # (count, 3, H, W)
        y = labels[plan[a:a + 10, 0].long()]                                      # column 0 is the source frame
"""
from __future__ import annotations

import torch

from . import ops, synth

AUGMENT_KEYS = ("flip_p", "max_shift", "contrast", "brightness")


def augment_options(augment) -> dict:
    """the four options of an `augment` dict with their defaults filled in, validated (ValueError) without a GPU"""
    if augment is None:
        augment = {}
    if not isinstance(augment, dict):
        raise ValueError("augment must be a dict of " + ", ".join(AUGMENT_KEYS) + " or None")
    unknown = sorted(set(augment) - set(AUGMENT_KEYS))
    if unknown:
        raise ValueError(f"unknown augment option(s) {unknown}: the options are {', '.join(AUGMENT_KEYS)}")
    return dict(zip(AUGMENT_KEYS, ops.augment_spec(**augment)))


def epoch_plan(n, seed=synth.BASE_SEED, index=0, shuffle=False, flip_p=0.0, max_shift=0, contrast=0.0, brightness=0.0, device=None):
    """int32 (n, 8) plan of pass `index` over n frames, rows {src, flip, dx, dy, gain bits, bias bits, 0, 0}"""
    ops.augment_spec(flip_p, max_shift, contrast, brightness)       # ValueError before a device is needed
    dev = torch.device("cuda", torch.cuda.current_device()) if device is None else torch.device(device)
    plan = torch.empty(max(int(n), 1), 8, dtype=torch.int32, device=dev)
    with torch.cuda.device(dev):
        return ops.epoch_plan(plan, int(n), seed, int(index), shuffle, flip_p, max_shift, contrast, brightness)


def gather_augmented(table, plan, start, count):
    """(count, C, H, W) fp32: the frames rows [start, start + count) of `plan` name, augmented as those rows say. `table` is the
    (N, C, H, W) fp32 video on the GPU. The colour step (gain, bias, clamp to [0, 1]) runs only if a row of the plan asks for it."""
    if not (torch.is_tensor(table) and table.is_cuda and table.dtype == torch.float32 and table.dim() == 4):
        raise RuntimeError("gather_augmented: the table must be a (N, C, H, W) float32 GPU tensor")
    if not (0 <= start and count >= 1 and start + count <= plan.shape[0]):
        raise RuntimeError(f"rows [{start}, {start + count}) are not inside a plan of {plan.shape[0]} rows")
    table = table.contiguous()
    with torch.cuda.device(table.device):
        ident = torch.tensor([0x3F800000, 0], dtype=torch.int32, device=plan.device)
        colour = bool((plan[:, 4:6] != ident).any())
        out = torch.empty((count,) + tuple(table.shape[1:]), dtype=torch.float32, device=table.device)
        cursor = torch.tensor([start], dtype=torch.int64, device=table.device)
        return ops.frames_gather_aug(table, out, plan, count, cursor[0], 0, colour)
