"""Shuffled, augmented passes over a video that is resident on the GPU (EXTENSION — the reference feeds every video in time order
with the same pixels every epoch; DESIGN.md §4.13, include/goalnet_epoch.h).

A *plan* is drawn on the device once per pass: row i names the i-th frame the pass consumes and that frame's horizontal flip,
integer shift (edge-replicate), contrast gain and brightness bias. `loop.VideoTrainer(shuffle=..., augment=...)` consumes it inside
its captured graphs; the two functions here are the same kernels for the drop-in path (`model(a, v)` with a stock optimizer):

    plan = epoch_plan(len(frames), seed, epoch, shuffle=True, flip_p=0.5, max_shift=2, device="cuda:0")
    for a in range(0, len(frames), 10):
        x = gather_augmented(frames, plan, a, min(10, len(frames) - a))          # (count, 3, H, W)
        y = labels[plan[a:a + 10, 0].long()]                                      # column 0 is the source frame

Audio augmentation and mixup (include/goalnet_mix.h) draw a second table beside the plan and gather through both:

    plan2 = epoch_plan2(plan, seed, epoch, bins=audio.shape[2], max_shift=3, time_mask=6, gain=0.25, noise=0.5, strength=0.5, p=0.5)
        x = gather_mixed(frames, plan, plan2, a, count)                           # the frames, mixed with their partners'
        s = gather_audio_augmented(audio, plan, plan2, a, count, noise=0.5)       # (count, 30, B): shifted, masked, scaled, noised, mixed
        y = mix_rows(labels, plan, plan2, a, count)                               # the labels, blended the same way
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


# ---- audio augmentation and mixup on such a pass (EXTENSION; DESIGN.md §4.18, include/goalnet_mix.h) ------------------------------
AUDIO_AUGMENT_KEYS = ("max_shift", "time_mask", "coeff_mask", "gain", "noise")
MIXUP_KEYS = ("strength", "p")


def _options(what, given, keys, spec):
    if given is None:
        given = {}
    if not isinstance(given, dict):
        raise ValueError(f"{what} must be a dict of " + ", ".join(keys) + " or None")
    unknown = sorted(set(given) - set(keys), key=str)
    if unknown:
        raise ValueError(f"unknown {what} option(s) {unknown}: the options are {', '.join(keys)}")
    return dict(zip(keys, spec(**given)))


def audio_augment_options(audio_augment) -> dict:
    """the five options of an `audio_augment` dict with their defaults filled in, validated (ValueError) without a GPU"""
    return _options("audio_augment", audio_augment, AUDIO_AUGMENT_KEYS, ops.audio_augment_spec)


def mixup_options(mixup) -> dict:
    """the two options of a `mixup` dict with their defaults filled in, validated (ValueError) without a GPU"""
    return _options("mixup", mixup, MIXUP_KEYS, ops.mixup_spec)


def epoch_plan2(plan, seed=synth.BASE_SEED, index=0, coeffs=30, bins=30, max_shift=0, time_mask=0, coeff_mask=0, gain=0.0, noise=0.0,
                strength=0.0, p=0.0):
    """int32 (n, 12) second table of pass `index` for the finished (n, 8) `plan` of the same pass: rows {a_shift, t0, tw, c0, cw,
    gain bits, partner, lambda bits, nkey lo, nkey hi, 0, 0} — a time shift, a time mask [t0, t0 + tw), a coefficient mask [c0, c0 + cw)
    (never coefficient 0), a gain and a noise key for the frame's (coeffs, bins) audio row, and its mixup partner (a position in the
    plan) with the weight lambda of its own sample. A row whose lambda is exactly 1.0 is not mixed."""
    ops.audio_augment_spec(max_shift, time_mask, coeff_mask, gain, noise)       # ValueError before a device is needed
    ops.mixup_spec(strength, p)
    if not (torch.is_tensor(plan) and plan.is_cuda):
        raise RuntimeError("epoch_plan2: the plan must be the GPU tensor epoch_plan returned")
    plan2 = torch.empty(plan.shape[0], 12, dtype=torch.int32, device=plan.device)
    with torch.cuda.device(plan.device):
        return ops.epoch_plan2(plan2, plan, plan.shape[0], seed, int(index), int(coeffs), int(bins), max_shift, time_mask, coeff_mask, gain, noise,
                               strength, p)


def _window(who, table, dim, plan, start, count):
    if not (torch.is_tensor(table) and table.is_cuda and table.dtype == torch.float32 and table.dim() == dim):
        raise RuntimeError(f"{who}: the table must be a {dim}-dimensional float32 GPU tensor")
    if not (0 <= start and count >= 1 and start + count <= plan.shape[0]):
        raise RuntimeError(f"rows [{start}, {start + count}) are not inside a plan of {plan.shape[0]} rows")
    return torch.tensor([start], dtype=torch.int64, device=table.device)[0]


def gather_audio_augmented(table, plan, plan2, start, count, noise=0.0):
    """(count, C, B) fp32: the audio rows that rows [start, start + count) of `plan` name, augmented and mixed as those rows of `plan2`
    say. `table` is the (N, C, B) fp32 audio of the video on the GPU; `noise` is the amplitude plan2 was drawn with (the table holds
    only the per-frame keys). Gain and mix run only if a row of plan2 asks for them."""
    with torch.cuda.device(table.device):
        cursor = _window("gather_audio_augmented", table, 3, plan, start, count)
        one = torch.tensor(0x3F800000, dtype=torch.int32, device=plan2.device)
        out = torch.empty((count,) + tuple(table.shape[1:]), dtype=torch.float32, device=table.device)
        return ops.audio_gather_aug(table.contiguous(), out, plan, plan2, count, cursor, 0, gain=bool((plan2[:, 5] != one).any()), noise=noise,
                                    mix=bool((plan2[:, 7] != one).any()))


def gather_mixed(table, plan, plan2, start, count):
    """gather_augmented with mixup: a row that `plan2` marks as mixed is lambda * its own augmented frame + (1 - lambda) * its
    partner's augmented frame; every other row is what gather_augmented returns"""
    with torch.cuda.device(table.device):
        cursor = _window("gather_mixed", table, 4, plan, start, count)
        ident = torch.tensor([0x3F800000, 0], dtype=torch.int32, device=plan.device)
        out = torch.empty((count,) + tuple(table.shape[1:]), dtype=torch.float32, device=table.device)
        return ops.frames_gather_mix(table.contiguous(), out, plan, plan2, count, cursor, 0, bool((plan[:, 4:6] != ident).any()))


def mix_rows(table, plan, plan2, start, count):
    """(count, ...) fp32: rows of a per-frame table (labels, loss weights) in the plan's order, mixed with their partners' as the frames are"""
    with torch.cuda.device(table.device):
        cursor = _window("mix_rows", table, table.dim() if torch.is_tensor(table) else 1, plan, start, count)
        out = torch.empty((count,) + tuple(table.shape[1:]), dtype=torch.float32, device=table.device)
        ops.rows_mix_indexed([(table.contiguous(), out, count, cursor, 0)], plan, plan2)
        return out
