#!/usr/bin/env python3
"""Eval-mode forward vs train-mode forward, both under torch.no_grad(), at the same shape: one JSON line.

`model.eval()` replaces each BatchNorm block's statistics pass + finalise (and, at 40 x 40, the one-launch pool / statistics /
finalise kernel) by one pool launch that also writes the running-statistics affine (csrc/pool_bn.hip, goalnet_pool_bn_eval_fwd).
Both modes run the product path (AVM.forward_device, save=False) on device-resident inputs; times are device events around
`--steps` forwards after `--warmup`, the two modes alternating per repetition (`--reps`); the median repetition is reported.

    python scripts/bench_eval.py [--steps 10] [--warmup 3] [--reps 3] [--configs 224:256:fp32,224:256:bf16,...] [--modes train,eval]
"""
import argparse
import json
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from cvml_goalnet_amd import AVM, synth  # noqa: E402

DEFAULT = "224:256:fp32,224:256:bf16,224:256:fp16x3,40:10:fp32"


def time_forward(m, aud, vis, steps):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    with torch.no_grad():
        e0.record()
        for _ in range(steps):
            m.forward_device(aud, vis, save=False)
        e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / steps


def run(h, n, precision, modes, steps, warmup, reps):
    torch.manual_seed(7)
    m = AVM(audio_included=True, device="cuda:0", precision=precision, seed=synth.BASE_SEED)
    g = torch.Generator(device="cuda:0").manual_seed(11)
    vis = torch.rand(n, 3, h, h, device="cuda:0", generator=g)
    aud = torch.randn(n, 30, 30, device="cuda:0", generator=g) * 20
    res = {}
    for mode in modes:                                        # warm-up of both modes (first launches, cached operand buffers)
        m.train(mode == "train")
        time_forward(m, aud, vis, warmup)
    times = {mode: [] for mode in modes}
    for _ in range(reps):
        for mode in modes:
            m.train(mode == "train")
            times[mode].append(time_forward(m, aud, vis, steps))
    for mode in modes:
        res[f"{mode}_ms"] = round(statistics.median(times[mode]), 4)
        res[f"{mode}_all_ms"] = [round(t, 4) for t in times[mode]]
    if "train_ms" in res and "eval_ms" in res:
        res["eval_over_train"] = round(res["eval_ms"] / res["train_ms"], 4)
    del m
    torch.cuda.empty_cache()
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--configs", default=DEFAULT, help="comma-separated H:N:precision")
    ap.add_argument("--modes", default="train,eval")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_eval.py needs the GPU")
    modes = args.modes.split(",")
    out = {"metric": "no_grad forward, ms per call (device events), eval() vs train mode", "steps": args.steps,
           "warmup": args.warmup, "reps": args.reps, "device": torch.cuda.get_device_name(0), "results": {}}
    for cfg in args.configs.split(","):
        h, n, precision = cfg.split(":")
        out["results"][cfg] = run(int(h), int(n), precision, modes, args.steps, args.warmup, args.reps)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
