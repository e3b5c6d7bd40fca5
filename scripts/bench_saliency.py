#!/usr/bin/env python3
"""Input gradients (AVM.input_gradients / AVM.saliency, csrc/conv1.hip goalnet_conv1_dgrad) against the backward they are cut from.
Nothing here is asserted by the test suite; the condition the feature states is inputs_only < full on both shapes.

For N = 10 frames of 40 x 40 (the reference's sub-batch) and N = 1024 frames of 224 x 224 (bench.py's batch), fp32, audio on, on the
saved tensors of ONE train-mode forward:

  full          AVM.backward_device(ctx, dout): every parameter gradient into the arena (what loss.backward() runs)
  inputs_only   AVM.backward_device(ctx, dout, inputs=(True, True), params=False): the data-gradient chain alone, down to d_audio and
                d_visual — what input_gradients() runs behind its forward
  conv1_dgrad   goalnet_conv1_dgrad alone, reduce = 0 (dx) and reduce = 1 (max_ci |dx|), with the bandwidth its compulsory bytes
                (dy read once + dx or sal written once) amount to

One process, device events, the two sides alternating after warm-up, median of the repetitions.

    python scripts/bench_saliency.py [--out profiles/saliency_bench.json]
The driver starts the GPU step as a child process under its own `timeout`, and stops if it fails.
"""
import argparse
import json
import os
import statistics
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

SHAPES = ((10, 40), (1024, 224))


def _timed(torch, fn, steps):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(steps):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / steps


def child_measure(args):
    import torch
    from cvml_goalnet_amd import AVM, ops
    dev = "cuda:0"
    res = {"metric": "ms per call (device events), median of reps, sides alternating; GB/s from the compulsory bytes dy + dx (or dy + sal)",
           "device": torch.cuda.get_device_name(0), "precision": "fp32", "warmup": args.warmup, "reps": args.reps, "results": {}}
    for n, h in SHAPES:
        steps = args.steps if n <= 64 else max(1, args.steps // 10)
        torch.manual_seed(7)
        m = AVM(audio_included=True, device=dev)
        vis = torch.rand(n, 3, h, h, device=dev)
        aud = torch.randn(n, 30, 30, device=dev)
        m._materialize_for(aud, vis)
        out, ctx = m.forward_device(aud, vis, save=True)
        dout = torch.full((n,), 1.0 / n, device=dev)
        full = lambda: m.backward_device(ctx, dout)                                                      # noqa: E731
        only = lambda: m.backward_device(ctx, dout, inputs=(True, True), params=False)                   # noqa: E731
        ho = (h + 3) // 3 + 1
        dy = torch.randn(n, ho, ho, 64, device=dev)
        w1 = m._pflat("visbl.conv1.weight")
        dx, sal = torch.empty(n, 3, h, h, device=dev), torch.empty(n, h, h, device=dev)
        k0 = lambda: ops.conv1_dgrad(dy, w1, dx, 0, n, h, h)                                            # noqa: E731
        k1 = lambda: ops.conv1_dgrad(dy, w1, sal, 1, n, h, h)                                           # noqa: E731
        for fn in (full, only, k0, k1):
            _timed(torch, fn, args.warmup)
        tf, to, t0, t1 = [], [], [], []
        for _ in range(args.reps):
            tf.append(_timed(torch, full, steps))
            to.append(_timed(torch, only, steps))
            t0.append(_timed(torch, k0, args.steps))
            t1.append(_timed(torch, k1, args.steps))
        mf, mo, m0, m1 = (statistics.median(t) for t in (tf, to, t0, t1))
        b0, b1 = 4 * (dy.numel() + dx.numel()), 4 * (dy.numel() + sal.numel())
        res["results"][f"n{n}_h{h}"] = {
            "n": n, "h": h, "steps": steps,
            "full_backward_ms": round(mf, 4), "inputs_only_backward_ms": round(mo, 4), "ratio_inputs_only_over_full": round(mo / mf, 4),
            "inputs_only_is_faster": bool(mo < mf),
            "full_all_ms": [round(t, 4) for t in tf], "inputs_only_all_ms": [round(t, 4) for t in to],
            "conv1_dgrad_ms": round(m0, 5), "conv1_dgrad_bytes": b0, "conv1_dgrad_gbps": round(b0 / (m0 * 1e-3) / 1e9, 1),
            "conv1_dgrad_absmax_ms": round(m1, 5), "conv1_dgrad_absmax_bytes": b1, "conv1_dgrad_absmax_gbps": round(b1 / (m1 * 1e-3) / 1e9, 1)}
        with open(args.out, "w") as f:
            f.write(json.dumps(res) + "\n")
        del m, ctx, out, vis, aud, dy, dx, sal, full, only, k0, k1
        torch.cuda.empty_cache()
    print(json.dumps(res))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--child", choices=["measure"])
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "saliency_bench.json"))
    ap.add_argument("--steps", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--step-timeout", type=int, default=420, help="seconds for the GPU step")
    args = ap.parse_args()
    if args.child == "measure":
        return child_measure(args)
    me = os.path.abspath(__file__)
    out = os.path.abspath(args.out)
    rc = subprocess.run(["timeout", "-k", "10", str(args.step_timeout), sys.executable, me, "--child", "measure", "--steps", str(args.steps),
                         "--warmup", str(args.warmup), "--reps", str(args.reps), "--out", out]).returncode
    if rc != 0:
        raise SystemExit(f"bench_saliency: the measure step ended with status {rc}; nothing more is started")
    print("wrote", out)


if __name__ == "__main__":
    main()
