#!/usr/bin/env python3
"""The O(n^2) pairwise rank loss (csrc/loss.hip) in proportion to the one-block broadcast MSE it can replace, at
n = 1 024 predictions. Nothing here is asserted by the test suite and no speed claim hangs on it.

  rank         goalnet_frame_loss(GOALNET_LOSS_RANK): loss and dpred, two launches (rows, finish), the workspace lent once
  rank_loss    the same with dpred = NULL (what VideoTrainer.eval_video runs)
  mse          goalnet_frame_loss(GOALNET_LOSS_MSE): one block
  mse_bcast    goalnet_mse_bcast: one block

Raw C-ABI calls enqueued back to back between two device events (so a call of a few microseconds is bounded by the launch rate, and
is named that), warm-up first, the four alternating, median of the repetitions.

    python scripts/bench_loss.py [--out profiles/loss_bench.json]
"""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "loss_bench.json"))
    ap.add_argument("--n", type=int, default=1024)
    ap.add_argument("--steps", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--reps", type=int, default=7)
    args = ap.parse_args()
    import torch
    from cvml_goalnet_amd import _lib
    assert torch.cuda.is_available(), "bench_loss needs the GPU"
    lib = _lib.load()
    n = args.n
    g = torch.Generator().manual_seed(5)
    pred = (1.0 + 4.0 * torch.rand(n, generator=g)).cuda()
    lab = torch.randint(1, 6, (n,), generator=g).float().cuda()
    loss, dpred = torch.empty(1, device="cuda"), torch.empty(n, device="cuda")
    nbytes = lib.goalnet_frame_loss_ws_bytes(_lib.LOSS_KINDS["rank"], n)
    ws = torch.empty(nbytes // 8, dtype=torch.float64, device="cuda")
    st = torch.cuda.current_stream().cuda_stream
    P, Lp, D = pred.data_ptr(), lab.data_ptr(), dpred.data_ptr()
    calls = {
        "rank": lambda: lib.goalnet_frame_loss(4, 0.0, P, Lp, None, n, loss.data_ptr(), D, ws.data_ptr(), nbytes, st),
        "rank_loss": lambda: lib.goalnet_frame_loss(4, 0.0, P, Lp, None, n, loss.data_ptr(), None, ws.data_ptr(), nbytes, st),
        "mse": lambda: lib.goalnet_frame_loss(1, 0.0, P, Lp, None, n, loss.data_ptr(), D, None, 0, st),
        "mse_bcast": lambda: lib.goalnet_mse_bcast(P, Lp, n, loss.data_ptr(), D, st),
    }

    def timed(fn, steps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(steps):
            rc = fn()
            assert rc == 0, lib.goalnet_last_error()
        e1.record()
        torch.cuda.synchronize()
        return e0.elapsed_time(e1) / steps * 1e3

    for fn in calls.values():
        timed(fn, args.warmup)
    all_us = {k: [] for k in calls}
    for _ in range(args.reps):
        for k, fn in calls.items():
            all_us[k].append(timed(fn, args.steps))
    labels = lab.cpu()
    pairs = int((labels[:, None] > labels[None, :]).sum())
    res = {"metric": "microseconds per call: device events around back-to-back C-ABI calls (launch-rate bound where a call is a few us), "
                     "median of reps; extension, no reference code",
           "device": torch.cuda.get_device_name(0), "n": n, "ordered_pairs": pairs, "steps": args.steps, "warmup": args.warmup, "reps": args.reps,
           "results": {k: {"us": round(statistics.median(v), 3), "all_us": [round(t, 3) for t in v]} for k, v in all_us.items()}}
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(json.dumps(res) + "\n")
    print(json.dumps(res))


if __name__ == "__main__":
    main()
