"""Batched post-processing against the single-item path, in one process (cvml_goalnet_amd/postprocess.py).

For the two fixture shapes (`postproc_typical_n4500`: 41 clips x 3 376 columns; `postproc_long_n20000`: 200 clips x 15 001
columns) and 20 seeded perturbations of the fixture's prediction vector:

    (a) 20 sequential SummaryEvaluator.postprocess calls            (20 launches sets, 20 read-backs, 20 one-CU knapsacks in a row)
    (b) one SummaryEvaluator.postprocess_batch of the same vectors  (20 knapsacks on 20 CUs, one read-back)

as the user calls them (`api_ms`, read-backs included) and as bare launches without any read-back (`launch_ms`: the kernels
alone), plus B = 1 through the batched kernels against the single call. Device events around each side, sides alternating
within every repetition, median over the repetitions. Writes profiles/postproc_batch_bench.json and prints it.

    python scripts/bench_postproc_batch.py [--reps 15] [--out profiles/postproc_batch_bench.json]
"""
import argparse
import json
import os
import statistics
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
from _golden import load_postproc  # noqa: E402
from cvml_goalnet_amd import postprocess as pp  # noqa: E402

B = 20


def timed(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=15)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "postproc_batch_bench.json"))
    args = ap.parse_args()
    out = {"batch": B, "reps": args.reps, "device": torch.cuda.get_device_name(0)}
    for case in ("postproc_typical_n4500", "postproc_long_n20000"):
        z = load_postproc(case)
        skip, full_n = int(z["skip"][0]), int(z["full_n"][0])
        ev = pp.SummaryEvaluator(z["change_points"], full_n, skip, None)
        rng = np.random.default_rng(41)
        base = z["pred"][:, 0]
        preds = torch.from_numpy(np.stack([np.clip(base + rng.standard_normal(base.shape).astype(np.float32) * 0.3, 0.0, 6.0)
                                           for _ in range(B)])).cuda()
        rows = [preds[b] for b in range(B)]
        one = preds[:1]

        sides = {
            "a_api_20_single_calls": lambda: [ev.postprocess(r) for r in rows],
            "b_api_one_batch_call": lambda: ev.postprocess_batch(preds),
            "a_launch_20_single": lambda: [ev._launch(r, with_fscore=False) for r in rows],
            "b_launch_one_batch": lambda: ev._launch_batch(preds, with_fscore=False),
            "single_launch_1": lambda: ev._launch(rows[0], with_fscore=False),
            "batch_launch_1": lambda: ev._launch_batch(one, with_fscore=False),
        }
        # both paths give the same answer before anything is timed
        sel_b, mask_b = ev.postprocess_batch(preds)
        for b in range(B):
            sel, mask = ev.postprocess(rows[b])
            assert sel == sel_b[b] and np.array_equal(mask, mask_b[b]), (case, b)
        for fn in sides.values():
            fn()
        torch.cuda.synchronize()
        times = {k: [] for k in sides}
        for rep in range(args.reps):
            order = list(sides) if rep % 2 == 0 else list(sides)[::-1]        # alternate which side runs first
            for k in order:
                times[k].append(timed(sides[k]))
        med = {k: statistics.median(v) for k, v in times.items()}
        name = ev.lib.goalnet_postprocess_batch_kernel_name(ev.n_clips, ev.cap_scaled).decode()
        out[case] = {
            "clips": ev.n_clips, "columns": ev.cap_scaled + 1, "frames": full_n, "batch_knapsack_kernel": name,
            "a_api_ms": med["a_api_20_single_calls"], "b_api_ms": med["b_api_one_batch_call"],
            "api_ratio_a_over_b": med["a_api_20_single_calls"] / med["b_api_one_batch_call"],
            "a_launch_ms": med["a_launch_20_single"], "b_launch_ms": med["b_launch_one_batch"],
            "launch_ratio_a_over_b": med["a_launch_20_single"] / med["b_launch_one_batch"],
            "per_item_ms_single_path": med["a_launch_20_single"] / B, "per_item_ms_batch_path": med["b_launch_one_batch"] / B,
            "single_call_launch_ms": med["single_launch_1"], "batch_of_1_launch_ms": med["batch_launch_1"],
            "b_over_one_single_call": med["b_launch_one_batch"] / med["single_launch_1"],
            "workspace_bytes_single": ev.ws_bytes, "workspace_bytes_batch_20": ev._b_ws_bytes,
            "min_ms": {k: min(v) for k, v in times.items()},
        }
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    print(json.dumps(out))


if __name__ == "__main__":
    main()
