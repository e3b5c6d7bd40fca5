#!/usr/bin/env python3
"""Rank correlation (csrc/rankcorr.hip; extension, parity unpinned — no reference code) against the evaluation step it sits beside
and against the host route it replaces. Nothing here is asserted by the test suite.

For n in {150, 650, 20000} compared frames (150 and 650: the sampled frames of a 4 500- and a 19 500-frame video at skip_frames 30;
20 000: every frame of a video, frames="full" at skip_frames 30), A = 20 annotators, B in {1, 20} prediction vectors:

  rank         `RankEvaluator(...)(pred)` (B = 1) / `.batch(preds)` (B = 20) on predictions resident on the device, read-back included
  fscore       `SummaryEvaluator.__call__(pred)` / `.fscores_batch(preds)` on the same video (one clip per 60 frames, annotator
               summaries from the same scores): the evaluation step that exists without this metric
  scipy        the 40 B calls of scipy.stats.kendalltau / spearmanr on the host, after reading the predictions back — only where
               SciPy imports; host wall clock, one repetition

Device events, alternating after warm-up, median of the repetitions.

    python scripts/bench_rankcorr.py [--out profiles/rankcorr_bench.json]
The driver starts every GPU step as a child process under its own `timeout`, and stops at the first one that fails.
"""
import argparse
import json
import os
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

SKIP, A = 30, 20
# n -> (full_n_frames, frames)
CASES = {150: (4500, "sampled"), 650: (19500, "sampled"), 20000: (20000, "full")}
BS = (1, 20)


def _timed(torch, fn, steps):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(steps):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / steps


def _video(np, n):
    full_n, frames = CASES[n]
    rng = np.random.default_rng(7 + n)
    scores = np.repeat(rng.integers(1, 6, size=(A, -(-full_n // 60))), 60, axis=1)[:, :full_n].astype(np.float32)
    n_sampled = -(-full_n // SKIP)
    preds = (scores[:, ::SKIP].mean(axis=0)[None, :] + rng.normal(0.0, 0.8, size=(max(BS), n_sampled))).astype(np.float32)
    starts = np.arange(0, full_n, 60)
    cps = np.stack([starts, np.minimum(starts + 59, full_n - 1)], axis=1)
    return full_n, frames, scores, preds, cps


def _scipy_ms(np, scores, preds, frames, full_n):
    try:
        import scipy.stats as st
    except ImportError:
        return None
    import warnings
    t0 = time.perf_counter()
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        for p in preds:
            x = p[np.arange(full_n) // SKIP] if frames == "full" else p
            for row in scores:
                y = row if frames == "full" else row[::SKIP]
                st.kendalltau(x, y, variant="b")
                st.spearmanr(x, y)
    return (time.perf_counter() - t0) * 1e3


def child_measure(args):
    import numpy as np
    import torch
    from cvml_goalnet_amd import RankEvaluator
    from cvml_goalnet_amd.postprocess import SummaryEvaluator
    res = {"metric": "ms per call (device events around host calls that end in one read-back), median of reps; scipy: host wall "
                     "clock of the 40 B calls, one repetition; extension, parity unpinned (no reference code)",
           "device": torch.cuda.get_device_name(0), "annotators": A, "skip_frames": SKIP, "steps": args.steps, "warmup": args.warmup,
           "reps": args.reps, "results": {}}
    for n, (full_n, frames) in CASES.items():
        full_n, frames, scores, preds, cps = _video(np, n)
        rank = RankEvaluator(scores, SKIP, frames)
        assert rank.n == n
        fs = SummaryEvaluator.from_annotations(cps, full_n, SKIP, scores)
        dev = torch.from_numpy(preds).cuda()
        for B in BS:
            steps = max(1, args.steps // 4) if n * B >= 20000 else args.steps
            if B == 1:
                calls = ((lambda: rank(dev[0])), (lambda: fs(dev[0])))
            else:
                calls = ((lambda: rank.batch(dev[:B])), (lambda: fs.fscores_batch(dev[:B])))
            for fn in calls:
                _timed(torch, fn, args.warmup)
            tr, tf = [], []
            for _ in range(args.reps):
                tr.append(_timed(torch, calls[0], steps))
                tf.append(_timed(torch, calls[1], steps))
            mr, mf = statistics.median(tr), statistics.median(tf)
            sc = _scipy_ms(np, scores, dev[:B].cpu().numpy(), frames, full_n)
            res["results"][f"n{n}_B{B}"] = {
                "n": n, "frames": frames, "full_n_frames": full_n, "batch": B, "pair_evaluations": n * n * A * B,
                "rank_ms": round(mr, 4), "fscore_ms": round(mf, 4), "rank_all_ms": [round(t, 4) for t in tr],
                "fscore_all_ms": [round(t, 4) for t in tf], "ratio_rank_over_fscore": round(mr / mf, 4),
                "scipy_host_ms": None if sc is None else round(sc, 2),
                "pair_evaluations_per_s": round(n * n * A * B / (mr * 1e-3), 1)}
            with open(args.out, "w") as f:
                f.write(json.dumps(res) + "\n")
    print(json.dumps(res))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--child", choices=["measure"])
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "rankcorr_bench.json"))
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--step-timeout", type=int, default=300, help="seconds per GPU step")
    args = ap.parse_args()
    if args.child == "measure":
        return child_measure(args)
    me = os.path.abspath(__file__)
    out = os.path.abspath(args.out)
    rc = subprocess.run(["timeout", "-k", "10", str(args.step_timeout), sys.executable, me, "--child", "measure", "--steps", str(args.steps),
                         "--warmup", str(args.warmup), "--reps", str(args.reps), "--out", out]).returncode
    if rc != 0:
        raise SystemExit(f"bench_rankcorr: the measure step ended with status {rc}; nothing more is started")
    print("wrote", out)


if __name__ == "__main__":
    main()
