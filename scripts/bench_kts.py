#!/usr/bin/env python3
"""Temporal segmentation (csrc/kts.hip; extension, parity unpinned — no reference code) against the call it extends. Nothing here
is asserted by the test suite.

For n in {150, 300, 2000} sampled frames, d = 640 (the descriptor of a model with audio), skip_frames 30, default
max_change_points = min(n - 1, ceil(full_n / 60)):

  segment      `TemporalSegmenter().segment(descriptors, full_n, skip)` on descriptors resident on the device, read-back included
  summarize    `VideoSummarizer(model, change_points, skip)(video)` with GIVEN change points (one clip per 60 frames) on a synthetic
               video of the same n (24 x 32 frames, audio features given): the path that exists without segmentation, and what the
               segment figure is to be read against. Expectation to check: segment <= summarize, i.e. auto-segmenting at most
               doubles a summary.

Device events, alternating after warm-up, median of the repetitions. The per-kernel split of `segment` comes from
`rocprofv3 --kernel-trace --stats` over a short run of the same calls (times under the profiler).

    python scripts/bench_kts.py [--out profiles/kts_bench.json] [--no-profile]
The driver starts every GPU step as a child process under its own `timeout`, and stops at the first one that fails.
"""
import argparse
import csv
import glob
import json
import os
import statistics
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

NS = (150, 300, 2000)
D, SKIP, H0, W0 = 640, 30, 24, 32


def _planted(torch, n, seed):
    """unit rows in scenes of about 20 samples plus noise: a segmentation with something to find"""
    g = torch.Generator().manual_seed(seed)
    x = torch.zeros(n, D)
    a = 0
    while a < n:
        b = min(n, a + 12 + int(torch.randint(0, 17, (1,), generator=g)))
        x[a:b] = torch.randn(D, generator=g)
        a = b
    x += 0.05 * torch.randn(n, D, generator=g)
    return (x / x.norm(dim=1, keepdim=True)).cuda()


def _timed(torch, fn, steps):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(steps):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / steps


def _calls(torch, n):
    import numpy as np
    from cvml_goalnet_amd import AVM, TemporalSegmenter, VideoSummarizer, synth
    full_n = n * SKIP
    x = _planted(torch, n, 11 + n)
    seg = TemporalSegmenter()
    model = AVM(audio_included=True, device="cuda:0", seed=synth.BASE_SEED).eval()
    g = torch.Generator(device="cuda:0").manual_seed(5 + n)
    video = torch.randint(0, 256, (full_n, H0, W0, 3), dtype=torch.uint8, device="cuda:0", generator=g)
    audio = torch.from_numpy(synth.make_audio(n)).cuda()
    starts = np.arange(0, full_n, 60)
    cps = np.stack([starts, np.minimum(starts + 59, full_n - 1)], axis=1)
    vs = VideoSummarizer(model, cps, skip_frames=SKIP)
    return (lambda: seg.segment(x, full_n, SKIP)), (lambda: vs(video, audio_features=audio)), seg.default_max_change_points(n, full_n)


def child_measure(args):
    import torch
    res = {"metric": "ms per call (device events around host calls that end in one read-back), median of reps; extension, parity "
                     "unpinned (no reference code)",
           "device": torch.cuda.get_device_name(0), "d": D, "skip_frames": SKIP, "steps": args.steps, "warmup": args.warmup,
           "reps": args.reps, "results": {}}
    for n in NS:
        segment, summarize, max_cp = _calls(torch, n)
        m = segment().n_change_points
        for fn in (segment, summarize):
            _timed(torch, fn, args.warmup)
        ts, tv = [], []
        for _ in range(args.reps):
            ts.append(_timed(torch, segment, args.steps))
            tv.append(_timed(torch, summarize, args.steps))
        ms, mv = statistics.median(ts), statistics.median(tv)
        res["results"][f"n{n}"] = {"n": n, "full_n_frames": n * SKIP, "max_change_points": max_cp, "change_points_found": m,
                                   "segment_ms": round(ms, 4), "summarize_given_change_points_ms": round(mv, 4),
                                   "segment_all_ms": [round(t, 4) for t in ts], "summarize_all_ms": [round(t, 4) for t in tv],
                                   "ratio_segment_over_summarize": round(ms / mv, 4)}
    with open(args.out, "w") as f:
        f.write(json.dumps(res) + "\n")
    print(json.dumps(res))


def child_profile(args):
    import torch
    from cvml_goalnet_amd import TemporalSegmenter
    n = args.n
    x = _planted(torch, n, 11 + n)
    seg = TemporalSegmenter()
    for _ in range(3):
        seg.segment(x, n * SKIP, SKIP)
    torch.cuda.synchronize()


def _kernel_split(csv_path, calls):
    out = {}
    for r in csv.DictReader(open(csv_path)):
        name = r["Name"].replace("(anonymous namespace)::", "").replace("void ", "").split("(")[0]
        if name.startswith("kts_"):
            out[name] = {"launches_per_call": int(r["Calls"]) // calls, "ms_per_call": round(float(r["TotalDurationNs"]) / 1e6 / calls, 4)}
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--child", choices=["measure", "profile"])
    ap.add_argument("--n", type=int, default=0)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "kts_bench.json"))
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--no-profile", action="store_true")
    ap.add_argument("--step-timeout", type=int, default=240, help="seconds per GPU step")
    args = ap.parse_args()
    if args.child == "measure":
        return child_measure(args)
    if args.child == "profile":
        return child_profile(args)

    me = os.path.abspath(__file__)
    out = os.path.abspath(args.out)
    limit = ["timeout", "-k", "10", str(args.step_timeout)]
    common = ["--steps", str(args.steps), "--warmup", str(args.warmup), "--reps", str(args.reps), "--out", out]
    rc = subprocess.run(limit + [sys.executable, me, "--child", "measure"] + common).returncode
    if rc != 0:
        raise SystemExit(f"bench_kts: the measure step ended with status {rc}; nothing more is started")
    if args.no_profile:
        return
    res = json.loads(open(out).read())
    for n in NS:
        with tempfile.TemporaryDirectory() as tmp:
            rc = subprocess.run(limit + ["rocprofv3", "--kernel-trace", "--stats", "--output-format", "csv", "-d", tmp, "--",
                                         sys.executable, me, "--child", "profile", "--n", str(n)], cwd=tmp,
                                env={**os.environ, "TMPDIR": tmp}, stdout=subprocess.DEVNULL).returncode
            if rc != 0:
                raise SystemExit(f"bench_kts: the rocprofv3 step for n = {n} ended with status {rc}; nothing more is started")
            found = sorted(glob.glob(os.path.join(tmp, "**", "*_kernel_stats.csv"), recursive=True), key=os.path.getmtime)
            if not found:
                raise SystemExit("bench_kts: rocprofv3 wrote no *_kernel_stats.csv")
            res["results"][f"n{n}"]["kernels_under_profiler"] = _kernel_split(found[-1], 3)
    with open(out, "w") as f:
        f.write(json.dumps(res) + "\n")
    print("wrote", out)


if __name__ == "__main__":
    main()
