#!/usr/bin/env python3
"""The two HBM-traffic kernels of the inference mode (csrc/summary.hip) on one synthetic 9 000-frame 360 x 640 video (6.2 GB of
uint8, `torch.randint` on the device), skip_frames 30 and 60. Nothing here is asserted by the test suite.

  strided preprocess   `frames_to_tensor(video, stride=skip)` against what the parent commit offers for a resident video,
                       `frames_to_tensor(video[::skip].contiguous())`: same input, same process, device events, alternating after
                       warm-up; outputs compared bit for bit. ratio = strided / baseline (< 1: the strided call is faster).
  clip gather          `ops.gather_clips` (offset scan + copy) of the clips a random importance vector selects, against
                       `dst.copy_(src)` of the same number of bytes; achieved bytes/s counts read + write.
                       ratio = gather / copy (1.2 = 20 % slower than the plain copy).

The driver starts every GPU step as a child process under its own `timeout`, and stops at the first one that fails:
    python scripts/bench_summary.py [--out profiles/summary_bench.json] [--stats-md profiles/summary_kernel_stats.md] [--no-profile]
  step 1  measure  -> --out
  step 2  `rocprofv3 --kernel-trace --stats` over a short run of the same calls -> --stats-md (kernel names and times)
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

N_FRAMES, H0, W0 = 9000, 360, 640
SKIPS = (30, 60)
N_CLIPS = 120


def _setup(torch):
    from cvml_goalnet_amd import postprocess as pp
    g = torch.Generator(device="cuda:0").manual_seed(5)
    video = torch.randint(0, 256, (N_FRAMES, H0, W0, 3), dtype=torch.uint8, device="cuda:0", generator=g)
    cuts = torch.randperm(N_FRAMES - 1, generator=torch.Generator().manual_seed(6))[:N_CLIPS - 1].sort().values + 1
    starts = torch.cat([torch.zeros(1, dtype=torch.int64), cuts])
    ends = torch.cat([cuts - 1, torch.tensor([N_FRAMES - 1])])
    cps = torch.stack([starts, ends], dim=1).numpy()
    evs = {}
    for skip in SKIPS:
        n = (N_FRAMES + skip - 1) // skip
        pred = 1.0 + 4.0 * torch.rand(n, generator=torch.Generator().manual_seed(7 + skip))
        ev = pp.SummaryEvaluator(cps, N_FRAMES, skip)
        ev.postprocess(pred)                                  # leaves the 0/1 flags in ev.selected on the device
        evs[skip] = ev
    return video, evs


def _timed(torch, fn, steps):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(steps):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / steps


def _gather_call(torch, video, ev):
    from cvml_goalnet_amd import ops
    cap = ev.capacity
    out = torch.empty((cap,) + tuple(video.shape[1:]), dtype=torch.uint8, device=video.device)
    src_index = torch.empty(cap, dtype=torch.int32, device=video.device)
    count = torch.zeros(1, dtype=torch.int64, device=video.device)
    status = torch.zeros(1, dtype=torch.int32, device=video.device)
    return out, count, status, lambda: ops.gather_clips(video, ev.cps, ev.selected, out, cap, src_index, count, status)


def child_measure(args):
    import torch
    from cvml_goalnet_amd.preprocess import frames_to_tensor
    video, evs = _setup(torch)
    frame_bytes = H0 * W0 * 3
    res = {"metric": "inference-mode kernels on a resident 9000 x 360 x 640 x 3 uint8 video: ms per call (device events), median of reps",
           "device": torch.cuda.get_device_name(0), "steps": args.steps, "warmup": args.warmup, "reps": args.reps, "results": {}}
    for skip in SKIPS:
        r = {}
        base = lambda: frames_to_tensor(video[::skip].contiguous(), (40, 40))          # noqa: E731
        strided = lambda: frames_to_tensor(video, (40, 40), stride=skip)               # noqa: E731
        assert torch.equal(base(), strided()), "strided preprocess differs from the contiguous copy"
        for fn in (base, strided):
            _timed(torch, fn, args.warmup)
        tb, ts = [], []
        for _ in range(args.reps):
            tb.append(_timed(torch, base, args.steps))
            ts.append(_timed(torch, strided, args.steps))
        n = (N_FRAMES + skip - 1) // skip
        r["preprocess"] = {"frames": n, "baseline_copy_then_preprocess_ms": round(statistics.median(tb), 4),
                           "strided_ms": round(statistics.median(ts), 4), "baseline_all_ms": [round(t, 4) for t in tb],
                           "strided_all_ms": [round(t, 4) for t in ts],
                           "ratio_strided_over_baseline": round(statistics.median(ts) / statistics.median(tb), 4),
                           "source_bytes_read_once": n * frame_bytes}

        ev = evs[skip]
        out, count, status, gather = _gather_call(torch, video, ev)
        gather()
        k = int(count.item())
        assert k >= 1 and int(status.item()) == 0
        sel = torch.nonzero(ev.selected).flatten().tolist()
        cps = ev.cps.cpu()
        want = torch.cat([video[int(cps[c, 0]):int(cps[c, 1])] for c in sel])
        assert torch.equal(out[:k], want), "gather differs from the concatenated slices"
        src, dst = want.contiguous(), torch.empty_like(want)
        copy = lambda: dst.copy_(src)                                                   # noqa: E731
        for fn in (gather, copy):
            _timed(torch, fn, args.warmup)
        tg, tc = [], []
        for _ in range(args.reps):
            tg.append(_timed(torch, gather, args.steps))
            tc.append(_timed(torch, copy, args.steps))
        mg, mc = statistics.median(tg), statistics.median(tc)
        moved = 2 * k * frame_bytes
        r["gather"] = {"clips_selected": len(sel), "frames": k, "capacity": ev.capacity, "bytes_read_plus_written": moved,
                       "gather_ms": round(mg, 4), "copy_ms": round(mc, 4), "gather_all_ms": [round(t, 4) for t in tg],
                       "copy_all_ms": [round(t, 4) for t in tc], "gather_TBps": round(moved / mg / 1e9, 3),
                       "copy_TBps": round(moved / mc / 1e9, 3), "ratio_gather_over_copy": round(mg / mc, 4)}
        res["results"][f"skip{skip}"] = r
        del want, src, dst, out
    with open(args.out, "w") as f:
        f.write(json.dumps(res) + "\n")
    print(json.dumps(res))


def child_profile(args):
    import torch
    from cvml_goalnet_amd.preprocess import frames_to_tensor
    video, evs = _setup(torch)
    for skip in SKIPS:
        _, _, _, gather = _gather_call(torch, video, evs[skip])
        for _ in range(3):
            frames_to_tensor(video[::skip].contiguous(), (40, 40))
            frames_to_tensor(video, (40, 40), stride=skip)
            gather()
    torch.cuda.synchronize()


def _short(name):
    name = name.replace("(anonymous namespace)::", "").replace("void ", "").split("(")[0]
    return name if len(name) <= 120 else name[:117] + "..."


def write_stats_md(csv_path, md_path):
    rows = list(csv.DictReader(open(csv_path)))
    tot = sum(float(r["TotalDurationNs"]) for r in rows)
    with open(md_path, "w") as o:
        o.write("# rocprofv3 --kernel-trace --stats — scripts/bench_summary.py\n\n")
        o.write("`rocprofv3 --kernel-trace --stats --output-format csv -- python3 scripts/bench_summary.py --child profile`: per skip_frames "
                "(30, 60) three calls each of `frames_to_tensor(video[::skip].contiguous())` (the route without the strided entry point: "
                "a torch copy kernel, `frame_minmax_kernel`, `frame_resize_kernel`), `frames_to_tensor(video, stride=skip)` "
                "(`minmax_init_kernel`, `frame_minmax_strided_kernel`, `frame_resize_strided_kernel`) and `ops.gather_clips` "
                "(`clip_offsets_kernel`, `gather_clips_kernel`) on the 9 000 x 360 x 640 x 3 uint8 video; the set-up (random video, "
                "one postprocess per skip) is in the trace too. Times under the profiler; the timed numbers are in `summary_bench.json`.\n\n")
        o.write(f"Total kernel time {tot / 1e6:.1f} ms.\n\n| kernel | calls | total ms | avg ms | min ms | max ms | % |\n|---|---:|---:|---:|---:|---:|---:|\n")
        for r in rows:
            o.write(f"| `{_short(r['Name'])}` | {r['Calls']} | {float(r['TotalDurationNs']) / 1e6:.3f} | {float(r['AverageNs']) / 1e6:.4f} | "
                    f"{float(r['MinNs']) / 1e6:.4f} | {float(r['MaxNs']) / 1e6:.4f} | {float(r['Percentage']):.2f} |\n")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--child", choices=["measure", "profile"])
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "summary_bench.json"))
    ap.add_argument("--stats-md", default=os.path.join(ROOT, "profiles", "summary_kernel_stats.md"))
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--no-profile", action="store_true")
    ap.add_argument("--step-timeout", type=int, default=240, help="seconds per GPU step")
    args = ap.parse_args()
    if args.child == "measure":
        return child_measure(args)
    if args.child == "profile":
        return child_profile(args)

    me = os.path.abspath(__file__)
    limit = ["timeout", "-k", "10", str(args.step_timeout)]
    common = ["--steps", str(args.steps), "--warmup", str(args.warmup), "--reps", str(args.reps), "--out", os.path.abspath(args.out)]
    rc = subprocess.run(limit + [sys.executable, me, "--child", "measure"] + common).returncode
    if rc != 0:
        raise SystemExit(f"bench_summary: the measure step ended with status {rc}; nothing more is started")
    if args.no_profile:
        return
    with tempfile.TemporaryDirectory() as tmp:
        rc = subprocess.run(limit + ["rocprofv3", "--kernel-trace", "--stats", "--output-format", "csv", "-d", tmp, "--",
                                     sys.executable, me, "--child", "profile"], cwd=tmp, env={**os.environ, "TMPDIR": tmp},
                            stdout=subprocess.DEVNULL).returncode
        if rc != 0:
            raise SystemExit(f"bench_summary: the rocprofv3 step ended with status {rc}")
        found = sorted(glob.glob(os.path.join(tmp, "**", "*_kernel_stats.csv"), recursive=True), key=os.path.getmtime)
        if not found:
            raise SystemExit("bench_summary: rocprofv3 wrote no *_kernel_stats.csv")
        write_stats_md(found[-1], os.path.abspath(args.stats_md))
    print("wrote", args.stats_md)


if __name__ == "__main__":
    main()
