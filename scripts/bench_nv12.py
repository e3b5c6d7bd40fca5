#!/usr/bin/env python3
"""Cost of NV12 as an input (csrc/nv12.hip) on one synthetic video resident on the device — 600 frames of
1080 x 1920, NV12 with a pitch of 2048 (1620 rows: 1.99 GB) and the same pictures as packed BGR (3.73 GB), skip_frames = 60:

  (a) `frames_to_tensor(nv12, stride=60, pixel_format="nv12")`: goalnet_nv12_preprocess_strided, 10 sampled frames
  (b) `frames_to_tensor(bgr, stride=60)`: goalnet_frames_preprocess_strided on the same pictures
  (c) `nv12.gather_clips_bgr`: the selected clips (90 frames = int(0.15 * 600), 3 clips of 30) converted on the way
  (d) `ops.gather_clips` of the same clips from the BGR video

Device events, the four sides alternating after warm-up, median of --reps windows of --steps calls (scripts/bench_summary.py's
protocol). (a) == (b) and (c) == (d) bit for bit is checked before anything is timed. Nothing here is asserted by the test suite.

    python scripts/bench_nv12.py [--out profiles/nv12_bench.json] [--frames 600] [--steps 20] [--reps 5]
    rocprofv3 --kernel-trace --stats --output-format csv -d DIR -- python scripts/bench_nv12.py --child profile
    python scripts/bench_nv12.py --stats DIR/.../kernel_stats.csv [--out profiles/nv12_bench.json]     (no GPU needed)

The last form folds the profiler's average kernel times into the JSON file: achieved GB/s of the two min / max kernels against
the bytes they actually read (the sampled frames' picture bytes: 1.5 B/px for NV12, 3 B/px for BGR), and writes the kernel table
as markdown next to it.
"""
import argparse
import csv
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

H0, W0, PITCH, SKIP, SIZE = 1080, 1920, 2048, 60, (40, 40)
ROWS = H0 + H0 // 2


def _timed(torch, fn, steps):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(steps):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / steps


def _setup(torch, frames):
    from cvml_goalnet_amd import nv12, ops
    from cvml_goalnet_amd.preprocess import frames_to_tensor
    dev = torch.device("cuda:0")
    g = torch.Generator(device=dev).manual_seed(20)
    video = torch.randint(0, 256, (frames, ROWS, PITCH), dtype=torch.uint8, device=dev, generator=g)
    bgr = nv12.nv12_to_bgr(video, (H0, W0))
    cap = int(0.15 * frames)
    length = cap // 3
    starts = [frames // 10, frames // 2, frames - length - 1]
    cps = torch.tensor([[s, s + length] for s in starts] + [[0, starts[0]]], dtype=torch.int32, device=dev)
    selected = torch.tensor([1, 1, 1, 0], dtype=torch.int32, device=dev)
    out = torch.empty(cap, H0, W0, 3, dtype=torch.uint8, device=dev)
    out2 = torch.empty_like(out)
    src, src2 = (torch.empty(cap, dtype=torch.int32, device=dev) for _ in range(2))
    count = torch.zeros(1, dtype=torch.int64, device=dev)
    status = torch.zeros(1, dtype=torch.int32, device=dev)
    sides = {
        "a_nv12_preprocess": lambda: frames_to_tensor(video, SIZE, stride=SKIP, pixel_format="nv12", frame_size=(H0, W0)),
        "b_bgr_preprocess": lambda: frames_to_tensor(bgr, SIZE, stride=SKIP),
        "c_nv12_gather_bgr": lambda: nv12.gather_clips_bgr(video, (H0, W0), None, "bt601", cps, selected, out, cap, src, count, status),
        "d_bgr_gather": lambda: ops.gather_clips(bgr, cps, selected, out2, cap, src2, count, status),
    }
    assert torch.equal(sides["a_nv12_preprocess"](), sides["b_bgr_preprocess"]())
    sides["c_nv12_gather_bgr"]()
    sides["d_bgr_gather"]()
    assert int(count.item()) == 3 * length and int(status.item()) == 0
    assert torch.equal(out[:3 * length], out2[:3 * length]) and torch.equal(src[:3 * length], src2[:3 * length])
    return sides, 3 * length


def _fold_stats(path, out):
    """average kernel times of a rocprofv3 kernel_stats.csv -> GB/s of the two min / max kernels, and the table as markdown"""
    res = json.load(open(out))
    n = res["sampled_frames"]
    rows = list(csv.DictReader(open(path)))
    read = {"nv12_minmax_strided_kernel": n * H0 * W0 * 3 // 2, "frame_minmax_strided_kernel": n * H0 * W0 * 3}
    res["minmax_kernels"] = {}
    lines = ["| kernel | calls | avg us | min us | max us |", "|---|---:|---:|---:|---:|"]
    for r in sorted(rows, key=lambda r: -float(r["TotalDurationNs"])):
        name = r["Name"]
        lines.append(f"| `{name[:110]}` | {r['Calls']} | {float(r['AverageNs']) / 1e3:.2f} | {float(r['MinNs']) / 1e3:.2f} | {float(r['MaxNs']) / 1e3:.2f} |")
        for key, nbytes in read.items():
            if key in name:
                avg = float(r["AverageNs"])
                res["minmax_kernels"][key] = {"bytes_read": nbytes, "avg_us_under_profiler": round(avg / 1e3, 2), "calls": int(r["Calls"]),
                                              "GBps": round(nbytes / avg, 1)}
    with open(out, "w") as f:
        f.write(json.dumps(res) + "\n")
    md = os.path.join(os.path.dirname(out), "nv12_kernel_stats.md")
    with open(md, "w") as f:
        f.write("# rocprofv3 --kernel-trace --stats — scripts/bench_nv12.py --child profile\n\n"
                f"{res['video']}; every side of the benchmark once for the equality check and three times more, the set-up (random video, one full "
                "conversion) is in the trace too. Times under the profiler; the timed numbers are in `nv12_bench.json`.\n\n" + "\n".join(lines) + "\n")
    print(json.dumps(res["minmax_kernels"]))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "nv12_bench.json"))
    ap.add_argument("--frames", type=int, default=600)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--child", choices=["profile"])
    ap.add_argument("--stats")
    args = ap.parse_args()
    if args.stats:
        return _fold_stats(args.stats, args.out)
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("bench_nv12.py measures on the GPU: none found")
    sides, gathered = _setup(torch, args.frames)
    if args.child == "profile":
        for _ in range(3):
            for fn in sides.values():
                fn()
        torch.cuda.synchronize()
        return
    for fn in sides.values():
        _timed(torch, fn, args.warmup)
    times = {k: [] for k in sides}
    for _ in range(args.reps):
        for k, fn in sides.items():
            times[k].append(_timed(torch, fn, args.steps))
    med = {k: statistics.median(v) for k, v in times.items()}
    n = -(-args.frames // SKIP)
    px = H0 * W0
    res = {"metric": "NV12 in against BGR in on one resident video: ms per call (device events), median of reps",
           "video": f"{args.frames} frames of {H0} x {W0}, NV12 pitch {PITCH} ({ROWS} rows) / packed BGR, skip_frames = {SKIP}",
           "device": torch.cuda.get_device_name(0), "steps": args.steps, "warmup": args.warmup, "reps": args.reps,
           "sampled_frames": n, "gathered_frames": gathered,
           "resident_bytes": {"nv12": args.frames * ROWS * PITCH, "nv12_compact": args.frames * px * 3 // 2, "bgr": args.frames * px * 3},
           "ms": {k: round(v, 4) for k, v in med.items()}, "all_ms": {k: [round(t, 4) for t in v] for k, v in times.items()},
           "ratio_a_over_b": round(med["a_nv12_preprocess"] / med["b_bgr_preprocess"], 3),
           "ratio_c_over_d": round(med["c_nv12_gather_bgr"] / med["d_bgr_gather"], 3),
           "gather_bytes": {"c_read_plus_written": gathered * px * 3 // 2 + gathered * px * 3, "d_read_plus_written": 2 * gathered * px * 3},
           "gather_TBps": {"c": round((gathered * px * 9 // 2) / med["c_nv12_gather_bgr"] / 1e9, 3),
                           "d": round((gathered * px * 6) / med["d_bgr_gather"] / 1e9, 3)}}
    with open(args.out, "w") as f:
        f.write(json.dumps(res) + "\n")
    print(json.dumps(res))


if __name__ == "__main__":
    main()
