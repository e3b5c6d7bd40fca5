#!/usr/bin/env python3
"""Cost of the audio front end (csrc/wave.hip): `to_mono` on 10 minutes of stereo int16, resident on the device,
at 44 100 Hz (1 / 2: one shared phase row, staged in LDS) and at 48 000 Hz (147 / 320: phase rows from global memory), beside

  (a) `dst.copy_(src)` of the same number of bytes in + out: the HBM yardstick (ratio = to_mono / copy), and
  (b) `extract_audio_features(result, 300, 30)`: the MFCC pipeline the waveform feeds. The expectation to check is
      to_mono < (b): accepting a file must not dominate audio pre-processing.

Device events, the sides alternating after warm-up, median of --reps windows of --steps calls (scripts/bench_summary.py's
protocol). Nothing here is asserted by the test suite.

    python scripts/bench_wave.py [--out profiles/wave_bench.json] [--minutes 10] [--steps 20] [--reps 5]
"""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

SLOTS, BIN_LENGTH = 300, 30


def _timed(torch, fn, steps):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(steps):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / steps


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "wave_bench.json"))
    ap.add_argument("--minutes", type=float, default=10.0)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--reps", type=int, default=5)
    args = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("bench_wave.py measures on the GPU: none found")
    from cvml_goalnet_amd import to_mono
    from cvml_goalnet_amd.preprocess import extract_audio_features
    res = {"metric": f"to_mono on {args.minutes:g} min of stereo int16 resident on the device: ms per call (device events), median of reps",
           "device": torch.cuda.get_device_name(0), "steps": args.steps, "warmup": args.warmup, "reps": args.reps, "results": {}}
    for sr in (44100, 48000):
        n = int(args.minutes * 60 * sr)
        g = torch.Generator(device="cuda:0").manual_seed(sr)
        x = torch.randint(-32768, 32768, (n, 2), dtype=torch.int16, device="cuda:0", generator=g)
        y = to_mono(x, sr)
        assert bool(torch.isfinite(y).all()) and torch.equal(y, to_mono(x, sr))
        moved = x.numel() * 2 + y.numel() * 4
        src = torch.empty(moved // 2, dtype=torch.uint8, device="cuda:0")          # copy_ reads and writes every byte: half each way
        dst = torch.empty_like(src)
        front = lambda: to_mono(x, sr)                                               # noqa: E731
        copy = lambda: dst.copy_(src)                                                # noqa: E731
        feats = lambda: extract_audio_features(y, SLOTS, BIN_LENGTH)                 # noqa: E731
        sides = {"to_mono": front, "copy": copy, "features": feats}
        for fn in sides.values():
            _timed(torch, fn, args.warmup)
        times = {k: [] for k in sides}
        for _ in range(args.reps):
            for k, fn in sides.items():
                times[k].append(_timed(torch, fn, args.steps))
        med = {k: statistics.median(v) for k, v in times.items()}
        res["results"][str(sr)] = {
            "frames_in": n, "samples_out": y.numel(), "bytes_read_plus_written": moved,
            "to_mono_ms": round(med["to_mono"], 4), "copy_same_bytes_ms": round(med["copy"], 4), "features_300x30_ms": round(med["features"], 4),
            "to_mono_all_ms": [round(t, 4) for t in times["to_mono"]], "copy_all_ms": [round(t, 4) for t in times["copy"]],
            "features_all_ms": [round(t, 4) for t in times["features"]],
            "to_mono_TBps": round(moved / med["to_mono"] / 1e9, 3), "copy_TBps": round(moved / med["copy"] / 1e9, 3),
            "ratio_to_mono_over_copy": round(med["to_mono"] / med["copy"], 3),
            "ratio_to_mono_over_features": round(med["to_mono"] / med["features"], 4),
            "front_end_cheaper_than_features": bool(med["to_mono"] < med["features"])}
        del x, y, src, dst
    with open(args.out, "w") as f:
        f.write(json.dumps(res) + "\n")
    print(json.dumps(res))


if __name__ == "__main__":
    main()
