"""Cost of audio augmentation and mixup at the reference's operating point: the 40x40, 10-frames-per-step loop of
scripts/bench_loop.py on one video, graph-driven, with the features off, with the five audio options, with mixup and with both.
Prints one JSON line with the per-step times. The protocol is scripts/bench_shuffle.py's.

    python scripts/bench_mix.py [--frames 300] [--videos 20] [--rounds 8] [--hw 40] [--dtype f32|bf16]

Every configuration owns a model and a trainer, is warmed up on two videos (every sub-batch size has run eagerly and been captured),
and the configurations are timed alternately (a different one leads every round), `--rounds` times each: a window is `--videos` passes
that end in a device synchronise (the loop's one host read per video, main.py:203, is part of it). Reported per configuration: the
median and the spread (min, max) of its windows in us per optimizer step; an overhead is a difference of medians and means something
only beyond the spreads.
"""
import argparse
import json
import os
import statistics
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from cvml_goalnet_amd import AVM, synth  # noqa: E402
from cvml_goalnet_amd.loop import VideoTrainer  # noqa: E402

AUDIO = dict(max_shift=3, time_mask=6, coeff_mask=5, gain=0.25, noise=0.5)
MIXUP = dict(strength=0.5, p=0.5)
CONFIGS = {
    "off": dict(),
    "audio": dict(audio_augment=AUDIO),
    "mixup": dict(mixup=MIXUP),
    "audio+mixup": dict(audio_augment=AUDIO, mixup=MIXUP),
}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=300)
    ap.add_argument("--videos", type=int, default=20)
    ap.add_argument("--rounds", type=int, default=8)
    ap.add_argument("--hw", type=int, default=40)
    ap.add_argument("--sub", type=int, default=10)
    ap.add_argument("--dtype", default="f32")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_mix.py measures on the GPU: none found")
    dev = "cuda:0"
    n, h = a.frames, a.hw
    vis = torch.from_numpy(synth.make_visual(n, h, h)).to(dev)
    aud = torch.from_numpy(synth.make_audio(n)).to(dev)
    lab = torch.from_numpy(synth.make_labels(n)).to(dev)
    steps = a.videos * ((n + a.sub - 1) // a.sub)
    trainers = {}
    for name, kw in CONFIGS.items():
        model = AVM(audio_included=True, device=dev, precision="bf16" if a.dtype == "bf16" else "fp32")
        trainers[name] = VideoTrainer(model, subbatch_size=a.sub, **kw)
        for _ in range(2):
            trainers[name].train_video(aud, vis, lab)
    torch.cuda.synchronize()
    windows = {name: [] for name in CONFIGS}
    names = list(trainers)
    for r in range(a.rounds):
        for name in names[r % len(names):] + names[:r % len(names)]:      # a different configuration leads every round
            tr = trainers[name]
            t0 = time.perf_counter()
            for _ in range(a.videos):
                losses, _ = tr.train_video(aud, vis, lab)
                losses.mean().item()
            torch.cuda.synchronize()
            windows[name].append((time.perf_counter() - t0) / steps * 1e6)
    res = {"config": {"hw": h, "frames_per_video": n, "subbatch": a.sub, "dtype": a.dtype, "videos_per_window": a.videos, "rounds": a.rounds}}
    for name, w in windows.items():
        res[name] = {"us_per_step_median": statistics.median(w), "us_per_step_min": min(w), "us_per_step_max": max(w),
                     "replays": trainers[name].replays, "eager_steps": trainers[name].eager_steps}
    for name in ("audio", "mixup", "audio+mixup"):
        res[name]["overhead_us_per_step"] = res[name]["us_per_step_median"] - res["off"]["us_per_step_median"]
    print(json.dumps(res))


if __name__ == "__main__":
    main()
