#!/usr/bin/env python3
"""Fine-tuning (requires_grad=False on AVM parameters): what a step costs when part of the model is frozen.
Nothing here is asserted by the test suite; the condition the feature states is that every frozen step is faster than the
all-trainable step of the same build at both shapes (and that step is the parent's: bench.py's headline).

  loop40    loop.VideoTrainer (captured graphs) over a 400-frame video of 40 x 40 in sub-batches of 10: ms per optimizer step
  step224   AVM.train_step on 1024 frames of 224 x 224: ms per step

for the sets: all trainable | visbl.* frozen | visbl.* + audbl.* frozen | only visbl.linear5.weight frozen. fp32, audio on, one
model per set, one process, device events, the sets alternating after warm-up, median of the repetitions.

    python scripts/bench_finetune.py [--out profiles/finetune_bench.json]
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

SETS = {
    "all_trainable": lambda k: False,
    "visbl_frozen": lambda k: k.startswith("visbl."),
    "visbl_audbl_frozen": lambda k: k.startswith(("visbl.", "audbl.")),
    "linear5_weight_frozen": lambda k: k == "visbl.linear5.weight",
}


def _timed(torch, fn, steps):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(steps):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / steps


def _models(torch, n, h):
    from cvml_goalnet_amd import AVM
    out = {}
    for name, rule in SETS.items():
        torch.manual_seed(7)
        m = AVM(audio_included=True, device="cuda:0")
        m._materialize_for(torch.zeros(n, 30, 30), torch.zeros(n, 3, h, h))
        for k, p in m.named_parameters():
            p.requires_grad = not rule(k)
        out[name] = m
    return out


def _table(times):
    med = {k: statistics.median(v) for k, v in times.items()}
    base = med["all_trainable"]
    return {k: {"ms_per_step": round(med[k], 4), "ratio_to_all_trainable": round(med[k] / base, 4), "faster_than_all_trainable": bool(med[k] < base),
                "all_ms": [round(t, 4) for t in times[k]]} for k in SETS}


def child_measure(args):
    import torch
    from cvml_goalnet_amd.loop import VideoTrainer
    dev = "cuda:0"
    res = {"metric": "ms per optimizer step (device events), median of reps, sets alternating", "device": torch.cuda.get_device_name(0),
           "precision": "fp32", "warmup": args.warmup, "reps": args.reps, "results": {}}

    # the reference's operating point: the graph loop, 10 frames of 40 x 40 per optimizer step
    frames, sb, h = 400, 10, 40
    torch.manual_seed(11)
    vid = (torch.randn(frames, 30, 30, device=dev), torch.rand(frames, 3, h, h, device=dev), torch.rand(frames, device=dev) * 4 + 1)
    trainers = {k: VideoTrainer(m, subbatch_size=sb) for k, m in _models(torch, sb, h).items()}
    for tr in trainers.values():
        _timed(torch, lambda: tr.train_video(*vid), args.warmup)
    times = {k: [] for k in SETS}
    for _ in range(args.reps):
        for k, tr in trainers.items():
            times[k].append(_timed(torch, lambda: tr.train_video(*vid), args.videos) / (frames // sb))
    res["results"]["loop40_n10_h40"] = dict(_table(times), frames=frames, subbatch=sb,
                                            replays={k: tr.replays for k, tr in trainers.items()})
    with open(args.out, "w") as f:
        f.write(json.dumps(res) + "\n")
    del trainers, vid
    torch.cuda.empty_cache()

    # bench.py's batch: one eager step of 1024 frames of 224 x 224
    n, h = 1024, 224
    aud, vis, lab = torch.randn(n, 30, 30, device=dev), torch.rand(n, 3, h, h, device=dev), torch.rand(n, device=dev) * 4 + 1
    models = _models(torch, n, h)
    for m in models.values():
        _timed(torch, lambda: m.train_step(aud, vis, lab), args.warmup)
    times = {k: [] for k in SETS}
    for _ in range(args.reps):
        for k, m in models.items():
            times[k].append(_timed(torch, lambda: m.train_step(aud, vis, lab), args.steps))
    res["results"]["step224_n1024_h224"] = dict(_table(times), steps=args.steps)
    with open(args.out, "w") as f:
        f.write(json.dumps(res) + "\n")
    print(json.dumps(res))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--child", choices=["measure"])
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "finetune_bench.json"))
    ap.add_argument("--steps", type=int, default=2, help="1024-frame steps per timed interval")
    ap.add_argument("--videos", type=int, default=2, help="400-frame videos per timed interval")
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--step-timeout", type=int, default=420, help="seconds for the GPU step")
    args = ap.parse_args()
    if args.child == "measure":
        return child_measure(args)
    me = os.path.abspath(__file__)
    out = os.path.abspath(args.out)
    rc = subprocess.run(["timeout", "-k", "10", str(args.step_timeout), sys.executable, me, "--child", "measure", "--steps", str(args.steps),
                         "--videos", str(args.videos), "--warmup", str(args.warmup), "--reps", str(args.reps), "--out", out]).returncode
    if rc != 0:
        raise SystemExit(f"bench_finetune: the measure step ended with status {rc}; nothing more is started")
    print("wrote", out)


if __name__ == "__main__":
    main()
