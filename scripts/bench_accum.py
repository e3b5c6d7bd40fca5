"""Gradient accumulation on the fused step: what a micro-step costs, variants alternating in one process, device events.

    python scripts/bench_accum.py [rounds=5] [--out profiles/accum_bench.json] [part ...]

Parts:
  kernels40   the arena of the 40 x 40 model (23.5 M parameters): goalnet_grad_accum_dev_ranges with first = 1 (8 B per parameter) and
              first = 0 (12 B) beside goalnet_adam_step_dev (28 B)
  step10      the 10-frame step at 40 x 40 as loop.VideoTrainer replays it (HIP graphs, 120-frame video = 12 sub-batches): without
              accumulate=, and with accumulate=4 — per sub-batch over the whole video, and per replay by phase (device events around
              every replay: a window's non-final micro-steps and its final one)

Each part runs in a child process of its own under a time limit; the parent never touches the GPU and stops at the first child that
fails. Nothing is gated: the figures are recorded as measured."""
import json, os, statistics, subprocess, sys, tempfile
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "scripts"))

from bench_ema import alternate, report      # noqa: E402

PARTS = ("kernels40", "step10")
CHILD_TIMEOUT_S = 300


def kernels40(rounds):
    import torch
    from cvml_goalnet_amd import ops
    dev = "cuda:0"
    n = 23482433 // 4 * 4
    p = torch.randn(n, device=dev) * 0.01; g = torch.randn(n, device=dev) * 1e-3
    m = torch.zeros(n, device=dev); v = torch.zeros(n, device=dev); acc = torch.zeros(n, device=dev)
    step = torch.zeros(1, dtype=torch.int64, device=dev)
    times = alternate(torch, {
        "adam_step_dev": lambda: ops.adam_step_dev(p, g, m, v, 1e-3, 0.9, 0.999, 1e-8, step, step_bias=1),
        "grad_accum first": lambda: ops.grad_accum_dev_ranges(acc, g, [(0, n)], 0.25, True),
        "grad_accum add": lambda: ops.grad_accum_dev_ranges(acc, g, [(0, n)], 0.25, False),
    }, rounds)
    per = {"adam_step_dev": 28, "grad_accum first": 8, "grad_accum add": 12}
    gbs = {k: (lambda ms, b=per[k]: f"{n * b / ms / 1e6:7.0f} GB/s") for k in times}
    out = report(f"arena 40x40 ({n / 1e6:.1f} M)", times, "adam_step_dev", extra=gbs)
    for k, row in out["variants"].items():
        row["GB_per_s"] = n * per[k] / row["median"] / 1e6
    out["parameters"] = n
    return out


def step10(rounds):
    import torch
    from cvml_goalnet_amd import AVM, synth
    from cvml_goalnet_amd.loop import VideoTrainer
    dev = "cuda:0"
    frames = 120
    aud = torch.from_numpy(synth.make_audio(frames)); vis = torch.from_numpy(synth.make_visual(frames, 40, 40))
    lab = torch.from_numpy(synth.make_labels(frames))
    trainers = {}
    for name, k in (("default", 1), ("accumulate 4", 4)):
        tr = VideoTrainer(AVM(audio_included=True, device=dev, seed=synth.BASE_SEED), subbatch_size=10, accumulate=k)
        tr.train_video(aud, vis, lab)               # eager steps, captures, replays
        tr.train_video(aud, vis, lab)
        trainers[name] = tr
    times = alternate(torch, {k: (lambda tr=tr: tr.train_video(aud, vis, lab)) for k, tr in trainers.items()}, rounds)
    out = report("10 x 40x40 step", times, "default", unit_scale=1e3 / (frames // 10), unit="us/sub-batch (incl. the video's upload)")
    out["replays"] = {k: tr.replays for k, tr in trainers.items()}
    # per replay, by phase: device events around every _run of one more video per round
    phases = {}
    for name, tr in trainers.items():
        run = tr._run
        marks = []

        def timed(n, run=run, tr=tr, marks=marks):
            e0 = torch.cuda.Event(enable_timing=True); e1 = torch.cuda.Event(enable_timing=True)
            e0.record(); run(n); e1.record()
            marks.append((tr._phase[1], e0, e1))
        tr._run = timed
        for _ in range(rounds):
            tr.train_video(aud, vis, lab)
        torch.cuda.synchronize()
        tr._run = run
        for last in (False, True):
            ts = [e0.elapsed_time(e1) * 1e3 for ph, e0, e1 in marks if ph is last]
            if ts:
                label = "final" if last else "non-final"
                phases.setdefault(name, {})[label] = {"median_us": statistics.median(ts), "min_us": min(ts), "max_us": max(ts), "replays": len(ts)}
                print(f"10 x 40x40 step, {name:14s} {label:10s} micro-step: {statistics.median(ts):8.1f} us ({min(ts):.1f}-{max(ts):.1f}) over {len(ts)} replays",
                      flush=True)
    out["per_replay_by_phase"] = phases
    return out


def main():
    args = sys.argv[1:]
    if args and args[0] == "--child":
        res = globals()[args[1]](int(args[2]))
        with open(args[3], "w") as f:
            json.dump(res, f)
        return
    out_path = os.path.join(ROOT, "profiles", "accum_bench.json")
    if "--out" in args:
        i = args.index("--out")
        out_path = os.path.abspath(args[i + 1])
        del args[i:i + 2]
    rounds = int(args[0]) if args else 5
    parts = args[1:] or PARTS
    print(f"{rounds} alternations", flush=True)
    result = {"script": "scripts/bench_accum.py", "rounds": rounds}
    for r in parts:
        if r not in PARTS:
            sys.exit(f"unknown part {r!r}: one of {PARTS}")
        with tempfile.TemporaryDirectory() as tmp:
            piece = os.path.join(tmp, "part.json")
            rc = subprocess.run([sys.executable, os.path.abspath(__file__), "--child", r, str(rounds), piece], timeout=CHILD_TIMEOUT_S).returncode
            if rc != 0:
                sys.exit(f"part {r}: child exited with {rc}; nothing more is started")
            with open(piece) as f:
                result[r] = json.load(f)
        with open(out_path, "w") as f:              # after every part: what has been measured so far is kept
            json.dump(result, f, indent=1)
            f.write("\n")
    print(f"wrote {out_path}", flush=True)


if __name__ == "__main__":
    main()
