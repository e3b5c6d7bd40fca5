"""Optimizer options on the fused step: what they cost, variants alternating in one process, device events.

    python scripts/bench_optim.py [rounds=5] [part ...]

Parts:
  kernels40, kernels224   the arena of the 40 x 40 / 224 x 224 model (23.5 M / 1.29 G parameters): goalnet_adam_step_dev_ranges against
                          goalnet_optim_step_dev_ranges with options off, with decoupled decay + clipping + cosine, and goalnet_grad_sumsq
                          alone. The step moves 28 B per parameter either way, the norm reads 4 B.
  step10                  the 10-frame step at 40 x 40 as loop.VideoTrainer replays it (HIP graphs, 100-frame video), default against
                          options on (decoupled decay, no_decay on biases and BatchNorm, clipping, warm-up + cosine)
  step1024                the fp32 step of 1 024 frames at 224 x 224, default (linear5.weight updated in its weight-gradient epilogue)
                          against options on (one norm pass and one update pass over the arena after backward)

Each part runs in a child process of its own under a time limit; the parent never touches the GPU and stops at the first child that
fails. Every turn is the median of three timed calls after one untimed call; printed are median and min-max over the rounds and the
ratio of the medians. The ratio is reported, not gated."""
import os, statistics, subprocess, sys
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

PARTS = ("kernels40", "kernels224", "step10", "step1024")
CHILD_TIMEOUT_S = 420


def timeit(torch, fn, reps=3):
    fn(); torch.cuda.synchronize()
    e0 = torch.cuda.Event(enable_timing=True); e1 = torch.cuda.Event(enable_timing=True)
    ts = []
    for _ in range(reps):
        e0.record(); fn(); e1.record(); torch.cuda.synchronize()
        ts.append(e0.elapsed_time(e1))
    return statistics.median(ts)


def alternate(torch, variants, rounds):
    """{name: fn} -> {name: [ms per round]}, the variants taking turns inside every round"""
    out = {k: [] for k in variants}
    for _ in range(rounds):
        for k, fn in variants.items():
            out[k].append(timeit(torch, fn))
    return out


def report(title, times, base, unit_scale=1.0, unit="ms", extra=None):
    mb = statistics.median(times[base])
    for k, ts in times.items():
        m = statistics.median(ts)
        note = "" if extra is None or k not in extra else f" | {extra[k](m)}"
        print(f"{title:22s} {k:34s} {m * unit_scale:10.3f} {unit} ({min(ts) * unit_scale:.3f}-{max(ts) * unit_scale:.3f}) | x{m / mb:.3f} of {base}{note}",
              flush=True)


def _options(max_norm=1.0):
    from cvml_goalnet_amd.optim import OptimOptions
    return OptimOptions(weight_decay=0.01, decoupled=True, no_decay=("bias", "bnorm"), max_grad_norm=max_norm, schedule="cosine", warmup_steps=2,
                        total_steps=1000)


def kernels(n, rounds, title):
    import torch
    from cvml_goalnet_amd import ops
    from cvml_goalnet_amd.optim import OptimOptions
    dev = "cuda:0"
    p = torch.randn(n, device=dev) * 0.01; g = torch.randn(n, device=dev) * 1e-3
    m = torch.zeros(n, device=dev); v = torch.zeros(n, device=dev)
    step = torch.zeros(1, dtype=torch.int64, device=dev)
    hyper = (1e-3, 0.9, 0.999, 1e-8)
    ss = ops.grad_sumsq(g, [(0, n, 0, False)])
    on = _options()
    times = alternate(torch, {
        "adam_step_dev_ranges": lambda: ops.adam_step_dev_ranges(p, g, m, v, [(0, n, 0)], *hyper, step),
        "optim_step_dev_ranges, options off": lambda: ops.optim_step_dev_ranges(p, g, m, v, [(0, n, 0, False)], *hyper, OptimOptions(), step),
        "optim_step_dev_ranges, options on": lambda: ops.optim_step_dev_ranges(p, g, m, v, [(0, n, 0, True)], *hyper, on, step, sumsq=ss),
        "grad_sumsq": lambda: ops.grad_sumsq(g, [(0, n, 0, False)], out=ss),
    }, rounds)
    gbs = {k: (lambda ms, b=(4 if k == "grad_sumsq" else 28): f"{n * b / ms / 1e6:7.0f} GB/s") for k in times}
    report(f"{title} ({n / 1e6:.1f} M)", times, "adam_step_dev_ranges", extra=gbs)


def kernels40(rounds):
    kernels(23482433 // 4 * 4, rounds, "arena 40x40")


def kernels224(rounds):
    kernels(1286754368, rounds, "arena 224x224")


def step10(rounds):
    import torch
    from cvml_goalnet_amd import AVM, synth
    from cvml_goalnet_amd.loop import VideoTrainer
    dev = "cuda:0"
    frames = 100
    aud = torch.from_numpy(synth.make_audio(frames)); vis = torch.from_numpy(synth.make_visual(frames, 40, 40))
    lab = torch.from_numpy(synth.make_labels(frames))
    probe = AVM(audio_included=True, device=dev, seed=synth.BASE_SEED)
    probe.train_step(aud[:10].to(dev), vis[:10].to(dev), lab[:10].to(dev))
    half = 0.5 * probe.grad_norm().item()
    trainers = {}
    for name, opt in (("default", None), ("options on", _options(half))):
        tr = VideoTrainer(AVM(audio_included=True, device=dev, seed=synth.BASE_SEED), subbatch_size=10, optim=opt)
        tr.train_video(aud, vis, lab)               # eager step, capture, replays
        trainers[name] = tr
    times = alternate(torch, {k: (lambda tr=tr: tr.train_video(aud, vis, lab)) for k, tr in trainers.items()}, rounds)
    report("10 x 40x40 step", times, "default", unit_scale=1e3 / (frames // 10), unit="us/step (incl. the video's upload)")
    print(f"replays: { {k: tr.replays for k, tr in trainers.items()} }", flush=True)


def step1024(rounds):
    import torch
    from cvml_goalnet_amd import AVM, synth
    dev = "cuda:0"
    n, h = 1024, 224
    g = torch.Generator(device=dev).manual_seed(1)
    vis = torch.rand(n, 3, h, h, device=dev, generator=g); aud = torch.rand(n, 30, 30, device=dev, generator=g) - 0.5
    lab = torch.rand(n, device=dev, generator=g) * 4 + 1
    models = {"default": (AVM(audio_included=True, device=dev, seed=synth.BASE_SEED), None),
              "options on": (AVM(audio_included=True, device=dev, seed=synth.BASE_SEED), _options(1.0))}
    variants = {k: (lambda m=m, o=o: m.train_step(aud, vis, lab, optim=o)) for k, (m, o) in models.items()}
    for fn in variants.values():
        fn(); fn()
    times = alternate(torch, variants, rounds)
    report("1024 x 224x224 fp32 step", times, "default")
    print(f"epilogue-fused steps: { {k: m.epi_fused_dw for k, (m, _) in models.items()} }", flush=True)


def main():
    args = sys.argv[1:]
    if args and args[0] == "--child":
        globals()[args[1]](int(args[2]))
        return
    rounds = int(args[0]) if args else 5
    parts = args[1:] or PARTS
    print(f"{rounds} alternations", flush=True)
    for r in parts:
        if r not in PARTS:
            sys.exit(f"unknown part {r!r}: one of {PARTS}")
        rc = subprocess.run([sys.executable, os.path.abspath(__file__), "--child", r, str(rounds)], timeout=CHILD_TIMEOUT_S).returncode
        if rc != 0:
            sys.exit(f"part {r}: child exited with {rc}; nothing more is started")


if __name__ == "__main__":
    main()
