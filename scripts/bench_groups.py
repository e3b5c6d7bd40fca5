"""Parameter groups and AMSGrad on the fused step: what the launch over a table of hyper-parameters costs next to the
single-rate launch it grew from, variants alternating in one process, device events.

    python scripts/bench_groups.py [rounds=5] [part ...]

Parts:
  kernels40, kernels224   the arena of the 40 x 40 / 224 x 224 model (23.5 M / 1.29 G parameters), under decoupled decay, clipping and a
                          cosine schedule:
                            optim_step_dev_ranges                 goalnet_optim_step_dev_ranges, the base
                            optim_step_dev_ranges (again)         the same launch a second time in every round: its own run-to-run spread
                            optim_step_dev_ranges, three ranges   the base over the three ranges of "three groups": what the cut alone costs
                            group step, default group only        goalnet_group_step_dev_ranges, one row, one range
                            group step, three groups              three ranges under three rows (rates, betas, eps, decay of their own)
                            group step, AMSGrad everywhere        one row with amsgrad: the fourth arena, 36 B per parameter instead of 28

Each part runs in a child process of its own under a time limit; the parent never touches the GPU and stops at the first child that
fails (kernels224 needs 5 x 5.1 GB; a card that cannot hold it ends that part, not the run). Every turn is the median of three timed
calls after one untimed call; printed are median and min-max over the rounds, GB/s from the bytes the variant moves, and the ratio of
the medians to the base. The ratios are reported, not gated."""
import os, statistics, subprocess, sys
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

PARTS = ("kernels40", "kernels224")
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


def report(title, times, base, nbytes):
    mb = statistics.median(times[base])
    for k, ts in times.items():
        m = statistics.median(ts)
        print(f"{title:24s} {k:36s} {m:10.3f} ms ({min(ts):.3f}-{max(ts):.3f}) | {nbytes[k] / m / 1e6:7.0f} GB/s | x{m / mb:.3f} of {base}", flush=True)


def kernels(n, rounds, title):
    import torch
    from cvml_goalnet_amd import ops
    from cvml_goalnet_amd.optim import OptimOptions
    dev = "cuda:0"
    p = torch.randn(n, device=dev) * 0.01; g = torch.randn(n, device=dev) * 1e-3
    m = torch.zeros(n, device=dev); v = torch.zeros(n, device=dev); vmax = torch.zeros(n, device=dev)
    step = torch.zeros(1, dtype=torch.int64, device=dev)
    hyper = (1e-3, 0.9, 0.999, 1e-8)
    ss = ops.grad_sumsq(g, [(0, n, 0, False)])
    on = OptimOptions(weight_decay=0.01, decoupled=True, max_grad_norm=1.0, schedule="cosine", warmup_steps=2, total_steps=1000)
    one = [(*hyper, 0.01, False)]
    three = [(*hyper, 0.01, False), (1e-4, 0.9, 0.999, 1e-8, 0.01, False), (1e-2, 0.8, 0.5, 1e-6, 0.05, False)]
    a, b = n // 3 // 64 * 64, 2 * n // 3 // 64 * 64               # three ranges that tile the arena, aligned like the model's slots
    thirds = [(0, a, 0, True, 0), (a, b - a, 0, True, 1), (b, n - b, 0, True, 2)]

    def base():
        ops.optim_step_dev_ranges(p, g, m, v, [(0, n, 0, True)], *hyper, on, step, sumsq=ss)
    times = alternate(torch, {
        "optim_step_dev_ranges": base,
        "optim_step_dev_ranges (again)": base,
        "optim_step_dev_ranges, three ranges": lambda: ops.optim_step_dev_ranges(p, g, m, v, [r[:4] for r in thirds], *hyper, on, step, sumsq=ss),
        "group step, default group only": lambda: ops.group_step_dev_ranges(p, g, m, v, None, [(0, n, 0, True, 0)], one, on, step, sumsq=ss),
        "group step, three groups": lambda: ops.group_step_dev_ranges(p, g, m, v, None, thirds, three, on, step, sumsq=ss),
        "group step, AMSGrad everywhere": lambda: ops.group_step_dev_ranges(p, g, m, v, vmax, [(0, n, 0, True, 0)], [(*hyper, 0.01, True)], on, step,
                                                                           sumsq=ss),
    }, rounds)
    report(f"{title} ({n / 1e6:.1f} M)", times, "optim_step_dev_ranges", {k: n * (36 if "AMSGrad" in k else 28) for k in times})
    both = times["optim_step_dev_ranges"] + times["optim_step_dev_ranges (again)"]
    print(f"{title}: the base launch's own spread over {len(both)} turns: {min(both):.3f}-{max(both):.3f} ms "
          f"(+-{(max(both) - min(both)) / 2 / statistics.median(both) * 100:.2f} % of its median)", flush=True)


def kernels40(rounds):
    kernels(23482433 // 4 * 4, rounds, "arena 40x40")


def kernels224(rounds):
    kernels(1286754368, rounds, "arena 224x224")


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
