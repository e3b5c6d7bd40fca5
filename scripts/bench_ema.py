"""The weight average behind the fused step: what it costs, variants alternating in one process, device events.

    python scripts/bench_ema.py [rounds=5] [--out profiles/ema_bench.json] [part ...]

Parts:
  kernels40, kernels224   the arena of the 40 x 40 / 224 x 224 model (23.5 M / 1.29 G parameters): goalnet_ema_update_dev_ranges beside
                          goalnet_adam_step_dev and goalnet_swap_ranges. The average moves 12 B per parameter, Adam 28, the swap 16.
  step10                  the 10-frame step at 40 x 40 as loop.VideoTrainer replays it (HIP graphs, 100-frame video): without ema=, with
                          every = 1 and with every = 8; and the C-ABI calls of one eager step with and without the average
  step1024                the fp32 step of 1 024 frames at 224 x 224 (linear5.weight updated in its weight-gradient epilogue either way):
                          without ema=, with every = 1 and with every = 8

Each part runs in a child process of its own under a time limit; the parent never touches the GPU and stops at the first child that
fails. Every turn is the median of three timed calls after one untimed call; recorded are median and min-max over the rounds and the
ratio of the medians. The kernel-level condition — the average's pass takes no longer than the Adam pass measured in the same run —
is recorded as `ema_no_slower_than_adam`; the rest is reported, not gated."""
import collections, json, os, statistics, subprocess, sys, tempfile
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
    rows = {}
    for k, ts in times.items():
        m = statistics.median(ts)
        note = "" if extra is None or k not in extra else f" | {extra[k](m)}"
        print(f"{title:26s} {k:30s} {m * unit_scale:10.3f} {unit} ({min(ts) * unit_scale:.3f}-{max(ts) * unit_scale:.3f}) | x{m / mb:.3f} of {base}{note}",
              flush=True)
        rows[k] = {"median": m * unit_scale, "min": min(ts) * unit_scale, "max": max(ts) * unit_scale, "ratio_to_" + base.replace(" ", "_"): m / mb}
    return {"unit": unit, "rounds": len(times[base]), "variants": rows}


def kernels(n, rounds, title):
    import torch
    from cvml_goalnet_amd import ops
    from cvml_goalnet_amd.optim import EmaOptions
    dev = "cuda:0"
    p = torch.randn(n, device=dev) * 0.01; g = torch.randn(n, device=dev) * 1e-3
    m = torch.zeros(n, device=dev); v = torch.zeros(n, device=dev); e = p.clone()
    step = torch.zeros(1, dtype=torch.int64, device=dev)
    ema = EmaOptions(decay=0.999)
    times = alternate(torch, {
        "adam_step_dev": lambda: ops.adam_step_dev(p, g, m, v, 1e-3, 0.9, 0.999, 1e-8, step, step_bias=1),
        "ema_update_dev_ranges": lambda: ops.ema_update_dev_ranges(p, e, [(0, n)], ema, step),
        "swap_ranges": lambda: ops.swap_ranges(p, e, [(0, n)]),
    }, rounds)
    per = {"adam_step_dev": 28, "ema_update_dev_ranges": 12, "swap_ranges": 16}
    gbs = {k: (lambda ms, b=per[k]: f"{n * b / ms / 1e6:7.0f} GB/s") for k in times}
    out = report(f"{title} ({n / 1e6:.1f} M)", times, "adam_step_dev", extra=gbs)
    for k, row in out["variants"].items():
        row["GB_per_s"] = n * per[k] / row["median"] / 1e6
    out["parameters"] = n
    out["ema_no_slower_than_adam"] = out["variants"]["ema_update_dev_ranges"]["median"] <= out["variants"]["adam_step_dev"]["median"]
    print(f"{title}: the average's pass takes no longer than Adam's: {out['ema_no_slower_than_adam']}", flush=True)
    return out


def kernels40(rounds):
    return kernels(23482433 // 4 * 4, rounds, "arena 40x40")


def kernels224(rounds):
    return kernels(1286754368, rounds, "arena 224x224")


class _Counting:
    """libgoalnet_hip.so with every entry point counted by name"""

    def __init__(self, lib):
        self._lib, self.calls = lib, collections.Counter()

    def __getattr__(self, name):
        fn = getattr(self._lib, name)
        if not name.startswith("goalnet_") or name.endswith(("_ws_bytes", "_last_error", "_abi_version", "_ok", "_name", "_blocks", "_parts", "_layout")):
            return fn

        def counted(*a):
            self.calls[name] += 1
            return fn(*a)
        return counted


def _abi_calls(torch, ema):
    """C-ABI calls of the SECOND eager 10-frame train_step (the first allocates), by name"""
    from cvml_goalnet_amd import AVM, _lib, synth
    dev = "cuda:0"
    m = AVM(audio_included=True, device=dev, seed=synth.BASE_SEED)
    aud = torch.from_numpy(synth.make_audio(10)).to(dev); vis = torch.from_numpy(synth.make_visual(10, 40, 40)).to(dev)
    lab = torch.from_numpy(synth.make_labels(10)).to(dev)
    kw = {} if ema is None else {"ema": ema}
    m.train_step(aud, vis, lab, **kw)
    real = _lib.load()
    _lib._lib = counting = _Counting(real)
    try:
        m.train_step(aud, vis, lab, **kw)
    finally:
        _lib._lib = real
    torch.cuda.synchronize()
    return counting.calls


def step10(rounds):
    import torch
    from cvml_goalnet_amd import AVM, synth
    from cvml_goalnet_amd.loop import VideoTrainer
    from cvml_goalnet_amd.optim import EmaOptions
    dev = "cuda:0"
    frames = 100
    aud = torch.from_numpy(synth.make_audio(frames)); vis = torch.from_numpy(synth.make_visual(frames, 40, 40))
    lab = torch.from_numpy(synth.make_labels(frames))
    trainers = {}
    for name, ema in (("default", None), ("ema every 1", EmaOptions(0.999)), ("ema every 8", EmaOptions(0.999, every=8))):
        tr = VideoTrainer(AVM(audio_included=True, device=dev, seed=synth.BASE_SEED), subbatch_size=10, ema=ema)
        tr.train_video(aud, vis, lab)               # eager step, capture, replays
        trainers[name] = tr
    times = alternate(torch, {k: (lambda tr=tr: tr.train_video(aud, vis, lab)) for k, tr in trainers.items()}, rounds)
    out = report("10 x 40x40 step", times, "default", unit_scale=1e3 / (frames // 10), unit="us/step (incl. the video's upload)")
    out["replays"] = {k: tr.replays for k, tr in trainers.items()}
    off, on = _abi_calls(torch, None), _abi_calls(torch, EmaOptions(0.999))
    out["abi_calls_per_eager_step"] = {"default": sum(off.values()), "ema every 1": sum(on.values()),
                                       "added": {k: on[k] - off[k] for k in sorted(set(on) | set(off)) if on[k] != off[k]}}
    print(f"replays: {out['replays']}; C-ABI calls of one eager step: {out['abi_calls_per_eager_step']}", flush=True)
    return out


def step1024(rounds):
    import torch
    from cvml_goalnet_amd import AVM, synth
    from cvml_goalnet_amd.optim import EmaOptions
    dev = "cuda:0"
    n, h = 1024, 224
    g = torch.Generator(device=dev).manual_seed(1)
    vis = torch.rand(n, 3, h, h, device=dev, generator=g); aud = torch.rand(n, 30, 30, device=dev, generator=g) - 0.5
    lab = torch.rand(n, device=dev, generator=g) * 4 + 1
    models = {k: (AVM(audio_included=True, device=dev, seed=synth.BASE_SEED), e)
              for k, e in (("default", None), ("ema every 1", EmaOptions(0.999)), ("ema every 8", EmaOptions(0.999, every=8)))}
    variants = {k: (lambda m=m, e=e: m.train_step(aud, vis, lab, **({} if e is None else {"ema": e}))) for k, (m, e) in models.items()}
    for fn in variants.values():
        fn(); fn()
    times = alternate(torch, variants, rounds)
    out = report("1024 x 224x224 fp32 step", times, "default")
    out["epilogue_fused_steps"] = {k: m.epi_fused_dw for k, (m, _) in models.items()}
    print(f"epilogue-fused steps: {out['epilogue_fused_steps']}", flush=True)
    return out


def main():
    args = sys.argv[1:]
    if args and args[0] == "--child":
        res = globals()[args[1]](int(args[2]))
        with open(args[3], "w") as f:
            json.dump(res, f)
        return
    out_path = os.path.join(ROOT, "profiles", "ema_bench.json")
    if "--out" in args:
        i = args.index("--out")
        out_path = os.path.abspath(args[i + 1])
        del args[i:i + 2]
    rounds = int(args[0]) if args else 5
    parts = args[1:] or PARTS
    print(f"{rounds} alternations", flush=True)
    result = {"script": "scripts/bench_ema.py", "rounds": rounds}
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
