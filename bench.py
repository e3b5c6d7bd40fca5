#!/usr/bin/env python3
"""bench.py — training clips/s of the AVM hot path on MI355X (BASELINE.json metric), one JSON line on stdout.

    python bench.py --gpus 1 --steps K --warmup W [--dump-outputs DIR] [--full]
    python -m torch.distributed.run --nnodes=1 --nproc-per-node N --master-addr 127.0.0.1 --master-port P \
        bench.py --gpus N --steps K --warmup W

A plain run sets up, runs W warm-up steps, times exactly K steps and prints the headline (`metric`, `value`, `unit`,
`higher_is_better`, `dtype`, `ms_per_step`, `config`). Everything else on the line below — roofline and per-kernel figures with
their counter passes, parity, cpu_baseline, the other precisions, the 40x40 loop, the drop-in path, comm — is measured only
with --full (the --no-* options then leave parts of it out). --dump-outputs DIR writes what the last timed step returned
(loss.npy, pred.npy, float32) from rank 0; the inputs are seeded, so two builds run with the same arguments can be compared
output for output. --full runs the parity probe's forward before the timed steps, which draws one set of dropout masks: its
outputs are comparable with other --full runs, not with plain ones.

A step = one pass of the hot path over one batch of synthetic input: forward, broadcast-MSE, backward and the
fused Adam of `AVM` (/root/reference/main.py:187-193) on 64 clips x 16 frames = 1024 frames of 3x224x224 (+ a
30x30 MFCC each) per GPU — the configuration BASELINE.json's metric is quoted on. Inputs are resident in HBM
before the timed region. N > 1 is weak scaling: every rank trains its own 64 clips (local BatchNorm, local
MSE, as an independent reference process would), gradients are summed over RCCL/xGMI in three buckets
overlapped with backward and averaged inside the fused Adam (cvml_goalnet_amd/ddp.py).

The headline (`value`, `dtype`, `roofline`) is the REFERENCE'S PRECISION: `--dtype f32` (default), every contraction on
the fp32 matrix cores (`v_mfma_f32_32x32x2_f32`), timed over the full --steps / --warmup. The reduced-precision engine
(bf16 MFMA contractions, fp32 accumulation / statistics / master weights / Adam; an extension — the reference has no such
mode) is measured with --full in the same run, with the same K / W, and reported beside it as `bf16_path`.

Objects on the JSON line of a --full run:
  roofline      the dominant kernel = the implicit-GEMM convolution forward (conv2 + conv3, 84 % of forward MACs):
                algorithmic flops of its launches / their duration, measured with HIP events inside the timed steps;
                peak = 157.3 TFLOP/s (fp32 MFMA) / 2 500 TFLOP/s (dense bf16 MFMA), MI355X_MICROARCH.md. `kernel` is
                the template the library's dispatcher selects for these dims (goalnet_conv3x3_fwd*_kernel_name);
                `traffic` is measured in the same run: before this process touches the GPU it runs the two convolutions
                under `rocprofv3 --pmc FETCH_SIZE` and `--pmc WRITE_SIZE` (separate passes; scripts/conv_fwd_probe.py) and
                reports (2 FETCH + WRITE) x 1024 bytes per launch; --no-live-traffic falls back to the committed
                profiles/conv_fwd_traffic_<dtype>.json (only while the kernel sources still hash to what was profiled).
  cpu_baseline  the oracle (CPU restatement of the reference, oracle/avm_ref.py) timed on this host's cores on a
                bounded sample (1 clip = 16 frames of 224x224 per step), rank 0, N = 1 only.
  parity        pre-sigmoid logit MAE / max-abs of the HIP forward vs that CPU reference on the same 32 frames (n > 16: the
                branch the timed step runs), weights and dropout masks: on the random-init weights before the first
                optimizer step, and again on the weights the W + K steps left.
  bf16x6_path  (N = 1, --dtype f32) the SAME fp32 step with conv2's forward and conv3's forward / data gradient / weight gradient on split
                operands (precision="bf16x6", csrc/split3.hip: every fp32 operand value as a bf16 triple hi + mid + lo, six partial
                products per product on the 16-bit MFMA, fp32 accumulation): fp32-grade results — held to the fp32 engine's parity
                criteria by tests/test_gpu_bench_shapes.py — at the 16-bit MFMA's rate. roofline.achieved counts the 6 x MFMA flops
                against the 16-bit peak; useful_tflops the convolution's own flops. NOT the headline: `value` stays on the fp32 MFMA.
  bf16_path, fp16_path  (N = 1, --dtype f32) ms_per_step, clips_per_s, roofline, other_kernels, parity of precision="bf16" / "fp16"
                (the same 16-bit engine with bfloat16 / IEEE binary16 storage; fp16 adds a loss scale and an overflow guard).
  comm          (N > 1) ranks, exchange mode, bytes per bucket, a stand-alone all-reduce of bucket 1 (algorithm bandwidth)
                and the exposed (non-overlapped) wait per step, max over ranks.
  dropin_path   /root/reference/main.py:187-196 verbatim on this AVM (CPU tensors, nn.MSELoss, stock optim.Adam) at 40x40 / N = 10 and at
                224x224 / N = 64, us per step, with the fused device-resident step beside it.
  native_40x40_loop  SURVEY.md §8(d) "report additionally frames/s at the reference-native 40x40": the reference's own
                operating point (main.py:169-198: one video at a time, 10 frames per optimizer step, fp32), run by
                loop.VideoTrainer as one HIP-graph launch per sub-batch, with the CPU oracle's step beside it; N = 1 only.
"""
from __future__ import annotations

import argparse
import hashlib
import json
import os
import re
import sys
import time

import torch

ROOT = os.path.dirname(os.path.abspath(__file__))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

FP32_MFMA_PEAK_TFLOPS = 157.3   # MI355X_MICROARCH.md, chip-level parameters
BF16_MFMA_PEAK_TFLOPS = 2500.0  # dense bf16 MFMA (not the 2:1-sparsity marketing figure)
FRAMES_PER_CLIP = 16
PROBE_FRAMES = 32               # > 16: AVM.forward_device's bf16 linear5 / p3 / y3 branches, i.e. what the timed step runs

# the source files each conv-forward kernel is built from: roofline.traffic is only as current as these
KERNEL_SOURCES = {
    "f32": ["gemm_f32.hip", "gemm_common.h", "common.h"],
    "bf16": ["gemm_bf16_256.hip", "gemm_bf16.hip", "gemm_bf16_common.h", "gemm_common.h", "common.h"],
}


def log(*a):
    print(*a, file=sys.stderr, flush=True)


def kernel_sources_sha(dtype):
    h = hashlib.sha256()
    for f in KERNEL_SOURCES[dtype]:
        h.update(open(os.path.join(ROOT, "cvml_goalnet_amd", "csrc", f), "rb").read())
    return h.hexdigest()[:16]


def _norm(name):
    return re.sub(r"\s+|\(anonymous namespace\)::|goalnet::", "", name or "")


def conv_fwd_kernel(dtype, n, h, w):
    """The kernel template the library dispatches conv3's forward to at this size (conv2 takes the same template)."""
    from cvml_goalnet_amd import AVM, ops
    (_, _), _, (hp2, wp2), _ = AVM._sizes(h, w)
    lib = ops.lib()
    if dtype == "bf16":
        raw = lib.goalnet_conv3x3_fwd_bf16p_kernel_name(n, hp2, wp2, 256, 512, 1).decode()
        base = "gemm_bf16_256_kernel" if "256" in raw.split("[")[0] else "gemm_bf16_kernel"
    else:
        raw = lib.goalnet_conv3x3_fwd_kernel_name(n, hp2, wp2, 256, 512, 1).decode()
        base = "gemm_f32_kernel"
    m = re.search(r"\[(.*)\]", raw)
    args = [a.split("=", 1)[1].strip() for a in m.group(1).split(", ") if "=" in a] if m else []
    args = [a.replace("(anonymous namespace)::", "").replace("goalnet::", "") for a in args]
    return f"{base}<{', '.join(args)}>"


_LIVE_TRAFFIC = {}      # dtype -> (bytes per launch, source) measured by live_traffic() at the start of this run


def live_traffic(dtype, clips, h, timeout=300):
    """HBM bytes per launch of the conv2 + conv3 forward kernels, measured NOW: two rocprofv3 passes (--pmc FETCH_SIZE, --pmc
    WRITE_SIZE: they do not fit one pass) over scripts/conv_fwd_probe.py, which launches exactly those two convolutions at the
    bench shape. bytes = (2 x FETCH_SIZE + WRITE_SIZE) x 1024 (gfx950: FETCH_SIZE reports half of a wide coalesced read stream,
    MI355X_MICROARCH.md "HBM"). Must run BEFORE this process touches the GPU (the profiler is a child process). Returns
    (bytes, source) or (None, why)."""
    import csv
    import glob
    import shutil
    import subprocess
    import tempfile
    exe = shutil.which("rocprofv3") or "/opt/rocm/bin/rocprofv3"
    if not os.path.exists(exe):
        return None, "rocprofv3 not found"
    vals = {}
    tmp = tempfile.mkdtemp(prefix="goalnet_pmc_", dir="/tmp")
    env = dict(os.environ, TMPDIR="/tmp")
    try:
        for ctr in ("FETCH_SIZE", "WRITE_SIZE"):
            out = os.path.join(tmp, ctr)
            cmd = [exe, "--pmc", ctr, "--output-format", "csv", "-d", out, "--", sys.executable, os.path.join(ROOT, "scripts", "conv_fwd_probe.py"),
                   "--dtype", dtype, "--frames", str(clips * FRAMES_PER_CLIP), "--hw", str(h), "--reps", "2"]
            r = subprocess.run(cmd, cwd="/tmp", env=env, capture_output=True, text=True, timeout=timeout)
            if r.returncode != 0:
                return None, f"rocprofv3 --pmc {ctr} failed (rc {r.returncode}): {r.stderr.strip()[-200:]}"
            per = []
            for f in glob.glob(os.path.join(out, "**", "*_counter_collection.csv"), recursive=True):
                for row in csv.DictReader(open(f)):
                    if row.get("Counter_Name") == ctr and "gemm_" in row.get("Kernel_Name", ""):
                        per.append(float(row["Counter_Value"]))
            if not per:
                return None, f"no {ctr} rows for the convolution kernels in the profiler's output"
            vals[ctr] = (sum(per) / len(per), len(per))
    except Exception as e:
        return None, f"live counter pass failed: {e!r}"
    finally:
        shutil.rmtree(tmp, ignore_errors=True)
    fe, wr = vals["FETCH_SIZE"][0], vals["WRITE_SIZE"][0]
    return (2 * fe + wr) * 1024, (f"measured in this run: rocprofv3 --pmc FETCH_SIZE / --pmc WRITE_SIZE (separate passes) over scripts/conv_fwd_probe.py, "
                                 f"{vals['FETCH_SIZE'][1]} launches, FETCH_SIZE avg {fe:.0f} KiB, WRITE_SIZE avg {wr:.0f} KiB, bytes = (2 FETCH + WRITE) x 1024")


def traffic_of(dtype, kernel, clips, h):
    """HBM bytes per launch of `kernel`: this run's own counter passes (live_traffic), else the committed --pmc summary, or (None, why)."""
    if dtype in _LIVE_TRAFFIC and _LIVE_TRAFFIC[dtype][0] is not None:
        return _LIVE_TRAFFIC[dtype]
    tj = os.path.join(ROOT, "profiles", f"conv_fwd_traffic_{dtype}.json")
    if not (os.path.exists(tj) and clips == 64 and h == 224):
        return None, "no counter summary for this workload"
    try:
        j = json.load(open(tj))
    except Exception as e:
        return None, f"unreadable {tj}: {e!r}"
    if _norm(j.get("kernel")) != _norm(kernel):
        return None, f"counter summary is for {j.get('kernel')!r}, the dispatcher now selects {kernel!r}"
    if j.get("sources_sha256") != kernel_sources_sha(dtype):
        return None, "kernel sources changed since the counter passes (re-run scripts/profile_bench.sh pmc)"
    return j.get("hbm_bytes_per_launch"), f"{j.get('source')} @ {j.get('git_head')}"


def make_inputs(n, h, w, device, seed):
    from cvml_goalnet_amd import ops, synth
    vis = torch.empty(n, 3, h, w, device=device)
    ops.fill_uniform(vis.view(-1), seed, synth.TID_VISUAL, 0.0, 1.0)
    flat = vis.view(n, -1)
    mn = flat.amin(dim=1, keepdim=True)
    mx = flat.amax(dim=1, keepdim=True)
    flat.sub_(mn).div_(mx - mn)                      # per-frame min-max to [0,1], as utils.py:284 (data prep, untimed)
    aud = torch.from_numpy(synth.make_audio(n, 30, seed)).to(device)
    lab = torch.from_numpy(synth.make_labels(n, seed)).to(device)
    return aud, vis, lab


def logit_parity(model, h, w, seed):
    """Logits of the HIP forward vs the CPU oracle on the same PROBE_FRAMES frames, weights and dropout masks (regenerated
    from the seed formula on both sides); BatchNorm in train mode. The probe restores the model's BatchNorm buffers."""
    from cvml_goalnet_amd import synth
    from oracle import avm_ref
    n = PROBE_FRAMES
    aud, vis, lab = make_inputs(n, h, w, model._device, seed + 1)
    if not model.audio_included:
        aud = None
    if not model._materialized:
        with torch.no_grad():
            model.forward_device(aud, vis, save=False)               # Lazy parameters take their random init here
        for i in (1, 2, 3):                                          # ... and the buffers go back to their initial state
            bn = getattr(model.visbl, f"bnorm{i}")
            bn.running_mean.zero_(); bn.running_var.fill_(1.0); bn.num_batches_tracked.zero_()
    sd = model.state_dict()                                          # torch-native layouts, CPU
    p = {k: v for k, v in sd.items() if v.is_floating_point() and "running" not in k}
    b = {k: v.clone() for k, v in sd.items() if k not in p}
    step = model._drop_step
    masks = [torch.from_numpy(m) for m in synth.make_drop_masks(n, seed=model.dropout_seed, step=step)]
    bn_backup = {k: getattr(*model._module_of(k)).clone() for k in b}
    with torch.no_grad():
        model.forward_device(aud, vis, save=False)
    hip_logit = model.last_logit.cpu()
    for k, v in bn_backup.items():                                   # the parity probe must not disturb the model
        getattr(*model._module_of(k)).copy_(v)
    inter = {}
    with torch.no_grad():
        avm_ref.forward(p, {k: v.clone() for k, v in b.items()}, None if aud is None else aud.cpu(), vis.cpu(), masks,
                        model.audio_included, inter)
    ref_logit = inter["logit"].view(-1)
    d = (hip_logit - ref_logit).abs()
    mx = ref_logit.abs().max().item()
    return {"logit_mae_vs_cpu_ref": d.mean().item(), "logit_maxabs_vs_cpu_ref": d.max().item(),
            "max_abs_logit": mx, "frames": n,
            "criterion": "absolute: max-abs logit error <= 1e-3 (BASELINE.json north star; |logit| <= 1 here)" if mx <= 1.0 else
                         "relative: max-abs logit error <= 1e-3 of max|logit| (|logit| > 1: an absolute 1e-3 is below the 16-bit formats' resolution of the logit itself)",
            "criterion_met": bool(d.max().item() <= 1e-3 * max(1.0, mx))}


def host_cpu_info():
    """CPU model string, physical cores (distinct (socket, core id) pairs) and hardware threads of this host, from /proc/cpuinfo"""
    model, cores, phys, core = None, set(), None, None
    try:
        for line in open("/proc/cpuinfo"):
            k, _, v = line.partition(":")
            k, v = k.strip(), v.strip()
            if k == "model name" and model is None:
                model = v
            elif k == "physical id":
                phys = v
            elif k == "core id":
                core = v
            elif not k and phys is not None and core is not None:
                cores.add((phys, core))
                phys = core = None
        if phys is not None and core is not None:
            cores.add((phys, core))
    except OSError:
        pass
    return {"cpu_model": model, "physical_cores": len(cores) or None, "hardware_threads": os.cpu_count()}


def cpu_baseline(model, h, w, seed, max_seconds=40.0):
    """Time the oracle's train step on the host cores (bounded sample: one clip per step), and — BASELINE.json config 1 / SURVEY.md
    §8(d) — the oracle's forward alone on one 16-frame clip (utils.py:260-272 under no_grad), with the HIP forward of the same clip."""
    from cvml_goalnet_amd import synth
    from oracle import avm_ref
    n = FRAMES_PER_CLIP
    threads = torch.get_num_threads()
    sd = model.state_dict()
    p = {k: v for k, v in sd.items() if v.is_floating_point() and "running" not in k}
    b = {k: v.clone() for k, v in sd.items() if k not in p}
    aud, vis, lab = make_inputs(n, h, w, model._device, seed + 1)
    a_c, v_c, l_c = aud.cpu(), vis.cpu(), lab.cpu()
    masks = [torch.from_numpy(m) for m in synth.make_drop_masks(n, seed=model.dropout_seed, step=0)]
    # train steps of one clip (the Adam state allocation of the first step is the warm-up)
    state = {}
    times = []
    t_begin = time.time()
    for i in range(3):
        t0 = time.time()
        avm_ref.train_step(p, b, state, a_c if model.audio_included else None, v_c, l_c, masks, model.audio_included)
        times.append(time.time() - t0)
        if time.time() - t_begin > max_seconds:
            break
    t = min(times[1:]) if len(times) > 1 else times[0]
    # config 1: forward only, one clip, on the updated weights (the cost does not depend on their values)
    fts = []
    with torch.no_grad():
        for i in range(3):
            t0 = time.time()
            avm_ref.forward(p, {k: v.clone() for k, v in b.items()}, a_c if model.audio_included else None, v_c, masks, model.audio_included)
            fts.append(time.time() - t0)
    tf = min(fts[1:])
    bn_backup = {k: getattr(*model._module_of(k)).clone() for k in b}
    hts = []
    with torch.no_grad():
        for i in range(4):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            model.forward_device(aud if model.audio_included else None, vis, save=False)
            torch.cuda.synchronize()
            hts.append(time.perf_counter() - t0)
    for k, v in bn_backup.items():
        getattr(*model._module_of(k)).copy_(v)
    info = host_cpu_info()
    out = {"value": (n / FRAMES_PER_CLIP) / t, "unit": "clips/s", "cores": threads, "kind": "port",
           "sample": f"oracle train step (fwd+MSE+bwd+Adam) on {n} frames (1 clip) of {h}x{w}, fp32, torch {torch.__version__} CPU, "
                     f"{len(times)} steps, best of the non-first: {t:.2f} s/step; {threads} ATen threads on {info['cpu_model']} "
                     f"({info['physical_cores']} physical cores, {info['hardware_threads']} hardware threads)"}
    out.update(info)
    out["cfg1_cpu_forward"] = {"what": f"BASELINE.json config 1: forward only (no_grad, train-mode BN) on one {n}-frame clip of {h}x{w}, CPU oracle",
                               "ms": 1e3 * tf, "clips_per_s": 1.0 / tf, "threads": threads,
                               "hip_forward_ms_same_clip": 1e3 * min(hts[1:]), "hip_clips_per_s": 1.0 / min(hts[1:])}
    return out


def roofline_of(events, dtype, n, h, w, clips):
    ev = events.get("conv_fwd", [])
    if not ev:
        return None, {}
    ms = [a.elapsed_time(b) for a, b, _ in ev]
    fl = [f for _, _, f in ev]
    achieved = sum(fl) / (sum(ms) * 1e-3) / 1e12
    peak = BF16_MFMA_PEAK_TFLOPS if dtype == "bf16" else FP32_MFMA_PEAK_TFLOPS
    kname = conv_fwd_kernel(dtype, n, h, w)
    traffic, src = traffic_of(dtype, kname, clips, h)
    roof = {"bound": "mfma", "achieved": achieved, "peak": peak, "unit": "TFLOP/s", "frac": achieved / peak, "traffic": traffic,
            "traffic_source": src, "kernel": kname + " (conv2 + conv3 forward, implicit GEMM; name from the library's dispatcher)",
            "launches": len(ms), "avg_launch_ms": sum(ms) / len(ms), "algorithmic_flops_per_launch": sum(fl) / len(fl)}
    others = {}
    for k, lst in events.items():
        if k == "conv_fwd":
            continue
        t = sum(a.elapsed_time(b) for a, b, _ in lst) * 1e-3
        others[k] = {"tflops": sum(f for _, _, f in lst) / t / 1e12, "ms_per_launch": 1e3 * t / len(lst), "launches": len(lst),
                     "measured": "two instrumented steps after the timed region, without side-stream overlap"}
    return roof, others


def x6_roofline(roof, others, nseg=6.0):
    """precision="bf16x6" / "fp16x3": six / three partial products per product — the matrix cores execute 6 x / 3 x the algorithmic flops.
    The roofline counts THOSE against the 16-bit peak; `useful_tflops` is the convolution's own flop count per second (the fp32 MFMA tops
    out at 157.3)."""
    if roof is None:
        return roof, others
    roof["useful_tflops"] = roof["achieved"]
    roof["achieved"] = nseg * roof["useful_tflops"]
    roof["frac"] = roof["achieved"] / roof["peak"]
    roof["mfma_flops_per_launch"] = nseg * roof["algorithmic_flops_per_launch"]
    roof["kernel"] = roof["kernel"].replace("ConvAPadLoader256<64>", "ConvAPadLoader256<64, %d>" % nseg).replace("KCLoader256<32>", "KCLoader256<32, %d>" % nseg) \
        .replace(", 0, false>", ", 0, true>" if nseg == 3.0 else ", 0, false>") \
        + "; split operands %s, %d K-segments per launch (csrc/split3.hip)" % ("[hi | mid | lo] (bf16)" if nseg == 6.0 else "[hi | mid] (scaled fp16)", nseg)
    roof["traffic"], roof["traffic_source"] = None, "no counter pass for the split-operand launches"
    for v in others.values():
        v["useful_tflops"] = v["tflops"]
    return roof, others


def timed_steps(model, aud, vis, lab, warmup, steps, distributed, dev, instrument=True):
    """W untimed steps, then exactly K steps bracketed by barrier + synchronize on both sides; max over ranks.
    Returns (seconds, kernel events, loss, pred): loss and pred as the last timed step returned them. Without `instrument`
    no events are recorded and no extra steps run."""
    import torch.distributed as dist
    for _ in range(warmup):
        model.train_step(aud, vis, lab)
    # inside the timed steps only the forward convolutions are bracketed with events: they run alone on the stream, whereas the
    # backward overlaps weight gradients, the fused Adam and HBM-bound passes on a second stream (avm._Fork) and a bracket there
    # would time the neighbours too. The backward GEMMs are timed afterwards, in two instrumented steps without overlap.
    if instrument:
        model.kernel_events, model.time_labels = {}, {"conv_fwd"}
        if model.grad_sync is not None:
            model.grad_sync.timing = {}
    if distributed:
        dist.barrier()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(steps):
        loss, pred = model.train_step(aud, vis, lab)
    torch.cuda.synchronize()
    if distributed:
        dist.barrier()
    dt = time.perf_counter() - t0
    if distributed:
        tt = torch.tensor([dt], device=dev, dtype=torch.float64)
        dist.all_reduce(tt, op=dist.ReduceOp.MAX)
        dt = tt.item()
    loss, pred = loss.clone(), pred.clone()                          # the last timed step's results, whatever later steps reuse
    assert torch.isfinite(loss).all() and torch.isfinite(pred).all(), "non-finite loss/prediction"
    if not instrument:
        return dt, {}, loss, pred
    events = model.kernel_events
    if model.grad_sync is not None:
        model.grad_sync.timing, keep_timing = None, model.grad_sync.timing
    model.kernel_events, model.time_labels = {}, None              # instrumented, serialised steps (untimed): every labelled kernel
    for _ in range(2):
        model.train_step(aud, vis, lab)
    torch.cuda.synchronize()
    for k, v in model.kernel_events.items():
        if k != "conv_fwd":
            events[k] = v
    model.kernel_events = None
    if model.grad_sync is not None:
        model.grad_sync.timing = keep_timing
    return dt, events, loss, pred


def reduced_precision_path(dev, dtype, n, h, w, audio, seed, steps, warmup, clips, with_parity):
    """The same workload, K and W on the other engine (N = 1 only): its own ms/step, roofline and parity."""
    from cvml_goalnet_amd import AVM, synth
    torch.manual_seed(1234)
    model = AVM(audio_included=audio, device=dev, seed=seed, precision={"bf16": "bf16", "fp16": "fp16", "bf16x6": "bf16x6", "fp16x3": "fp16x3"}.get(dtype, "fp32"))
    aud, vis, lab = make_inputs(n, h, w, dev, seed)
    if not audio:
        aud = None
    parity = None
    if with_parity:
        parity = logit_parity(model, h, w, synth.BASE_SEED)
        parity.update({"weights": "random init (before the first optimizer step)", "dropout": "masks from seed formula", "bn": "train"})
        torch.cuda.empty_cache()
    dt, events, loss, _ = timed_steps(model, aud, vis, lab, warmup, steps, False, dev)
    roof, others = roofline_of(events, "bf16" if dtype in ("fp16", "bf16x6", "fp16x3") else dtype, n, h, w, clips)
    if dtype in ("bf16x6", "fp16x3"):
        roof, others = x6_roofline(roof, others, 6.0 if dtype == "bf16x6" else 3.0)
    if roof is not None and dtype == "fp16":
        roof["kernel"] = roof["kernel"].replace("gemm_bf16_256_kernel<", "gemm_bf16_256_kernel<(F16 = true) ")
        bt = _LIVE_TRAFFIC.get("bf16", (None, None))
        roof["traffic"], roof["traffic_source"] = bt[0], ("the bf16 instantiation's counters (same loads and stores; no separate pass for fp16): " + str(bt[1])
                                                          if bt[0] is not None else "no counter pass for the fp16 instantiation (same loads and stores as bf16)")
    out = {"dtype": dtype, "ms_per_step": 1e3 * dt / steps, "clips_per_s": clips * steps / dt, "steps": steps, "warmup": warmup,
           "final_loss": float(loss.item()), "roofline": roof, "other_kernels": others,
           "arithmetic": (f"{dtype} MFMA contractions (conv2/conv3 fwd+dgrad+wgrad, linear5), {dtype} storage of the activations between them; "
                          "fp32 accumulation, BatchNorm statistics, block 1, AudBl, fusion MLP, loss, gradients, master weights, Adam"
                          + ("; loss scale 2^(10 + ceil(log2 n)) on dL/dpred with an overflow guard in the fused Adam" if dtype == "fp16" else ""))
                         if dtype not in ("f32", "bf16x6", "fp16x3") else
                         ("fp32 storage and arithmetic as the fp32 path, except conv2 forward and conv3 forward / data gradient / weight gradient: their "
                          "fp32 operands are split into bf16 triples hi + mid + lo (exact) and multiplied as six partial products on the 16-bit MFMA "
                          "with fp32 accumulation (csrc/split3.hip); held to the fp32 engine's parity criteria (tests/test_gpu_bench_shapes.py)"
                          if dtype == "bf16x6" else
                          "fp32 storage and arithmetic as the fp32 path, except conv2 forward, conv3 forward / data gradient / weight gradient and linear5: "
                          "their fp32 operands are scaled by a per-tensor power of two (from a magnitude pass) and split into fp16 pairs hi + mid (22 "
                          "significand bits), multiplied as three partial products on the 16-bit MFMA with fp32 accumulation, the scales undone in the "
                          "epilogues (csrc/split3.hip); held to the fp32 engine's parity criteria (tests/test_gpu_bench_shapes.py)"
                          if dtype == "fp16x3" else "fp32 MFMA everywhere (the reference's arithmetic)")}
    if dtype == "fp16":
        out["overflow_skipped_steps"] = int(model._guard[1].item())
    if parity is not None:
        parity[f"after_{warmup + steps + 2}_adam_steps"] = logit_parity(model, h, w, synth.BASE_SEED)
        out["parity"] = parity
    return out


def native40_loop(dev, frames=300, videos=3):
    """The reference's loop at its native size: 40x40 frames, sub-batches of 10, fp32, audio on (main.py:44-46, 169-198)."""
    from cvml_goalnet_amd import AVM, synth
    from cvml_goalnet_amd.loop import VideoTrainer
    vis = torch.from_numpy(synth.make_visual(frames, 40, 40)).to(dev)
    aud = torch.from_numpy(synth.make_audio(frames)).to(dev)
    lab = torch.from_numpy(synth.make_labels(frames)).to(dev)
    model = AVM(audio_included=True, device=dev, precision="fp32")
    tr = VideoTrainer(model, subbatch_size=10)
    tr.train_video(aud, vis, lab)                       # warm-up video: first step eager, graph captured at the second
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(videos):
        losses, preds = tr.train_video(aud, vis, lab)
        batch_loss = losses.mean().item()               # the one host read-back per video (main.py:203)
    torch.cuda.synchronize()
    dt = time.perf_counter() - t0
    steps = videos * ((frames + 9) // 10)
    # the same train step by the CPU oracle on this host's cores (what the reference's own loop costs per step), and the
    # SURVEY.md §8(d) CPU points at 40x40: N = 10 (the reference's sub-batch), 64, 1024
    cpu = {}
    try:
        from oracle import avm_ref
        sd = model.state_dict()
        p = {k: v for k, v in sd.items() if v.is_floating_point() and "running" not in k}
        b = {k: v.clone() for k, v in sd.items() if k not in p}
        all_threads = torch.get_num_threads()
        for nn, reps in ((10, 5), (64, 4), (1024, 2)):
            reps_n = (nn + frames - 1) // frames
            a_c = aud.cpu().repeat(reps_n, 1, 1)[:nn]; v_c = vis.cpu().repeat(reps_n, 1, 1, 1)[:nn]; l_c = lab.cpu().repeat(reps_n)[:nn]
            masks = [torch.from_numpy(m) for m in synth.make_drop_masks(nn, step=0)]
            best = None
            for th in sorted({8, all_threads}):          # small tensors: more threads are not always faster; report the better setting
                torch.set_num_threads(th)
                state, ts = {}, []
                pp = {k: v.clone() for k, v in p.items()}
                bb = {k: v.clone() for k, v in b.items()}
                for _ in range(reps):
                    t1 = time.perf_counter()
                    avm_ref.train_step(pp, bb, state, a_c, v_c, l_c, masks, True)
                    ts.append(time.perf_counter() - t1)
                if best is None or min(ts[1:]) < best[0]:
                    best = (min(ts[1:]), th)
            torch.set_num_threads(all_threads)
            cpu[f"n{nn}"] = {"us_per_step": 1e6 * best[0], "frames_per_s": nn / best[0], "threads": best[1]}
    except Exception as e:
        log(f"cpu oracle at 40x40 failed: {e!r}")
    return {"frames_per_s": videos * frames / dt, "cpu_oracle_us_per_step": cpu.get("n10", {}).get("us_per_step"),
            "cpu_threads": cpu.get("n10", {}).get("threads"), "cpu_oracle_train_step_40x40": cpu,
            "us_per_step": 1e6 * dt / steps, "frames_per_step": 10, "h": 40, "w": 40,
            "dtype": "f32", "mode": "one HIP graph launch per sub-batch (loop.VideoTrainer)", "graph_replays": tr.replays,
            "eager_steps": tr.eager_steps, "videos": videos, "frames_per_video": frames, "last_batch_loss": batch_loss}


def dropin_path(dev, h, n, steps, warmup):
    """The path "drops into the existing scripts" means: /root/reference/main.py:187-196 verbatim — CPU tensors in, `nn.MSELoss` with
    its (n,1) x (n,) broadcast, autograd filling `.grad` of 30 strided Parameter views, stock `optim.Adam` created BEFORE the first
    forward (main.py:70), two host syncs per step (`.item()`, `.tolist()`) — with the fused device-resident step beside it."""
    import warnings
    import torch.nn as nn
    import torch.optim as optim
    from cvml_goalnet_amd import AVM, synth
    torch.manual_seed(4321)
    frame_importance_model = AVM(audio_included=True, device=dev)
    criterion = nn.MSELoss()                                                                  # main.py:68
    optimizer = optim.Adam(params=frame_importance_model.parameters(), lr=0.001)              # main.py:70
    sub_frames = torch.from_numpy(synth.make_visual(n, h, h))                                 # CPU tensors, as the dataset yields them
    sub_audios = torch.from_numpy(synth.make_audio(n))
    sub_labels = torch.from_numpy(synth.make_labels(n))
    batch_loss, batch_predictions = 0.0, []
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")                                                       # torch warns about the (n,1) x (n,) broadcast
        for i in range(warmup + steps):
            if i == warmup:
                torch.cuda.synchronize()
                t0 = time.perf_counter()
            optimizer.zero_grad()                                                             # main.py:187
            subbatch_predictions = frame_importance_model(sub_audios, sub_frames)             # main.py:188
            subbatch_loss = criterion(subbatch_predictions, sub_labels)                       # main.py:191
            subbatch_loss.backward()                                                          # main.py:192
            optimizer.step()                                                                  # main.py:193
            batch_loss += subbatch_loss.item()                                                # main.py:195
            batch_predictions.extend(subbatch_predictions.flatten().tolist())                 # main.py:196
    torch.cuda.synchronize()
    t_drop = (time.perf_counter() - t0) / steps
    del optimizer, frame_importance_model
    torch.cuda.empty_cache()
    # the same loop with ONE changed line: optimizer = model.make_optimizer(lr) (cvml_goalnet_amd.optim.Adam: one fused pass over the arena)
    torch.manual_seed(4321)
    fm = AVM(audio_included=True, device=dev)
    opt2 = fm.make_optimizer(lr=0.001)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        for i in range(warmup + steps):
            if i == warmup:
                torch.cuda.synchronize()
                t0 = time.perf_counter()
            opt2.zero_grad()
            pr = fm(sub_audios, sub_frames)
            ls = criterion(pr, sub_labels)
            ls.backward()
            opt2.step()
            batch_loss += ls.item()
            batch_predictions.extend(pr.flatten().tolist())
    torch.cuda.synchronize()
    t_drop_fused_adam = (time.perf_counter() - t0) / steps
    del opt2, fm
    torch.cuda.empty_cache()
    torch.manual_seed(4321)
    m = AVM(audio_included=True, device=dev)
    a, v, l = sub_audios.to(dev), sub_frames.to(dev), sub_labels.to(dev)
    for i in range(warmup + steps):
        if i == warmup:
            torch.cuda.synchronize()
            t0 = time.perf_counter()
        m.train_step(a, v, l)
    torch.cuda.synchronize()
    t_fused = (time.perf_counter() - t0) / steps
    del m
    torch.cuda.empty_cache()
    return {"frames_per_step": n, "h": h, "w": h, "steps": steps, "dropin_us_per_step": 1e6 * t_drop,
            "dropin_with_goalnet_adam_us_per_step": 1e6 * t_drop_fused_adam, "fused_train_step_us_per_step": 1e6 * t_fused,
            "dropin_frames_per_s": n / t_drop, "last_loss": subbatch_loss.item(),
            "what": "main.py:187-196 verbatim (CPU tensors, nn.MSELoss, autograd, stock optim.Adam over 30 strided views, .item() + .tolist()) vs "
                    "AVM.train_step on device tensors, eager launches (no graph)"}


def comm_probe(model, dev, world):
    """stand-alone all-reduce of bucket 1's size on the idle machine: what the exchange costs when nothing hides it"""
    import torch.distributed as dist
    from cvml_goalnet_amd.ddp import bucket_slices
    sl = bucket_slices(model._specs, model._arena_numel)
    t = torch.zeros(sl[1][1] - sl[1][0], dtype=torch.float32, device=dev)
    for _ in range(2):
        dist.all_reduce(t)
    torch.cuda.synchronize()
    dist.barrier()
    t0 = time.perf_counter()
    for _ in range(3):
        dist.all_reduce(t)
    torch.cuda.synchronize()
    ms = (time.perf_counter() - t0) / 3 * 1e3
    nbytes = t.numel() * 4
    return {"bytes": nbytes, "ms": ms, "algorithm_GBps": nbytes / ms / 1e6,
            "bus_GBps": nbytes / ms / 1e6 * 2 * (world - 1) / max(world, 1)}, [4 * (b - a) for a, b in sl]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--clips", type=int, default=64, help="clips of 16 frames per GPU per step")
    ap.add_argument("--hw", type=int, default=224)
    ap.add_argument("--no-cpu-baseline", action="store_true")
    ap.add_argument("--no-audio", action="store_true")
    ap.add_argument("--no-native40", action="store_true", help="skip the extra 40x40 / 10-frame loop measurement")
    ap.add_argument("--no-second-path", action="store_true", help="skip the other precision's measurement (bf16_path / fp32_path)")
    ap.add_argument("--no-live-traffic", action="store_true",
                    help="do not run the rocprofv3 --pmc passes that measure roofline.traffic at the start of the run (N = 1 only; ~1-2 minutes)")
    ap.add_argument("--global-batch", action="store_true",
                    help="N > 1: BatchNorm statistics and the broadcast MSE over all ranks' frames, gradients summed "
                         "(ddp.SyncStats: the step equals one reference process on the global batch)")
    ap.add_argument("--shard-linear5", action="store_true",
                    help="N > 1: reduce-scatter linear5.weight's gradient, Adam on the rank's 1/N slice, asynchronous all-gather of the "
                         "updated weights (ddp.GradSync(shard_linear5=True)) instead of all-reduce + replicated Adam. Off by default: it "
                         "saves ~5 ms of Adam per step at N = 8, and no RCCL run with more than one rank has exercised it yet")
    ap.add_argument("--compress-bf16", action="store_true",
                    help="N > 1, without --shard-linear5: exchange linear5.weight's gradient as bf16 (an extension; off = exact fp32 sums)")
    ap.add_argument("--dtype", choices=["f32", "bf16", "bf16x6", "fp16x3"], default=os.environ.get("GOALNET_BENCH_DTYPE", "f32"),
                    help="f32 (default) = the reference's arithmetic on the fp32 matrix cores; bf16 = bf16-MFMA contractions with "
                         "fp32 accumulation / statistics / master weights (an extension); bf16x6 = the fp32 path with the large "
                         "convolutions on split operands (fp32 values as bf16 triples, six partial products on the 16-bit MFMA: fp32-grade)")
    ap.add_argument("--full", action="store_true",
                    help="also measure everything beyond the headline: roofline / other_kernels with their counter passes, parity, "
                         "cpu_baseline, the other precisions, the 40x40 loop, the drop-in path, comm (N > 1); the --no-* options "
                         "leave parts of it out")
    ap.add_argument("--dump-outputs", metavar="DIR",
                    help="write the loss and predictions of the last timed step (rank 0) as DIR/loss.npy, DIR/pred.npy (float32)")
    args = ap.parse_args()

    # stdout carries exactly ONE line (the JSON): anything libraries print meanwhile (RCCL prints a version banner to
    # stdout at communicator creation) is diverted to stderr until the result is ready
    sys.stdout.flush()
    saved_stdout = os.dup(1)
    os.dup2(2, 1)

    world = int(os.environ.get("WORLD_SIZE", "1"))
    rank = int(os.environ.get("RANK", "0"))
    local = int(os.environ.get("LOCAL_RANK", "0"))
    if args.full and world == 1 and not args.no_live_traffic and os.environ.get("GOALNET_DDP_FORCE") != "1":
        # roofline.traffic of THIS build, from counters: child processes under rocprofv3, started before this process initialises the GPU
        for dt in (("f32", "bf16") if (args.dtype == "f32" and not args.no_second_path) else ((args.dtype,) if args.dtype not in ("bf16x6", "fp16x3") else ())):
            t0 = time.time()
            _LIVE_TRAFFIC[dt] = live_traffic(dt, args.clips, args.hw)
            log(f"live traffic {dt}: {_LIVE_TRAFFIC[dt][0]} ({time.time() - t0:.0f} s) {_LIVE_TRAFFIC[dt][1][:120]}")
    if world != args.gpus:
        log(f"note: WORLD_SIZE={world} but --gpus {args.gpus}; using WORLD_SIZE")
    import torch.distributed as dist
    distributed = world > 1 or os.environ.get("GOALNET_DDP_FORCE") == "1"
    # GOALNET_BENCH_BACKEND=gloo: REHEARSAL of the N > 1 path on a one-GPU box — every rank uses cuda:0 and gloo carries the device
    # tensors through the host (RCCL needs one GPU per rank). Exercises everything of the multi-rank bench but RCCL itself; its
    # numbers mean nothing.
    backend = os.environ.get("GOALNET_BENCH_BACKEND", "nccl")
    if distributed:
        os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
        os.environ.setdefault("MASTER_PORT", "29511")
        if backend == "gloo":
            local = 0
            torch.cuda.set_device(0)
            dist.init_process_group("gloo", rank=rank, world_size=world)
        else:
            torch.cuda.set_device(local)
            dist.init_process_group("nccl", rank=rank, world_size=world, device_id=torch.device("cuda", local))
    else:
        torch.cuda.set_device(0)
        local = 0
    dev = torch.device("cuda", local)

    from cvml_goalnet_amd import AVM, synth
    from cvml_goalnet_amd.ddp import GradSync

    n = args.clips * FRAMES_PER_CLIP
    h = w = args.hw
    seed = synth.BASE_SEED + rank
    torch.manual_seed(1234 + rank)          # ranks build DIFFERENT models on purpose: GradSync.sync_params makes them one
    model = AVM(audio_included=not args.no_audio, device=dev, seed=seed, precision={"bf16": "bf16", "bf16x6": "bf16x6", "fp16x3": "fp16x3"}.get(args.dtype, "fp32"))
    aud, vis, lab = make_inputs(n, h, w, dev, seed)
    if args.no_audio:
        aud = None
    comm = None
    if distributed:
        compress = "bf16" if args.compress_bf16 else None
        if args.global_batch:
            from cvml_goalnet_amd.ddp import enable_global_batch
            enable_global_batch(model, compress=compress, shard_linear5=args.shard_linear5)
        else:
            model.grad_sync = GradSync(compress=compress, shard_linear5=args.shard_linear5)

    single = rank == 0 and world == 1
    parity = None
    if single and args.full and not args.no_cpu_baseline:
        try:
            parity = logit_parity(model, h, w, synth.BASE_SEED)     # on the random-init weights, before any optimizer step
            parity.update({"weights": "random init (before the first optimizer step)", "dropout": "masks from seed formula", "bn": "train"})
        except Exception as e:
            log(f"parity probe failed: {e!r}")
        torch.cuda.empty_cache()            # the probe's buffers must not fragment the pool the 1024-frame steps use
    if distributed:
        # RCCL builds its communicator, channels and staging buffers lazily on the first collectives of each kind (seen with one
        # forced rank: +80 ms per step over the first steps): get that out of the way before the W warm-up steps
        with torch.no_grad():
            model.forward_device(aud[:2] if aud is not None else None, vis[:2], save=False)      # materialise + sync_params
    if distributed and args.full:
        probe, bucket_bytes = comm_probe(model, dev, world)
        sharded = model.grad_sync.sharded(model)
        comm = {"ranks": world, "backend": "nccl (RCCL over xGMI)" if backend == "nccl" else "gloo (rehearsal on one GPU: not a measurement)",
                "bucket_bytes": bucket_bytes,
                "mode": ("bucket 1 (linear5.weight): reduce-scatter -> Adam on the rank's 1/%d slice -> asynchronous all-gather of the "
                         "updated weights (waited for before the next step's linear5); buckets 0, 2: all-reduce" % world) if sharded
                        else "all-reduce of three buckets overlapped with backward, replicated fused Adam",
                "allreduce_probe_bucket1": probe, "compress": compress}
    dt, events, loss, pred = timed_steps(model, aud, vis, lab, args.warmup, args.steps, distributed, dev, instrument=args.full)
    if rank == 0 and args.dump_outputs:
        import numpy as np
        os.makedirs(args.dump_outputs, exist_ok=True)
        for name, t in (("loss", loss), ("pred", pred)):
            np.save(os.path.join(args.dump_outputs, f"{name}.npy"), t.detach().float().cpu().numpy())
    if comm is not None and model.grad_sync.timing:
        ev = model.grad_sync.timing.get("exposed_ms", [])
        ex = torch.tensor([sum(a.elapsed_time(b) for a, b in ev) / max(len(ev), 1)], device=dev, dtype=torch.float64)
        dist.all_reduce(ex, op=dist.ReduceOp.MAX)
        comm["exposed_wait_ms_per_step_max_over_ranks"] = ex.item()
        model.grad_sync.timing = None

    if rank == 0:
        clips = args.clips * world * args.steps
        res = {
            "metric": "training clips/sec at batch 64, 16-frame 224² clips; logit MAE vs CPU ref",
            "value": clips / dt, "unit": "clips/s", "n_gpus": world, "steps": args.steps, "warmup": args.warmup,
            "ms_per_step": 1e3 * dt / args.steps, "higher_is_better": True, "scaling": "weak", "vs_baseline": None,
            "dtype": args.dtype, "data": "synthetic",
            "config": {"workload": f"AVM train step (forward + broadcast-MSE + backward + fused Adam), {args.clips} clips x 16 frames = "
                                   f"{n} frames of 3x{h}x{w} + 30x30 MFCC per GPU; dropout live (device masks), BatchNorm train mode",
                       "frames_per_gpu": n, "h": h, "w": w, "global_clips_per_step": args.clips * world,
                       "parallelism": f"dp{world}", "ddp_semantics": ("BatchNorm sums + broadcast MSE over all ranks' frames, gradient sum (global batch)"
                                                                 if distributed and args.global_batch else
                                                                 "local BN + local MSE per rank, gradient mean (standard DDP)") +
                       ("; linear5.weight gradient exchanged as bf16" if args.compress_bf16 and distributed else ""),
                       "params": int(sum(s.numel for s in model._specs)), "final_loss": float(loss.item())},
        }
        if args.full:
            roof, others = roofline_of(events, "bf16" if args.dtype in ("bf16x6", "fp16x3") else args.dtype, n, h, w, args.clips)
            if args.dtype in ("bf16x6", "fp16x3"):
                roof, others = x6_roofline(roof, others, 6.0 if args.dtype == "bf16x6" else 3.0)
            if roof is not None:
                res["roofline"] = roof
                res["other_kernels"] = others
        if comm is not None:
            res["comm"] = comm
        if single and args.full and not args.no_cpu_baseline:
            try:
                if parity is not None:
                    after = logit_parity(model, h, w, synth.BASE_SEED)
                    parity[f"after_{args.warmup + args.steps + 2}_adam_steps"] = after  # same probe on the trained weights (W + K + 2 instrumented steps)
                res["parity"] = parity
                res["cpu_baseline"] = cpu_baseline(model, h, w, synth.BASE_SEED)
            except Exception as e:  # the bench line must still be printed
                log(f"cpu_baseline failed: {e!r}")
                res["cpu_baseline"] = None
        if single and args.full:
            del model, aud, vis, lab
            torch.cuda.empty_cache()
            if not args.no_second_path:
                for other in (("fp16x3", "bf16x6", "bf16", "fp16") if args.dtype == "f32" else ("f32",)):
                    key = {"bf16": "bf16_path", "fp16": "fp16_path", "f32": "fp32_path", "bf16x6": "bf16x6_path", "fp16x3": "fp16x3_path"}[other]
                    try:
                        res[key] = reduced_precision_path(dev, other, n, h, w, not args.no_audio, seed, args.steps, args.warmup, args.clips,
                                                          not args.no_cpu_baseline)
                    except Exception as e:
                        log(f"{other} path failed: {e!r}")
                        res[key] = None
                    torch.cuda.empty_cache()
            if not args.no_native40:
                try:
                    res["native_40x40_loop"] = native40_loop(dev)
                except Exception as e:
                    log(f"native 40x40 loop failed: {e!r}")
                    res["native_40x40_loop"] = None
                try:
                    res["dropin_path"] = {"n10_h40": dropin_path(dev, 40, 10, 60, 10), "n64_h224": dropin_path(dev, 224, 64, 5, 2)}
                except Exception as e:
                    log(f"drop-in path timing failed: {e!r}")
                    res["dropin_path"] = None
        cands = [k for k in ("fp16x3_path", "bf16x6_path") if single and res.get(k)]
        if cands:
            # for the reader of the line: the fastest step that meets the fp32 engine's parity criteria (NOT `value`, which is the fp32 MFMA)
            best = max(cands, key=lambda k: res[k]["clips_per_s"])
            res["fp32_grade_best"] = {"path": best, "clips_per_s": res[best]["clips_per_s"], "ms_per_step": res[best]["ms_per_step"],
                                      "vs_value": res[best]["clips_per_s"] / res["value"],
                                      "note": "fp32 operands as 16-bit parts (bf16 triples / scaled fp16 pairs), the largest partial products on the "
                                              "16-bit MFMA with fp32 accumulation (csrc/split3.hip); held to the fp32 parity criteria by "
                                              "tests/test_gpu_bench_shapes.py"}
        sys.stdout.flush()
        os.dup2(saved_stdout, 1)
        print(json.dumps(res), flush=True)
        os.dup2(2, 1)
    if distributed:
        dist.barrier()
        dist.destroy_process_group()


if __name__ == "__main__":
    main()
