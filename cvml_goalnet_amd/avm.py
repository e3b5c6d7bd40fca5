"""`AVM` — the drop-in for the reference's hot path, running on one MI355X.

Mirrors `/root/reference/utils.py:229-272` (class AVM) and its callers' contract:

    model = AVM(audio_included)                       # main.py:64, 325; baseline.py:63
    optim.Adam(model.parameters(), lr=1e-3)           # main.py:70 — BEFORE the first forward (Lazy semantics)
    out = model(audio_input, visual_input)            # audio first; (N,30,B) / list of None, (N,3,H,W) -> (N,1)
    nn.MSELoss()(out, labels).backward(); optimizer.step()      # main.py:187-193
    torch.save(model.state_dict(), f) / model.load_state_dict(torch.load(f))   # main.py:66, 263, 282

Same sub-module names (`visbl`, `audbl`, `fusion`) and therefore the same `state_dict` keys, shapes and
torch-native layouts as the reference. A fresh model is in train mode, as the reference's is (it never
calls `.eval()`): BatchNorm uses batch statistics and updates its running buffers on every forward, also
under `torch.no_grad()`; dropout is live. `model.eval()` is honoured as by `nn.BatchNorm2d` / `nn.Dropout`:
BatchNorm normalises with the running statistics and leaves the buffers (and `num_batches_tracked`) alone,
the five dropouts are the identity and the dropout counter does not advance; gradients still flow (frozen
BatchNorm statistics: dp = gamma * invstd_running * dz). `model.train()` restores the train-mode behaviour.

All arithmetic runs in libgoalnet_hip.so (hand-written gfx950 kernels) — there is no CPU or eager-PyTorch
fallback. Parameters live in ONE flat fp32 arena in device layouts (conv weights OHWI, linear5 columns in
NHWC-flatten order); each `nn.Parameter` is a strided view of it with the reference's logical shape, so
stock `torch.optim.Adam` works on them, gradients are written straight into a parallel gradient arena,
and the fused Adam / the DDP all-reduce are single passes over flat memory.

Besides the drop-in surface there is a device-resident fast path, `train_step()`, that runs forward,
the broadcast MSE, backward, (optional) gradient all-reduce and the fused Adam without leaving the GPU.
"""
from __future__ import annotations

import contextlib
import math
import os
from typing import List, Optional

import torch
import torch.nn as nn
from torch.nn.parameter import UninitializedParameter

from . import ops
from ._lib import GoalnetError
from .synth import BASE_SEED, DROP_P, TID_DROP

F32 = torch.float32
BN_EPS = 1e-5
BN_MOMENTUM = 0.1
_ALIGN = 64  # arena slots are multiples of 64 floats (256 B)


class _LazyFlags:
    """`module.requires_grad_(flag)` that also works before the first forward: torch refuses the tensor method on a Lazy
    (uninitialised) parameter, but the flag is a plain attribute and stays with the nn.Parameter when AVM._materialize fixes its shape."""

    def requires_grad_(self, requires_grad: bool = True):
        for p in self.parameters():
            p.requires_grad = requires_grad
        return self


class _Holder(_LazyFlags, nn.Module):
    """A sub-module that only owns parameters/buffers (keeps the reference's state_dict key prefixes)."""

    def forward(self, *a, **k):  # pragma: no cover
        raise GoalnetError("sub-modules of the MI355X AVM are parameter holders; call the AVM itself")


class _Layers(_LazyFlags, nn.ModuleDict):
    pass


def _mk_layer(bias=True, bn_channels=0):
    h = _Holder()
    h.weight = UninitializedParameter()
    if bias:
        h.bias = UninitializedParameter()
    if bn_channels:
        h.register_buffer("running_mean", None)
        h.register_buffer("running_var", None)
        h.register_buffer("num_batches_tracked", None)
    return h


class _Fork:
    """Fork / join onto a second HIP stream for work that is off the critical path of a SMALL step (the reference's 10-frame
    sub-batches, main.py:177-196): there a step is ~80 short kernels in one dependency chain, most of them too small to fill
    256 CUs, and the weight-gradient / bias-gradient / AudBl kernels do not feed that chain. Run on a side stream they execute
    under it; inside a captured HIP graph the fork and join become graph edges (no runtime cost). Results are unchanged (same
    kernels, same order within each dependency chain). Tensors the side stream reads are kept alive until the join, so the
    caching allocator cannot hand their memory to the main stream while the side kernels are still running."""

    def __init__(self, model, enabled):
        self.enabled = enabled
        self.keep = []
        if enabled:
            if model._side_stream is None:
                model._side_stream = torch.cuda.Stream(device=model._device)
            self.side = model._side_stream
            self.forked = False

    def run(self, fn, *tensors):
        """fn() on the side stream, after everything enqueued on the current stream so far"""
        if not self.enabled:
            return fn()
        self.keep.extend(t for t in tensors if t is not None)
        self.side.wait_stream(torch.cuda.current_stream())
        self.forked = True
        with torch.cuda.stream(self.side):
            return fn()

    def run_marked(self, fn, *tensors):
        """run(fn) and return an event recorded right behind it on the side stream (None when not forking): `wait(event)` makes
        the current stream wait for THAT piece of side work only, not for everything the side stream holds"""
        r = self.run(fn, *tensors)
        if not self.enabled:
            return r, None
        ev = torch.cuda.Event()
        ev.record(self.side)
        return r, ev

    @staticmethod
    def wait(ev):
        if ev is not None:
            torch.cuda.current_stream().wait_event(ev)

    def join(self):
        if self.enabled and self.forked:
            torch.cuda.current_stream().wait_stream(self.side)
            self.forked = False
        self.keep.clear()


class _Bwd:
    """What ONE backward_device pass shares with _block_bwd / _conv_block_bwd: the side-stream fork, the trainable set (T, any_T) with
    where each parameter gradient goes (G), and the bias-gradient partials of blocks 3 and 2 that go out together at the end of the pass."""

    def __init__(self, model, train, fork):
        self.model, self.train, self.fork = model, train, fork
        self.scratch = {}              # name -> gradient of a tensor that is not trained, where a fused kernel cannot omit it
        self.dbias = {}                # block -> (partials, channels)
        self.T = train.__contains__

    def any_T(self, *layers):
        return any(f"{layer}.{leaf}" in self.train for layer in layers for leaf in ("weight", "bias"))

    def G(self, name):
        """the gradient arena's slot for a trained tensor; per-pass scratch for the small gradients a fused kernel cannot omit (BatchNorm
        affine, the fused MLP, the heads, AudBl's Conv1d layers), never the arena. The GEMM-sized gradients have no scratch: every launch
        that writes one is issued under T(name) alone."""
        m = self.model
        if name in self.train:
            return m._gflat(name)
        s = m.spec(name)
        if s.kind in ("ohwi", "lin5") and name != "visbl.conv1.weight":      # conv1's comes from the launch that sums conv1.bias's
            raise GoalnetError(f"a backward that does not train {name} asked for its gradient")
        t = self.scratch.get(name)
        if t is None:
            t = self.scratch[name] = torch.empty(s.numel, dtype=F32, device=m._device)
        return t


class _Spec:
    __slots__ = ("name", "kind", "shape", "numel", "offset", "fan_in")

    def __init__(self, name, kind, shape, fan_in):
        self.name, self.kind, self.shape, self.fan_in = name, kind, tuple(shape), fan_in
        self.numel = int(math.prod(shape))
        self.offset = 0


def trainable_ranges(specs, frozen, skipped):
    """[(begin, count, skipped)]: the arena ranges the fused Adam updates when the tensors named in `frozen` sit the step out
    (ops.adam_step_dev_ranges). Trainable tensors in neighbouring slots merge into one range — the slot padding between them included,
    which holds zeros in all four arenas and stays zero under Adam — as long as they sat out the same number of optimizer steps
    (`skipped`: name -> count, missing = 0), because a range has one bias-correction count. Pure: the host tests call it."""
    out, slot_end = [], None
    for s in sorted(specs, key=lambda s: s.offset):
        if s.name in frozen:
            slot_end = None
            continue
        k = int(skipped.get(s.name, 0))
        if out and slot_end == s.offset and out[-1][2] == k:
            out[-1] = (out[-1][0], s.offset + s.numel - out[-1][0], k)
        else:
            out.append((s.offset, s.numel, k))
        slot_end = s.offset + (s.numel + _ALIGN - 1) // _ALIGN * _ALIGN
    return out


EPI_FUSE_MIN_ROWS = 256        # frames from which linear5's weight gradient carries Adam in its epilogue (the size of _large_overlap)
EPI_FUSE_SKINNY_ROWS = 16      # up to here linear5 runs on the weight-streaming kernels, which have no such epilogue


def epi_fuse_pieces(env):
    """GOALNET_F32_EPI_FUSE (read per call) -> the set of fused epilogue pieces that may run: unset or "1" all of them, "0" none
    (the launches as before), otherwise the pieces named by letter ("a": linear5 dW + Adam). Pure: the host tests call it."""
    if env is None or env in ("", "1"):
        return frozenset("a")
    if env == "0":
        return frozenset()
    return frozenset(ch for ch in env.lower() if ch in "a")


def epi_fuse_dw_adam(n, *, plain, synced, precision, train_w5, shadowed, inspected, forced, pieces):
    """linear5's weight gradient with the Adam update of linear5.weight in its epilogue (ops.linear_bwd_dw_adam) for this
    train_step? Only where the early Adam would be legal — every tensor trains under the global step count (`plain`), no gradient
    exchange, the fp32 engine (no overflow guard, no 16-bit copy of the weight to refresh: `shadowed`) — linear5.weight trains, and
    the step is large: `forced` (model.epi_fuse) True drops the size rule down to the 128 x 128 tile's smallest step, False and a
    GOALNET_F32_EPI_FUSE without "a" switch the piece off. A step that is kept for inspection (`inspected`: model.keep_ctx) writes
    every gradient unless the piece is forced: the fused launch leaves linear5.weight's gradient slot alone. Pure: the host tests
    call it."""
    if forced is False or "a" not in pieces:
        return False
    if inspected and forced is not True:
        return False
    if not (plain and not synced and precision == "fp32" and train_w5 and not shadowed):
        return False
    if n <= EPI_FUSE_SKINNY_ROWS:
        return False
    return forced is True or n >= EPI_FUSE_MIN_ROWS


def optim_step_path(optim, *, sharded):
    """Does this optimizer step run under options (optim.OptimOptions)? None or trivial options: False — today's plan,
    launch for launch (early Adam, epilogue-fused linear5 update, the arena passes). Otherwise True: no early Adam and no fused
    epilogue — clipping needs the whole norm before any update and both shortcuts hard-code plain Adam — but, after backward, the
    gradient exchange and the fp16 finite check, ops.grad_sumsq (clipping only) and ONE ops.optim_step_dev_ranges over optim_ranges().
    `sharded` (ddp.GradSync(shard_linear5=True)) refuses: a rank holds only its slice of that gradient. Pure: the host tests call it."""
    if optim is None or optim.trivial:
        return False
    if sharded:
        raise GoalnetError("optimizer options (weight decay, clipping, schedules, parameter groups, AMSGrad) are not built for ddp.GradSync(shard_linear5=True): "
                           "a rank holds only its slice of linear5.weight's gradient; use a plain GradSync")
    return True


def ema_step_path(ema, *, sharded):
    """Does this optimizer step move a weight average (optim.EmaOptions)? None: False — no arena, no launch. Otherwise
    True: ONE ops.ema_update_dev_ranges over trainable_ranges() behind every update of the step, in front of the launch that advances
    the counters. The average observes: it switches off neither the early Adam nor the epilogue-fused update. `sharded`
    (ddp.GradSync(shard_linear5=True)) refuses: a rank's fp32 master of the foreign slices of linear5.weight is stale between steps.
    Pure: the host tests call it."""
    if ema is None:
        return False
    if not (hasattr(ema, "weight_at") and hasattr(ema, "signature")):
        raise ValueError("ema must be an optim.EmaOptions")
    if sharded:
        raise GoalnetError("a weight average (ema=) is not built for ddp.GradSync(shard_linear5=True): a rank holds only its slice of "
                           "linear5.weight's up-to-date master; use a plain GradSync")
    return True


def accum_count(k):
    """train_step's / VideoTrainer's `accumulate` -> the window length as an int >= 1; anything else — a bool, a
    float, 0 — is a ValueError. Pure: the host tests call it."""
    if isinstance(k, bool) or not isinstance(k, int) or k < 1:
        raise ValueError(f"accumulate must be an integer >= 1, got {k!r}")
    return k


def accum_windows(n_frames, subbatch_size, k):
    """[(rows, position, length)] per sub-batch of a video of n_frames: how loop.VideoTrainer(accumulate=k) cuts the video's sub-batches
    (main.py:177-184: subbatch_size frames each, a shorter last one) into windows of k micro-steps. Windows never span videos: the last
    window may be shorter, length j < k, and runs as a window of j (c = 1 / j), applied at the end of the video. Pure: the host tests
    call it."""
    k = accum_count(k)
    if n_frames < 1 or subbatch_size < 1:
        raise ValueError("n_frames and subbatch_size must be >= 1")
    rows = [min(subbatch_size, n_frames - off) for off in range(0, n_frames, subbatch_size)]
    out = []
    for s, r in enumerate(rows):
        start = s - s % k
        out.append((r, s - start, min(k, len(rows) - start)))
    return out


STATE_FORMAT = 1               # AVM.training_state()["format"]


def optim_ranges(specs, frozen, skipped, optim):
    """[(begin, count, skipped, decay)]: trainable_ranges() split further wherever the decay flag changes (optim.decays(name): weight
    decay is on and no `no_decay` substring matches). Neighbours merge, slot padding included (zero in all four arenas, and zero under
    decay), while they share the count of sat-out steps AND the flag. Pure: the host tests call it."""
    out, slot_end = [], None
    for s in sorted(specs, key=lambda s: s.offset):
        if s.name in frozen:
            slot_end = None
            continue
        k, d = int(skipped.get(s.name, 0)), bool(optim.decays(s.name))
        if out and slot_end == s.offset and out[-1][2] == k and out[-1][3] == d:
            out[-1] = (out[-1][0], s.offset + s.numel - out[-1][0], k, d)
        else:
            out.append((s.offset, s.numel, k, d))
        slot_end = s.offset + (s.numel + _ALIGN - 1) // _ALIGN * _ALIGN
    return out


def group_ranges(specs, frozen, skipped, optim, lr, betas, eps):
    """([(begin, count, skipped, decay, group)], hyper_table): optim_ranges() split further wherever the group index changes
    (optim.group_of(name): the first optim.ParamGroup whose `match` hits the name, else 0, the default group). The decay
    flag is optim.group_decays(name): an explicit group weight_decay reaches every tensor of the group. Neighbours merge, slot padding
    included, while they share the count of sat-out steps, the flag AND the group. hyper_table is optim.hyper_table(lr, betas, eps):
    one (lr, beta1, beta2, eps, weight_decay, amsgrad) per group, the call's own values in row 0. Pure: the host tests call it."""
    out, slot_end = [], None
    for s in sorted(specs, key=lambda s: s.offset):
        if s.name in frozen:
            slot_end = None
            continue
        k, d, q = int(skipped.get(s.name, 0)), bool(optim.group_decays(s.name)), int(optim.group_of(s.name))
        if out and slot_end == s.offset and out[-1][2:] == (k, d, q):
            out[-1] = (out[-1][0], s.offset + s.numel - out[-1][0], k, d, q)
        else:
            out.append((s.offset, s.numel, k, d, q))
        slot_end = s.offset + (s.numel + _ALIGN - 1) // _ALIGN * _ALIGN
    if len(out) > ops.ADAM_RANGES_MAX:
        raise GoalnetError(f"{len(out)} trainable ranges (split by weight decay and parameter group): the fused step takes {ops.ADAM_RANGES_MAX}")
    return out, optim.hyper_table(lr, betas, eps)


class AVM(_LazyFlags, nn.Module):
    def __init__(self, audio_included, device=None, seed: Optional[int] = None, precision: str = "fp32", head: str = "regression",
                 num_classes: int = 5):
        """`seed`: seed of the counter-based dropout stream. None (default) draws it from the torch RNG at construction, so
        dropout follows `torch.manual_seed` as the reference's does (utils.py:170, 245-254 use the global torch RNG) and two
        model instances / two runs do not replay the same masks; parity tests pass synth.BASE_SEED to regenerate the masks
        from the seed formula on the CPU side."""
        super().__init__()
        self.audio_included = audio_included                      # utils.py:235
        # head="classifier" (EXTENSION): the reference's commented-out variant — Linear(128 -> C), Softmax(dim=1) in place of
        # the Sigmoid (utils.py:257), then 4y+1 (utils.py:270); trained with CrossEntropyLoss on labels-1 (main.py:69, 189),
        # predictions = argmax + 1 (main.py:190). forward returns the (N, C) class scores.
        if head not in ("regression", "classifier"):
            raise ValueError("head must be 'regression' (the reference's live code) or 'classifier' (its commented-out variant)")
        if not 2 <= num_classes <= 8:
            raise ValueError("num_classes must be in 2..8")
        self.head = head
        self.num_classes = num_classes if head == "classifier" else 1
        if precision not in ("fp32", "bf16", "fp16", "bf16x6", "fp16x3"):
            raise ValueError("precision must be 'fp32' (the reference's arithmetic), 'bf16x6' / 'fp16x3' (fp32 operands as bf16 triples / scaled "
                             "fp16 pairs on the 16-bit MFMA: fp32-grade), 'bf16' or 'fp16' (16-bit MFMA contractions)")
        # "bf16x6": everything is stored and computed as under "fp32" except the large 3 x 3 convolutions (conv2 forward; conv3 forward,
        # data gradient and weight gradient at >= 65 536 output pixels), whose fp32 operands are split into bf16 triples hi + mid + lo
        # (exact) and multiplied as six partial products on the 16-bit MFMA with fp32 accumulation (csrc/split3.hip): fp32-grade
        # results (3-4 x the rounding error of the fp32 MFMA's own accumulation) at 1.4-1.65 x its speed.
        # "fp16x3": the same GEMMs on fp16 PAIRS hi + mid of each value scaled by a per-tensor power of two (22 significand bits; the scale
        # comes from a magnitude pass over the tensor, so no loss scale is involved) and three partial products: half the MFMA work.
        # "bf16" / "fp16": the dense contractions (conv2/conv3 forward + data / weight gradient, linear5) run on the 16-bit matrix
        # cores with fp32 accumulation; statistics, master weights, parameter gradients and Adam stay fp32.
        # fp16 keeps 11 significand bits against bf16's 8 (~8 x less rounding noise in the logits) but has 5 exponent bits:
        # the activation gradients it stores need a loss scale (loss_scale, below) and an overflow guard.
        # dL/dpred is multiplied by the loss scale before backward, the fused Adam divides it out again (a power of two: exact).
        # None (fp16 default) = 2^(10 + ceil(log2 n) - backoff) for a step of n frames: dL/dpred is O(1/n) and the 16-bit activation
        # gradients measured with scripts/grad_ranges.py (medians 6e-10 .. 1e-8, maxima 2e-7 .. 8e-6 at n = 1 024; ~1000 x that at
        # n = 10) then sit at 6e-4 .. 8 — inside binary16's normal range [6.1e-5, 65504] with four orders of magnitude of headroom.
        # The precision setter picks the default (None for fp16, 1.0 otherwise) unless the user assigned `loss_scale` explicitly.
        self._loss_scale, self._loss_scale_user = 1.0, False
        self._loss_scale_backoff = 0   # halvings of the automatic scale (update_loss_scale: one per check that found skipped steps)
        self._skipped_seen = 0
        self.precision = precision     # property: also sets _half / _h16 and the default loss scale
        self._guard = None             # fp16: int64[2] device counters — step stamped as overflowed, number of skipped updates
        if device is None:
            device = torch.device("cuda", torch.cuda.current_device()) if torch.cuda.is_available() else None
        self._device = torch.device(device) if device is not None else None

        self.visbl = _Holder()                                     # utils.py:237
        self.visbl.conv1 = _mk_layer()
        self.visbl.bnorm1 = _mk_layer(bn_channels=64)
        self.visbl.conv2 = _mk_layer()
        self.visbl.bnorm2 = _mk_layer(bn_channels=256)
        self.visbl.conv3 = _mk_layer()
        self.visbl.bnorm3 = _mk_layer(bn_channels=512)
        self.visbl.linear5 = _mk_layer()
        if audio_included:                                         # utils.py:239-240
            self.audbl = _Holder()
            self.audbl.conv1 = _mk_layer()
            self.audbl.conv2 = _mk_layer()
            self.audbl.linear3 = _mk_layer()
        self.fusion = _Layers({k: _mk_layer() for k in ("0", "3", "6", "9", "12")})   # utils.py:242-256

        # dropout (utils.py:170, 245-254): "device" = counter-based masks (synth.make_drop_masks formula),
        # "off" = p := 0, "given" = masks supplied through set_dropout_masks() (parity tests)
        self.dropout_mode = "device"
        self.dropout_seed = int(torch.randint(0, 2 ** 31 - 1, (1,)).item()) if seed is None else int(seed)
        self.dropout_row_offset = 0    # rows in front of this rank's rows in the global batch (ddp.enable_global_batch)
        self._drop_step = 0
        self._given_masks: Optional[List[torch.Tensor]] = None

        self._specs: List[_Spec] = []
        self._arena = self._garena = self._adam_m = self._adam_v = None
        self._adam_vmax = None             # AMSGrad's running maximum of v: laid out like _adam_v, allocated by the first AMSGrad step
        self._hw3 = self._l2 = None
        self._adam_t = 0
        self._adam_segs = None
        # fine-tuning: a tensor whose nn.Parameter has requires_grad=False is FROZEN — no gradient, no update, and
        # the optimizer steps it sits out are counted per tensor (torch.optim.Adam keeps a step count per parameter)
        self._sat_out = {}                 # name -> optimizer steps the tensor sat out so far (missing = 0)
        self._bwd_frozen = frozenset()     # the frozen set the last parameter backward ran under: what the next optimizer step skips
        self._fp16_frozen = None           # precision="fp16": the frozen set of the first optimizer step (it may not change afterwards)
        self._arena_grad_scale = 1.0       # the gradient arena currently holds this factor x gradient (fp16 train_step)
        self._w5b, self._w5b_version = None, None      # bf16 shadow of visbl.linear5.weight and the version stamps it matches
        self._load_count = 0                           # bumped by load_state_dict (its layout kernels write the arena directly)
        # the weight average: a third flat fp32 arena in the parameter arena's layout, allocated by the first step
        # that is given ema=; _averaged: inside `with model.averaged()` the two arenas are exchanged
        self._ema = None
        self._averaged = False
        # gradient accumulation: a second gradient arena, allocated by the first train_step(accumulate=k > 1); the
        # position in the window is HOST state — (micro-steps done, k) and the frozen set the window started under
        self._gacc = None
        self._accum_done, self._accum_k, self._accum_frozen = 0, 1, None
        self._norm_of_acc = False      # grad_norm() reads the accumulated gradient: the last backward was an accumulating train_step's
        self._state = None             # int64[4] device counters: adam step, dropout draw, frame cursor, sub-batch index
        self._materialized = False
        self.grad_sync = None          # optional ddp.GradSync: gradient exchange between backward and Adam
        self.stat_sync = None          # optional ddp.SyncStats: BatchNorm sums and the loss over all ranks' frames
        self.grad_bf16 = os.environ.get("GOALNET_DZ16", "1") != "0"   # precision="bf16": bf16 BatchNorm-output gradients (backward_device)
        self.act_bf16 = os.environ.get("GOALNET_P16", "1") != "0"     # precision="bf16": pooled activations of blocks 2, 3 stored as bf16
        # the A/B switches of DESIGN.md's table, read HERE and never again: a graph captured from a step bakes the routing in, so a
        # value that could change between two steps of one model would apply to eager steps and not to replays
        env = os.environ.get
        self.x6_off = env("GOALNET_X6_OFF") == "1"                    # _x6_conv / _x6_linear5
        self.x6_linear5 = env("GOALNET_X6_LINEAR5", "1") != "0"       # _x6_linear5
        self.x3_wgrad2 = env("GOALNET_X3_WGRAD2", "1") != "0"         # fp16x3: conv2's weight gradient on split operands (forward_device)
        self.x3_dgrad2 = env("GOALNET_X3_DGRAD2", "1") != "0"         # split precisions: conv2's data gradient on split operands (backward_device)
        self.mlp_fused = env("GOALNET_MLP_FUSED", "1") != "0"         # _mlp_fused
        self.small_bn = env("GOALNET_SMALL_BN", "1") != "0"           # _small_bn
        self.force_bf5 = env("GOALNET_FORCE_BF5") == "1"              # _bf5
        self.overlap_pair = env("GOALNET_OVERLAP_PAIR", "1") != "0"   # _pair
        # fp32 GEMM epilogue fusion (epi_fuse_dw_adam above): None = the size rule, True = also below it (tests), False = never
        self.epi_fuse = None
        self.epi_fused_dw = 0          # train_steps so far whose linear5 weight gradient ran with Adam in its epilogue
        self.keep_ctx = False          # tests: keep the last train_step's / input_gradients' saved tensors in last_ctx
        self.last_ctx = None
        self.last_used_w5b = False
        self._side_stream = None
        self.overlap_rows = int(os.environ.get("GOALNET_OVERLAP_ROWS", "64"))   # steps of <= this many frames fork their off-path work
        # Forking at LARGE sizes: off-path work (weight gradients, bias sums, AudBl) on the side stream AND the fused Adam over linear5.weight
        # there as soon as its gradient exists (train_step's "early Adam") — HBM-bound passes under MFMA-bound GEMMs and the other way
        # round. Bit-identical. Measured at 1 024 frames @224 (round 3, alternating runs on one box): bf16 73.7 -> 72.2 ms, fp16x3 182.7 ->
        # 178.6 ms, bf16x6 297.2 -> 295.6 ms, fp32 417.6 -> 428.7 ms (its GEMMs are 90 % of the step and gain nothing from company); at
        # 10 frames @40 845 -> 974 us (the 0.66 GB Adam stream slows every small kernel it runs beside). Hence the automatic rule: on for
        # the 16-bit and split-operand precisions at >= 256 frames, off otherwise. GOALNET_OVERLAP_LARGE=1 forces it at every size and
        # precision, =0 switches it off.
        _ol = os.environ.get("GOALNET_OVERLAP_LARGE")
        self.overlap_large = _ol == "1"
        self.overlap_auto = _ol is None
        self.time_labels = None        # bench: with kernel_events set, time only these labels (None = all, and no forking)
        self.kernel_events = None      # bench: {label: [(start_event, end_event, flops), ...]} when not None

    @property
    def precision(self) -> str:
        return self._precision

    @precision.setter
    def precision(self, value: str):
        if value not in ("fp32", "bf16", "fp16", "bf16x6", "fp16x3"):
            raise ValueError("precision must be 'fp32', 'bf16x6', 'fp16x3', 'bf16' or 'fp16'")
        self._precision = value
        self._half = value in ("bf16", "fp16")
        self._parts = {"bf16x6": 3, "fp16x3": 2}.get(value, 0)                # split-operand GEMMs (csrc/split3.hip); fp32 storage
        self._x6 = self._parts > 0
        self._h16 = torch.float16 if value in ("fp16", "fp16x3") else torch.bfloat16     # the 16-bit storage format of the GEMM operands
        self._w5b, self._w5b_version = None, None                              # a copy in the other format is not reusable
        self._padbufs, self._padgen = {}, {}                                   # nor are the cached padded 16-bit operand buffers
        if not self._loss_scale_user:
            # binary16's 5 exponent bits need the scale (its activation gradients would flush to zero without it, and the overflow
            # guard cannot see an underflow); bf16 / fp32 do not
            self._loss_scale = None if value == "fp16" else 1.0
            self._loss_scale_backoff = 0

    @property
    def loss_scale(self):
        return self._loss_scale

    @loss_scale.setter
    def loss_scale(self, value):
        """an explicit scale (a power of two keeps the unscale exact), or None = the automatic per-size scale of precision="fp16"; an
        explicit value survives later changes of `precision`"""
        self._loss_scale = None if value is None else float(value)
        self._loss_scale_user = value is not None
        self._loss_scale_backoff = 0

    # ------------------------------------------------------------------------------------------
    # parameter arena
    # ------------------------------------------------------------------------------------------
    def _param_specs(self, hw3: int, l2: int) -> List[_Spec]:
        """Arena order = gradient-readiness order in backward: [fusion, audbl, linear5.bias | linear5.weight |
        rest of visbl], so each DDP bucket is one contiguous slice (ddp.py)."""
        f0_in = 640 if self.audio_included else 512
        S = []

        def lin(name, out, inn, kind="plain"):
            S.append(_Spec(name + ".weight", kind, (out, inn), inn))
            S.append(_Spec(name + ".bias", "plain", (out,), inn))

        lin("fusion.12", self.num_classes, 128); lin("fusion.9", 128, 256); lin("fusion.6", 256, 512)
        lin("fusion.3", 512, 512); lin("fusion.0", 512, f0_in)
        if self.audio_included:
            lin("audbl.linear3", 128, 128 * l2)
            S.append(_Spec("audbl.conv2.weight", "plain", (128, 64, 3), 192)); S.append(_Spec("audbl.conv2.bias", "plain", (128,), 192))
            S.append(_Spec("audbl.conv1.weight", "plain", (64, 30, 3), 90)); S.append(_Spec("audbl.conv1.bias", "plain", (64,), 90))
        S.append(_Spec("visbl.linear5.bias", "plain", (512,), 512 * hw3))
        S.append(_Spec("visbl.linear5.weight", "lin5", (512, 512, hw3), 512 * hw3))      # logical (512, C, HW)
        for i, (co, ci) in ((3, (512, 256)), (2, (256, 64)), (1, (64, 3))):
            S.append(_Spec(f"visbl.bnorm{i}.weight", "bn_w", (co,), 0)); S.append(_Spec(f"visbl.bnorm{i}.bias", "bn_b", (co,), 0))
            S.append(_Spec(f"visbl.conv{i}.weight", "ohwi", (co, ci, 3, 3), ci * 9)); S.append(_Spec(f"visbl.conv{i}.bias", "plain", (co,), ci * 9))
        off = 0
        for s in S:
            s.offset = off
            off += (s.numel + _ALIGN - 1) // _ALIGN * _ALIGN
        self._arena_numel = off
        return S

    def _view(self, arena, s: _Spec):
        flat = arena[s.offset:s.offset + s.numel]
        if s.kind == "ohwi":
            o, i = s.shape[0], s.shape[1]
            return flat.view(o, 3, 3, i).permute(0, 3, 1, 2)          # logical OIHW over physical OHWI
        if s.kind == "lin5":
            o, c, hw = s.shape
            return flat.view(o, hw, c).permute(0, 2, 1)               # logical (512, C, HW) over physical (512, HW, C)
        return flat.view(s.shape)

    def _module_of(self, name):
        mod = self
        parts = name.split(".")
        for p in parts[:-1]:
            mod = mod[p] if isinstance(mod, nn.ModuleDict) else getattr(mod, p)
        return mod, parts[-1]

    def _require_device(self):
        if self._device is None or self._device.type != "cuda":
            raise GoalnetError("the MI355X AVM needs a GPU (torch.cuda.is_available() is False); there is no CPU fallback")
        ops.lib()

    def _make_state(self):
        """Device counters read by the graph-capturable kernels (csrc/stepstate.hip); host mirrors: _adam_t, _drop_step."""
        self._require_device()
        self._state = torch.tensor([self._adam_t, self._drop_step, 0, 0], dtype=torch.int64, device=self._device)
        self._guard = torch.zeros(2, dtype=torch.int64, device=self._device)

    def _materialize(self, hw3: int, l2: int, init: bool = True):
        """Fix the Lazy shapes (first forward or load_state_dict) and build the arena. Parameters are
        materialised IN PLACE so an optimizer created earlier keeps valid references (main.py:70)."""
        if self._materialized:
            if hw3 != self._hw3 or (self.audio_included and l2 != self._l2):
                raise RuntimeError(f"input size changed after materialisation: linear5 expects {512 * self._hw3} features "
                                   f"(got {512 * hw3}), audbl.linear3 {128 * (self._l2 or 0)} (got {128 * l2})")
            return
        self._require_device()
        if self._state is None:
            self._make_state()
        self._hw3, self._l2 = hw3, l2
        self._specs = self._param_specs(hw3, l2)
        dev = self._device
        self._arena = torch.zeros(self._arena_numel, dtype=F32, device=dev)
        seed = int(torch.randint(0, 2 ** 31 - 1, (1,)).item()) if init else 0
        for k, s in enumerate(self._specs):
            mod, leaf = self._module_of(s.name)
            prm = getattr(mod, leaf)
            view = self._view(self._arena, s)
            if init:
                flat = self._arena[s.offset:s.offset + s.numel]
                if s.kind == "bn_w":
                    flat.fill_(1.0)
                elif s.kind != "bn_b":
                    bound = 1.0 / math.sqrt(s.fan_in)                 # torch default init, SURVEY.md §8(a) row 1
                    ops.fill_uniform(flat, seed, k, -bound, bound)
            prm.data = view
            if isinstance(prm, UninitializedParameter):
                prm.__class__ = prm.cls_to_become                     # what UninitializedParameter.materialize does
        for i, c in ((1, 64), (2, 256), (3, 512)):
            bn = getattr(self.visbl, f"bnorm{i}")
            bn.running_mean = torch.zeros(c, dtype=F32, device=dev)
            bn.running_var = torch.ones(c, dtype=F32, device=dev)
            bn.num_batches_tracked = torch.zeros((), dtype=torch.int64)   # host counter (no launch per forward)
        self._materialized = True

    def spec(self, name) -> _Spec:
        for s in self._specs:
            if s.name == name:
                return s
        raise KeyError(name)

    def _pflat(self, name):
        s = self.spec(name)
        return self._arena[s.offset:s.offset + s.numel]

    def _gflat(self, name):
        s = self.spec(name)
        return self._garena[s.offset:s.offset + s.numel]

    def _ensure_garena(self):
        if self._garena is None:
            self._garena = torch.zeros(self._arena_numel, dtype=F32, device=self._device)

    def _frozen_names(self):
        """names of the parameter tensors with requires_grad=False (the flags live on the nn.Parameters, also while they are Lazy)"""
        return frozenset(k for k, p in self.named_parameters() if not p.requires_grad)

    def _check_freeze(self, frozen):
        if frozen and (self.grad_sync is not None or self.stat_sync is not None):
            raise GoalnetError("freezing under DDP is not built: every parameter must have requires_grad=True while a grad_sync / "
                               "stat_sync is attached (bucket layouts and sharding are laid out for the whole arena)")

    def _plain_step(self, frozen):
        """every tensor trains under the global step count: today's single pass over the arena"""
        return not frozen and not any(self._sat_out.values())

    def trainable_signature(self):
        """what a captured step bakes in about the trainable set: () while every tensor trains under the global step count, else the
        (begin, count, skipped) of every range of the fused Adam (before the Lazy shapes are fixed: the frozen names)"""
        frozen = self._frozen_names()
        if self._plain_step(frozen):
            return ()
        if not self._materialized:
            return tuple(sorted(frozen))
        return tuple(trainable_ranges(self._specs, frozen, self._sat_out))

    def _count_sat_out(self, frozen):
        for k in frozen:
            self._sat_out[k] = self._sat_out.get(k, 0) + 1

    def _exact_runs(self, names):
        """[(lo, hi)] of the named tensors, neighbours merged only where no slot padding lies between them"""
        runs = []
        for s in sorted((self.spec(k) for k in names), key=lambda s: s.offset):
            if runs and runs[-1][1] == s.offset:
                runs[-1] = (runs[-1][0], s.offset + s.numel)
            else:
                runs.append((s.offset, s.offset + s.numel))
        return runs

    # ------------------------------------------------------------------------------------------
    # state_dict interchange in the reference's torch-native layouts (main.py:66, 263, 282, 326)
    # ------------------------------------------------------------------------------------------
    def state_dict(self, *args, destination=None, prefix="", keep_vars=False):
        if not self._materialized:
            raise RuntimeError("state_dict() before the first forward / load_state_dict(): parameters are uninitialised")
        if self.grad_sync is not None:
            # ddp.GradSync(shard_linear5=True) in a 16-bit mode leaves the fp32 master of the other ranks' slices of linear5.weight
            # stale between steps. Bringing it up to date is a COLLECTIVE: state_dict() does not issue it behind the caller's back
            # (`if rank == 0: torch.save(model.state_dict())` would hang) — every rank calls grad_sync.consolidate(model) first.
            if self.grad_sync.master_stale:
                raise GoalnetError("state_dict(): foreign slices of visbl.linear5.weight's fp32 master are stale (GradSync(shard_linear5=True) "
                                   "in a 16-bit mode); call model.grad_sync.consolidate(model) on EVERY rank first (a collective)")
            self.grad_sync.wait_weights()                # fp32 + sharded: the in-flight all-gather of the updated weights (local wait)
        out = {} if destination is None else destination
        order = self._reference_key_order()
        for name in order:
            if name.endswith(("running_mean", "running_var", "num_batches_tracked")):
                mod, leaf = self._module_of(name)
                out[prefix + name] = getattr(mod, leaf).detach().cpu().clone()
                continue
            s = self.spec(name)
            flat = self._arena[s.offset:s.offset + s.numel]
            if s.kind == "ohwi":
                o, i = s.shape[0], s.shape[1]
                t = torch.empty(s.numel, dtype=F32, device=self._device)
                ops.transpose_inner(flat, t, o, 9, i)                  # [O][9][I] -> [O][I][9]
                t = t.view(o, i, 3, 3)
            elif s.kind == "lin5":
                o, c, hw = s.shape
                t = torch.empty(s.numel, dtype=F32, device=self._device)
                ops.transpose_inner(flat, t, o, hw, c)                 # [512][HW][C] -> [512][C][HW]
                t = t.view(o, c * hw)
            else:
                t = flat.view(s.shape).clone()
            out[prefix + name] = t.cpu()
        return out

    def _reference_key_order(self):
        from .synth import PARAM_ORDER
        keys = []
        for name in PARAM_ORDER:
            if name.startswith("audbl.") and not self.audio_included:
                continue
            keys.append(name)
            if ".bnorm" in name and name.endswith(".bias"):
                base = name.rsplit(".", 1)[0]
                keys += [base + ".running_mean", base + ".running_var", base + ".num_batches_tracked"]
        return keys

    def load_state_dict(self, state_dict, strict: bool = True, assign: bool = False):
        w5 = state_dict["visbl.linear5.weight"]
        if w5.dim() != 2 or w5.shape[0] != 512 or w5.shape[1] % 512:
            raise RuntimeError(f"visbl.linear5.weight has shape {tuple(w5.shape)}, expected (512, 512*H3*W3)")
        hw3 = w5.shape[1] // 512
        l2 = state_dict["audbl.linear3.weight"].shape[1] // 128 if self.audio_included else 0
        if self._averaged:
            raise GoalnetError("load_state_dict() inside `with model.averaged()`: the arena holds the averaged weights there")
        self._load_count += 1
        self._materialize(hw3, l2, init=False)
        if self.grad_sync is not None:
            # every slice of the master is about to be overwritten from the file (load_state_dict runs on all ranks, as in the
            # reference's single process): an in-flight gather must land first, and nothing is stale afterwards
            self.grad_sync.wait_weights()
            self.grad_sync.master_stale = False
        expected = set(self._reference_key_order())
        missing = sorted(expected - set(state_dict.keys()))
        unexpected = sorted(set(state_dict.keys()) - expected)
        if strict and (missing or unexpected):
            raise RuntimeError(f"load_state_dict: missing keys {missing}, unexpected keys {unexpected}")
        with torch.no_grad():
            for name in expected & set(state_dict.keys()):
                src = state_dict[name]
                if name.endswith(("running_mean", "running_var", "num_batches_tracked")):
                    mod, leaf = self._module_of(name)
                    getattr(mod, leaf).copy_(src)
                    continue
                s = self.spec(name)
                logical = (s.shape[0], s.shape[1] * s.shape[2]) if s.kind == "lin5" else s.shape
                if tuple(src.shape) != tuple(logical):
                    raise RuntimeError(f"size mismatch for {name}: {tuple(src.shape)} vs {tuple(logical)}")
                flat = self._arena[s.offset:s.offset + s.numel]
                t = src.detach().to(device=self._device, dtype=F32).contiguous().view(-1)
                if s.kind == "ohwi":
                    ops.transpose_inner(t, flat, s.shape[0], s.shape[1], 9)      # [O][I][9] -> [O][9][I]
                elif s.kind == "lin5":
                    ops.transpose_inner(t, flat, s.shape[0], s.shape[1], s.shape[2])  # [512][C][HW] -> [512][HW][C]
                else:
                    flat.copy_(t)
        if self._ema is not None:
            # weights from a file: the average restarts from them — in place, captured graphs hold the arena's address
            # (load_training_state puts the saved average back afterwards)
            self._ema.copy_(self._arena)
        return torch.nn.modules.module._IncompatibleKeys(missing, unexpected)

    # ------------------------------------------------------------------------------------------
    # dropout masks
    # ------------------------------------------------------------------------------------------
    def set_dropout_masks(self, masks: Optional[List[torch.Tensor]]):
        """Parity mode: five (N,width) multiplier tensors [visbl.drop5, fusion.2, .5, .8, .11] used by the next forward."""
        self.dropout_mode = "given" if masks is not None else "off"
        self._given_masks = None if masks is None else [m.to(self._device, F32).contiguous() for m in masks]

    def _masks(self, n: int, caller_ticks: bool = False):
        """(the five masks, draws the CALLER still has to add to the device counter state[1]): with caller_ticks the draw is left for
        the launch that advances all of train_step's counters at its end"""
        if not self.training or self.dropout_mode == "off":
            return [None] * 5, 0                 # eval(): the five dropouts are the identity and the draw counter stays put
        if self.dropout_mode == "given":
            for m, wdt in zip(self._given_masks, (512, 512, 512, 256, 128)):
                if tuple(m.shape) != (n, wdt):
                    raise RuntimeError(f"dropout mask shape {tuple(m.shape)} != {(n, wdt)}")
            return list(self._given_masks), 0
        # one launch for the five masks; the draw index is the device counter state[1] (graph-capturable)
        widths = (512, 512, 512, 256, 128)
        buf = torch.empty(n * sum(widths), dtype=F32, device=self._device)
        # global-batch mode: this rank draws rows [rank * n, (rank + 1) * n) of the masks one process would draw for the
        # concatenated batch; standard DDP: an independent stream per rank (ddp.GradSync.sync_params re-seeds)
        row0 = self.stat_sync.rank * n if self.stat_sync is not None else self.dropout_row_offset
        out = ops.dropout_masks_dev(buf, n, widths, self.dropout_seed, TID_DROP, 8, self._state[1], DROP_P, row_offset=row0)
        if not caller_ticks:
            ops.counter_add(self._state[1], 1)
        self._drop_step += 1
        return out, int(caller_ticks)

    # ------------------------------------------------------------------------------------------
    # forward / backward on device tensors
    # ------------------------------------------------------------------------------------------
    def _w5_bf16(self, k5):
        """bf16 copy of visbl.linear5.weight. The fused Adam of train_step refreshes it while it updates the fp32 master
        (ops.adam_step_dev_shadow), so the next forward needs no 7.7 GB cast pass; any other writer (a stock torch optimizer,
        load_state_dict, in-place edits of the Parameter or of the arena) changes `_w5_version()` and the copy is re-made."""
        w5 = self._pflat("visbl.linear5.weight")
        if self.grad_sync is not None and self.grad_sync.master_stale and self._w5b_version != self._w5_version():
            # the 16-bit copy is invalid (something wrote linear5.weight outside the fused step) AND the fp32 master of the other
            # ranks' slices is stale: re-casting would bake stale weights in, and the remedy is a collective that this rank-local
            # condition must not trigger on one rank alone (the others would not join it: deadlock)
            raise GoalnetError("visbl.linear5.weight was written outside the fused step while the other ranks' slices of its fp32 master "
                               "are stale (GradSync(shard_linear5=True), 16-bit mode): call model.grad_sync.consolidate(model) on every "
                               "rank BEFORE editing / optimizer steps outside train_step")
        if self._w5b is None or self._w5b.numel() != w5.numel():
            self._w5b, self._w5b_version = torch.empty(w5.numel(), dtype=self._h16, device=self._device), None
        if self._w5b_version != self._w5_version():
            ops.cast_bf16(w5, self._w5b)
            self._w5b_version = self._w5_version()
        return self._w5b

    def _w5_version(self):
        """version stamps of everything a Python-side writer of linear5.weight goes through: the arena tensor and the
        Parameter (whose `.data` alias has its own counter — that is the one a torch optimizer bumps)"""
        return (self._arena._version, self.visbl.linear5.weight._version, self._load_count)

    def _padbuf(self, key, n, h, w, c):
        """Cached zero-padded bf16 activation buffer (borders/guards zeroed once, interior rewritten every step)."""
        k = (key, n, h, w, c)
        if k not in self._padbufs:
            self._padbufs[k] = ops.padded_bf16_alloc(n, h, w, c, self._device, dtype=self._h16)
        self._padgen[key] = self._padgen.get(key, 0) + 1      # backward checks that its saved operand was not overwritten
        return self._padbufs[k][1]

    def _timed(self, label, flops, fn, *args):
        """Run one kernel launch; when bench.py asked for it, bracket it with HIP events on the launching stream."""
        if self.kernel_events is None or (self.time_labels is not None and label not in self.time_labels):
            return fn(*args)
        e0 = torch.cuda.Event(enable_timing=True)
        e1 = torch.cuda.Event(enable_timing=True)
        e0.record()
        r = fn(*args)
        e1.record()
        self.kernel_events.setdefault(label, []).append((e0, e1, flops))
        return r

    @staticmethod
    def _sizes(h, w):
        h1, w1 = (h + 3) // 3 + 1, (w + 3) // 3 + 1
        return (h1, w1), (h1 - 2, w1 - 2), (h1 - 4, w1 - 4), (h1 - 6, w1 - 6)

    def _global_sums(self, partials, width):
        """ddp.SyncStats: this rank's partial rows -> one row of `width` doubles -> all-reduce(SUM) over the ranks"""
        row = torch.empty(width, dtype=torch.float64, device=self._device)
        ops.partials_sum_f64(partials, width, row)
        return self.stat_sync.all_reduce(row)

    def _fork_ok(self, n):
        """side-stream overlap for this step? Not while every kernel is being timed (bench's instrumented steps: an overlapped
        kernel's bracket would measure its neighbours too)."""
        if self.kernel_events is not None and self.time_labels is None:
            return False
        return n <= self.overlap_rows or self._large_overlap(n)

    def _large_overlap(self, n):
        """fork (and run linear5's Adam early) at this size although it is above overlap_rows? (comment at overlap_large)"""
        return self.overlap_large or (self.overlap_auto and self._precision != "fp32" and n >= 256)

    @staticmethod
    def _bwd16_ok(wc):
        """widths goalnet_bnpool_bwd_bf16p(_t) serves: three ring rows (pooled row + 4 guard pixels) of a 32-channel slice (value +
        argmax byte) in 64 KB of LDS, i.e. conv outputs up to 134 pixels wide (frames up to ~404 px); wider blocks take the fp32 kernels"""
        return 3 * (wc + 2) * 32 * 5 <= 65536

    @staticmethod
    def _p16_ok(wc, c):
        """shapes goalnet_pool_bnstats_fwd_p16 serves (32-channel slices, three conv rows in 64 KB of LDS) and whose bf16
        pooled activation the fused backward can read back"""
        return c % 32 == 0 and 3 * wc * 32 * 4 <= 65536 and AVM._bwd16_ok(wc)

    def _x6_conv(self, m, cout):
        """precision="bf16x6": does this convolution (m output pixels, cout output channels of the GEMM) run on split operands?
        Only where the 256 x 256 tile is filled; everything else runs the fp32-MFMA kernels."""
        return self._x6 and m >= 65536 and cout >= 256 and not self.x6_off

    # split operands: every helper returns (parts tensor, magnitude word or None); `_osc(a, b)` = the epilogue scale of a GEMM of the two
    def _amax_of(self, x2d, rows, c, scale=None, shift=None, bnC=0):
        if self._parts != 2:
            return None
        return ops.absmax(x2d, torch.zeros(1, dtype=torch.int32, device=x2d.device), rows, c, scale=scale, shift=shift, bnC=bnC)

    def _osc(self, amax_a, amax_b):
        return ops.split_scales(amax_a, amax_b) if self._parts == 2 else None

    def _split_w(self, w, rows, c):
        am = self._amax_of(w, rows, c)
        return ops.split_rows(self._parts, w, torch.empty(rows * self._parts * c, dtype=self._h16, device=w.device), rows, c, amax=am), am

    def _split_act(self, key, x, scale, shift, n, h, w, c):
        am = self._amax_of(x, n * h * w, c, scale=scale, shift=shift, bnC=c)
        return ops.split_padded(self._parts, x, scale, shift, self._padbuf(key, n, h, w, self._parts * c), n, h, w, c, amax=am), am

    def _split_mat(self, x2d, rows, c, scale=None, shift=None, bnC=0):
        am = self._amax_of(x2d, rows, c, scale=scale, shift=shift, bnC=bnC)
        return ops.split_rows(self._parts, x2d, torch.empty(rows * self._parts * c, dtype=self._h16, device=x2d.device), rows, c,
                              scale=scale, shift=shift, bnC=bnC, amax=am), am

    def _x6_linear5(self, n, k5):
        """precision="bf16x6": linear5's three contractions on split operands (>= 256 frames: the 256 x 256 tile)"""
        return self._x6 and ops.linear_split_ok(self._parts, n, k5, 512) and not self.x6_off and self.x6_linear5

    def _mlp_fused(self, n):
        """the one-launch fusion MLP (csrc/mlp.hip): the regression head at the reference's sub-batch sizes"""
        return n <= 16 and self.head == "regression" and self.mlp_fused

    def _bf5(self, n):
        """16-bit modes: linear5 on the 16-bit MFMA kernels? At <= 16 rows it is a pure weight stream: the fp32 weight-streaming kernels
        (csrc/skinny.hip) read the arena once, which is cheaper (and exact) compared with casting 4 K J bytes to bf16 first"""
        return self._half and (n > 16 or self.force_bf5)

    def _pair(self, n):
        """a forked LARGE step: each weight gradient goes out behind its layer's data gradient (comment in backward_device)"""
        return self._large_overlap(n) and self.overlap_pair

    def _small_bn(self, a, b, n, hc, wc, c):
        """the one-launch pool / BatchNorm kernels (csrc/pool_bn.hip, goalnet_*_fused): fp32 tensors, local statistics, few elements"""
        return (a.dtype == F32 and b.dtype == F32 and self.stat_sync is None and c <= 512 and n * hc * wc * c <= ops.SMALL_BN_ELEMS
                and self.small_bn)

    def _bn_block(self, y, n, hc, wc, c, i, save, p16=False):
        """maxpool + BN statistics of block i on conv output y (N,hc,wc,c). Returns (p, idx, mean, invstd, scale, shift).
        p16: the pooled activation is stored as bf16 (precision="bf16", blocks whose every consumer is a bf16 GEMM pass)."""
        dev = self._device
        assert p16 or y.dtype == F32
        p = torch.empty(n, hc - 2, wc - 2, c, dtype=self._h16 if p16 else F32, device=dev)
        idx = torch.empty(n, hc - 2, wc - 2, c, dtype=torch.uint8, device=dev) if save else None
        bn = getattr(self.visbl, f"bnorm{i}")
        st = torch.empty(4, c, dtype=F32, device=dev)
        count = n * (hc - 2) * (wc - 2)
        if not self.training:
            # eval(): normalise with the running statistics (a fixed affine known before the pass) -> pool and the four rows of st in
            # one launch at every shape; the buffers and num_batches_tracked stay as they are, no statistic (and no collective)
            ops.pool_bn_eval_fwd(y, p, idx, self._pflat(f"visbl.bnorm{i}.weight"), self._pflat(f"visbl.bnorm{i}.bias"),
                                 bn.running_mean, bn.running_var, BN_EPS, st, n, hc, wc, c)
            return p, idx, st
        if self._small_bn(y, p, n, hc, wc, c):
            # the reference's operating point (10 frames of 40 x 40): pool, statistics AND the finalise step in one launch
            ops.pool_bn_fwd_small(y, p, idx, self._pflat(f"visbl.bnorm{i}.weight"), self._pflat(f"visbl.bnorm{i}.bias"),
                                  bn.running_mean, bn.running_var, BN_MOMENTUM, BN_EPS, st, n, hc, wc, c)
            bn.num_batches_tracked += 1
            return p, idx, st
        # one partial row per (frame, row band): up to 8 bands per frame keep the grid full for small sub-batches
        partials = torch.empty(ops.stat_parts(8 * n) * 2 * c, dtype=torch.float64, device=dev)
        ops.pool_bnstats_fwd(y, p, idx, partials, n, hc, wc, c)
        if self.stat_sync is not None:
            partials, count = self._global_sums(partials, 2 * c), count * self.stat_sync.world
        ops.bn_finalize(partials, self._pflat(f"visbl.bnorm{i}.weight"), self._pflat(f"visbl.bnorm{i}.bias"),
                        bn.running_mean, bn.running_var, BN_MOMENTUM, BN_EPS, count, c,
                        st[0], st[1], st[2], st[3])
        bn.num_batches_tracked += 1
        return p, idx, st

    def _conv_block_fwd(self, i, x, st_in, n, hc, wc, cin, cout, save, ctx, p16, keep_split):
        """Block i (2 or 3) of VisBl: 3 x 3 convolution (+ ReLU) of block i-1's pooled activation x (N,hc,wc,cin) with that block's
        BatchNorm (st_in) folded into the operand load, then _bn_block. The convolution runs on one of three engines: 16-bit MFMA
        (precision bf16 / fp16), split operands (bf16x6 / fp16x3 where _x6_conv says so) or fp32 MFMA.
        p16: store the pooled activation in 16 bits; keep_split: backward reuses the split operand (ctx x{i-1}s, x{i-1}s_amax, x{i-1}s_gen).
        Returns (p, idx, st, xh); xh is the padded 16-bit operand the weight gradient reads again, None on the other engines."""
        dev, P, BF16 = self._device, self._pflat, self._h16
        wname, bname, xk = f"visbl.conv{i}.weight", f"visbl.conv{i}.bias", f"x{i - 1}"
        flops = 2.0 * n * hc * wc * 9 * cin * cout
        # where p is kept in bf16 AND the 256 x 256 tile computes the convolution, the conv output is stored as bf16 too:
        # rounding is monotonic, so the max-pool of the rounded values is the rounded max-pool (same p, same statistics);
        # only ties in the argmax are broken differently
        y16 = p16 and ops.conv3x3_fwd_bf16p_o16_ok(n, hc, wc, cin, cout)
        y = torch.empty(n, hc, wc, cout, dtype=BF16 if y16 else F32, device=dev)
        xh = None
        if self._half:
            xh = ops.to_bf16_padded(x, st_in[2], st_in[3], self._padbuf(xk if save else xk + "e", n, hc, wc, cin), n, hc, wc, cin)
            wb = ops.cast_bf16(P(wname), torch.empty(cout * 9 * cin, dtype=BF16, device=dev))
            self._timed("conv_fwd", flops, ops.conv3x3_fwd_bf16p_o16 if y16 else ops.conv3x3_fwd_bf16p,
                        xh, wb, P(bname), True, y, n, hc, wc, cin, cout)
        elif self._x6_conv(n * hc * wc, cout):
            xs, ax = self._split_act(xk + ("s" if save else "se"), x, st_in[2], st_in[3], n, hc, wc, cin)
            ws, aw = self._split_w(P(wname), cout * 9, cin)
            self._timed("conv_fwd", flops, ops.conv3x3_fwd_split, self._parts,
                        xs, ws, P(bname), True, y, n, hc, wc, cin, cout, self._osc(ax, aw))
            if save and keep_split:
                ctx.update({xk + "s": xs, xk + "s_amax": ax, xk + "s_gen": self._padgen[xk + "s"]})
            del xs, ws
        else:
            self._timed("conv_fwd", flops, ops.conv3x3_fwd,
                        x, st_in[2], st_in[3], P(wname), P(bname), True, y, n, hc, wc, cin, cout)
        # the conv output is only an input of the pool: backward reads the ReLU mask off p (csrc/pool_bn.hip)
        return (*self._bn_block(y, n, hc, wc, cout, i, save, p16=p16), xh)

    def forward_device(self, audio, visual, save: bool, *, fused_loss=None, caller_ticks: bool = False, fused_loss_kind=None):
        """audio (N,30,B) / None, visual (N,3,H,W): contiguous fp32 GPU tensors. Returns (out (N,), ctx); ctx is None unless `save`.
        train_step's two riders: `fused_loss` = (labels, loss, dout) — where the one-launch MLP runs, it evaluates the broadcast MSE too
        (ctx["loss_done"] says whether it did), or, with `fused_loss_kind` = (name, param, weights), that loss (ops.loss_spec);
        `caller_ticks`: the dropout draw counter is advanced by the caller, by ctx["drop_ticks"]."""
        if visual.dim() != 4 or visual.shape[1] != 3:
            raise RuntimeError(f"visual_input must be (N,3,H,W), got {tuple(visual.shape)}")
        n, _, h, w = visual.shape
        (h1, w1), (hp1, wp1), (hp2, wp2), (hp3, wp3) = self._sizes(h, w)
        if hp3 < 1 or wp3 < 1:
            raise RuntimeError(f"frames of {h}x{w} are too small for VisBl")
        bins = l1 = l2 = 0
        if self.audio_included:
            if audio is None or audio.dim() != 3 or audio.shape[0] != n or audio.shape[1] != 30:
                raise RuntimeError("audio_input must be (N,30,B) when audio_included=True")
            bins = audio.shape[2]
            l1 = (bins - 1) // 2 + 1
            l2 = (l1 - 1) // 2 + 1
        self._materialize(hp3 * wp3, l2)
        if self.grad_sync is not None:
            self.grad_sync.ensure_params_synced(self)      # first synchronised step: every rank starts from rank 0's model
        dev = self._device
        P = self._pflat
        masks, drop_ticks = self._masks(n, caller_ticks)
        ctx = {"n": n, "h": h, "w": w, "bins": bins, "visual": visual, "audio": audio, "eval": not self.training,
               "drop_ticks": drop_ticks, "loss_done": False} if save else None

        fw = 640 if self.audio_included else 512
        voff = fw - 512
        cat = torch.empty(n, fw, dtype=F32, device=dev)          # torch.cat((audio, visual), -1), utils.py:266
        mcat = torch.empty(n, fw, dtype=F32, device=dev) if save else None
        a1 = a2 = None
        ffork = _Fork(self, self._fork_ok(n) and self.audio_included)
        if self.audio_included:
            # ---- AudBl, utils.py:214-227: independent of VisBl until the concatenation -> side stream for small steps (_Fork)
            a1 = torch.empty(n, 64, l1, dtype=F32, device=dev)
            a2 = torch.empty(n, 128, l2, dtype=F32, device=dev)

            def audbl_fwd():
                ops.conv1d_fwd(audio, P("audbl.conv1.weight"), P("audbl.conv1.bias"), a1, True, n, 30, bins, 64)
                ops.conv1d_fwd(a1, P("audbl.conv2.weight"), P("audbl.conv2.bias"), a2, True, n, 64, l1, 128)
                ops.linear_fwd(a2.view(n, 128 * l2), P("audbl.linear3.weight"), P("audbl.linear3.bias"), cat[:, :128], relu=True,
                               mult_out=None if mcat is None else mcat[:, :128])
            ffork.run(audbl_fwd, audio, cat, mcat, a1, a2)

        # ---- VisBl, utils.py:172-195
        y1 = torch.empty(n, h1, w1, 64, dtype=F32, device=dev)
        ops.conv1_fwd(visual, P("visbl.conv1.weight"), P("visbl.conv1.bias"), y1, n, h, w)
        # block 1 keeps its pooled activation in fp32 also under precision="bf16": measured with bf16 p1 the forward logit
        # error more than doubles (MAE 4.7e-5 -> 1.1e-4) and after 7 Adam steps it crosses 1e-3 (3.7e-4 -> 1.1e-3) for 0.6 ms
        p1, idx1, st1 = self._bn_block(y1, n, h1, w1, 64, 1, save)
        del y1          # the conv output is only an input of the pool: backward reads the ReLU mask off p (csrc/pool_bn.hip)
        bf = self._half
        BF16 = self._h16                 # the 16-bit storage format of this model (bfloat16 or float16)
        b2, b3 = (hp1, wp1, 64, 256), (hp2, wp2, 256, 512)          # (hc, wc, cin, cout) of the two 3 x 3 blocks
        # conv2's weight gradient (3 output tiles of 256 x 256): 12.9 + 2.6 ms (split of dy2) against the fp32 kernel's 13.9 with six
        # segments — no gain; with three (fp16x3) 6.5 + 3.3 against 14-20: taken. conv3 keeps its split operands in both modes.
        p2, idx2, st2, xh1 = self._conv_block_fwd(
            2, p1, st1, n, *b2, save, ctx, p16=bf and self.act_bf16 and self._p16_ok(wp1, 256),
            keep_split=self._parts == 2 and self.x3_wgrad2)
        bf5 = self._bf5(n)
        # p3 is linear5's operand: 16-bit only where linear5 runs its 16-bit kernels (bf5), i.e. fp32 for n <= 16
        p3, idx3, st3, xh2 = self._conv_block_fwd(
            3, p2, st2, n, *b3, save, ctx, p16=bf5 and self.act_bf16 and self._p16_ok(wp2, 512), keep_split=True)

        k5 = 512 * hp3 * wp3
        if self.grad_sync is not None:
            # shard_linear5: the all-gather of the updated weights has been running under the convolutions above
            self.grad_sync.wait_weights() if bf5 else self.grad_sync.gather_master(self)
        self.last_used_w5b = bool(bf5)                  # loop.VideoTrainer: does a graph captured from this call read the bf16 copy?
        if bf5:
            xh3 = ops.bn_apply_bf16(p3, st3[2], st3[3], torch.empty(p3.shape, dtype=BF16, device=dev), 512)
            w5b = self._w5_bf16(k5)
            ops.linear_fwd_bf16(xh3.view(n, k5), w5b, P("visbl.linear5.bias"), cat[:, voff:], relu=True,
                                dropmask=masks[0], mult_out=None if mcat is None else mcat[:, voff:])
            if save:
                ctx.update(xh3=xh3, w5b=w5b)
            del xh3, w5b
        elif self._x6_linear5(n, k5):
            # BatchNorm3 is applied in fp32 on the way into the split (one fmaf per value, as the fp32 kernel's load does)
            x3s, ax = self._split_mat(p3.view(n, k5), n, k5, scale=st3[2], shift=st3[3], bnC=512)
            w5s, aw = self._split_mat(P("visbl.linear5.weight").view(512, k5), 512, k5)
            ops.linear_fwd_split(self._parts, x3s, w5s, P("visbl.linear5.bias"), cat[:, voff:], n, k5, 512, relu=True,
                                 dropmask=masks[0], mult_out=None if mcat is None else mcat[:, voff:], oscale=self._osc(ax, aw))
            if save:
                ctx.update(x3s=x3s, w5s=w5s, x3s_amax=ax, w5s_amax=aw)
            del x3s, w5s
        else:
            ops.linear_fwd(p3.view(n, k5), P("visbl.linear5.weight"), P("visbl.linear5.bias"), cat[:, voff:], relu=True,
                           scale=st3[2], shift=st3[3], bnC=512, dropmask=masks[0], mult_out=None if mcat is None else mcat[:, voff:])

        if bf and save:
            ctx.update(xh1=xh1, xh2=xh2, bf5=bf5, padgen=(self._padgen["x1"], self._padgen["x2"]))
        ffork.join()                                # the audio half of `cat` is in place

        # ---- fusion, utils.py:242-258, 269-270
        hs, ms = [cat], [mcat]
        x = cat
        fused_mlp = self._mlp_fused(n)
        if fused_mlp:
            # the reference's sub-batch size: the five layers, the Sigmoid and 4y+1 in ONE launch (csrc/mlp.hip)
            keys = ("0", "3", "6", "9", "12")
            for width in ops.MLP_WIDTHS:
                hs.append(torch.empty(n, width, dtype=F32, device=dev))
                ms.append(torch.empty(n, width, dtype=F32, device=dev) if save else None)
            logit = torch.empty(n, dtype=F32, device=dev)
            out = torch.empty(n, dtype=F32, device=dev)
            lkw = {}
            if fused_loss is not None and fused_loss_kind is not None:
                lkw = dict(loss_kind=fused_loss_kind[0], loss_param=fused_loss_kind[1], weights=fused_loss_kind[2])
            ops.mlp_fwd(cat, [P(f"fusion.{k}.weight") for k in keys], [P(f"fusion.{k}.bias") for k in keys], masks[1:5],
                        hs[1:], ms[1:], logit, out, *(fused_loss if fused_loss is not None else (None, None, None)), **lkw)
            if save:
                ctx["loss_done"] = fused_loss is not None    # train_step: the broadcast MSE rode in the same launch
            x = hs[4]
        for li, (key, width) in enumerate(() if fused_mlp else (("0", 512), ("3", 512), ("6", 256), ("9", 128))):
            hnext = torch.empty(n, width, dtype=F32, device=dev)
            m = torch.empty(n, width, dtype=F32, device=dev) if save else None
            ops.linear_fwd(x, P(f"fusion.{key}.weight"), P(f"fusion.{key}.bias"), hnext, relu=True,
                           dropmask=masks[1 + li], mult_out=m)
            hs.append(hnext); ms.append(m)
            x = hnext
        if self.head == "classifier":                    # never fused: _mlp_fused serves the regression head only
            logit = torch.empty(n, self.num_classes, dtype=F32, device=dev)
            out = torch.empty(n, self.num_classes, dtype=F32, device=dev)          # class scores 4 softmax(z) + 1
            ops.cls_head_fwd(x, P("fusion.12.weight"), P("fusion.12.bias"), logit, out)
        elif not fused_mlp:
            logit = torch.empty(n, dtype=F32, device=dev)
            out = torch.empty(n, dtype=F32, device=dev)
            ops.head_fwd(x, P("fusion.12.weight"), P("fusion.12.bias"), logit, out)
        if save:
            ctx.update(p1=p1, idx1=idx1, st1=st1, p2=p2, idx2=idx2, st2=st2, p3=p3, idx3=idx3, st3=st3,
                       a1=a1, a2=a2, hs=hs, ms=ms, logit=logit, out=out, l1=l1, l2=l2)
        self.last_logit = logit
        self.last_features = cat                    # the fusion input (N, 512 | 640): what TemporalSegmenter segments (no copy)
        return out, ctx

    def _block_bwd(self, bwd, dbn, ctx, i, n, hc, wc, c):
        """BN backward + max-pool backward + ReLU backward of block i. dbn = grad wrt the BN output (N,hc-2,wc-2,c).
        Returns dy (N,hc,wc,c) = grad wrt the conv's pre-ReLU output; writes dgamma, dbeta, dbias where bwd.G(name) says (the grad arena;
        scratch for a frozen tensor and in the inputs-only backward: the fused kernels cannot omit dgamma / dbeta).
        No bias sums where conv{i}.bias is not trained."""
        dev, G, bias = self._device, bwd.G, bwd.T(f"visbl.conv{i}.bias")
        p, idx, st = ctx[f"p{i}"], ctx[f"idx{i}"], ctx[f"st{i}"]
        npix = n * (hc - 2) * (wc - 2)
        small = self._small_bn(dbn, p, n, hc, wc, c) and not (self._half and i > 1)
        frozen = ctx["eval"]          # the forward ran under eval(): st holds the running statistics, constants of the forward
        if small:
            # the reference's operating point: reduce + finalise in one launch (csrc/pool_bn.hip "small shapes"), then the rolling-row
            # max-pool / ReLU backward (13 us; the one-launch 9-window gather from global memory, ops.bnpool_bwd_small, measured 35), its
            # bias-gradient rows summed at the end of backward on the side stream
            coef3 = torch.empty(3 * c, dtype=F32, device=dev)
            (ops.bn_bwd_reduce_small_eval if frozen else ops.bn_bwd_reduce_small)(
                dbn, p, st[0], st[1], self._pflat(f"visbl.bnorm{i}.weight"), G(f"visbl.bnorm{i}.weight"), G(f"visbl.bnorm{i}.bias"),
                coef3, n, hc, wc, c)
            dy = torch.empty(n, hc, wc, c, dtype=F32, device=dev)
            dparts = torch.empty(ops.stat_parts(8 * n) * c, dtype=torch.float64, device=dev)
            ops.bnpool_bwd(dbn, p, idx, coef3, dy, dparts, n, hc, wc, c)
            # the bias gradients' row sums feed nothing but Adam: conv3's and conv2's go out together at the end of backward (one
            # launch, side stream); conv1's is written by goalnet_conv1_wgrad from its own sums of dy
            if i > 1 and bias:
                bwd.dbias[i] = (dparts, c)
            return dy
        coef3 = torch.empty(3 * c, dtype=F32, device=dev)
        partials = torch.empty(ops.stat_parts(npix // 64) * 2 * c, dtype=torch.float64, device=dev)
        ops.bn_bwd_reduce(dbn, p, st[0], st[1], partials, npix, c)
        if frozen:
            # dp = gamma invstd dz: no batch means to subtract, hence no cross-rank sums either
            ops.bn_bwd_finalize_eval(partials, self._pflat(f"visbl.bnorm{i}.weight"), st[1], c,
                                     G(f"visbl.bnorm{i}.weight"), G(f"visbl.bnorm{i}.bias"), coef3)
        else:
            ops.bn_bwd_finalize(partials, self._pflat(f"visbl.bnorm{i}.weight"), st[0], st[1], npix, c,
                                G(f"visbl.bnorm{i}.weight"), G(f"visbl.bnorm{i}.bias"), coef3)
        if self.stat_sync is not None and not frozen:
            # dgamma / dbeta above are this rank's sums (the gradient all-reduce adds the ranks up); the dx coefficients
            # need the sums over every rank's pixels
            scratch = torch.empty(2 * c, dtype=F32, device=dev)
            ops.bn_bwd_finalize(self._global_sums(partials, 2 * c), self._pflat(f"visbl.bnorm{i}.weight"), st[0], st[1],
                                npix * self.stat_sync.world, c, scratch[:c], scratch[c:], coef3)
        dparts = torch.empty(ops.stat_parts(8 * n) * c, dtype=torch.float64, device=dev)        # dbias partials per (frame, row band)
        if self._half and i > 1 and self._bwd16_ok(wc):
            # blocks 2, 3: the only consumers of dy are the bf16 GEMMs -> written once, as bf16, in their padded layout
            dy = self._padbuf(f"dy{i}", n, hc, wc, c)
            ops.bnpool_bwd_bf16p(dbn, p, idx, coef3, None, dy, dparts, n, hc, wc, c)
        elif self._half and i > 1:
            # frames wider than ~416 px: the rolling LDS rows of the fused bf16 kernel do not fit; fp32 kernel (dz and p are
            # fp32 for such widths, see _p16_ok / backward_device) + one cast pass into the padded layout
            dy32 = torch.empty(n, hc, wc, c, dtype=F32, device=dev)
            ops.bnpool_bwd(dbn, p, idx, coef3, dy32, dparts, n, hc, wc, c)
            dy = ops.to_bf16_padded(dy32, None, None, self._padbuf(f"dy{i}", n, hc, wc, c), n, hc, wc, c)
        else:
            dy = torch.empty(n, hc, wc, c, dtype=F32, device=dev)
            ops.bnpool_bwd(dbn, p, idx, coef3, dy, dparts, n, hc, wc, c)
        if not bias:
            return dy
        if i == 1:
            # conv1's bias gradient is written a second time by goalnet_conv1_wgrad (on the main stream, later): keep this
            # one on the main stream too so that the order of the two writers does not depend on the schedule
            ops.partials_sum(dparts, ops.stat_parts(8 * n), c, c, G(f"visbl.conv{i}.bias"))
        else:
            bwd.fork.run(lambda: ops.partials_sum(dparts, ops.stat_parts(8 * n), c, c, G(f"visbl.conv{i}.bias")), dparts)
        return dy

    def _conv_block_bwd(self, bwd, i, dbn, ctx, n, hc, wc, cin, cout, wt, flipped, wait_ev, pair, out16, split_dgrad, after_block=None,
                        dgrad=True):
        """Backward of block i (2 or 3): from dbn = grad wrt its BatchNorm output (N,hc-2,wc-2,cout) to the grad wrt block i-1's
        BatchNorm output (N,hc,wc,cin), returned. _block_bwd, then conv{i}'s weight gradient (side stream, into the arena) and data
        gradient on the engine its forward ran on (_conv_block_fwd).
        wt: buffer for the flipped weight (csrc/layout.hip); flipped: the joint early launch fills it, and wait_ev is that launch's
        event where this block is its first reader. pair: the weight gradient goes out behind the data gradient (backward_device).
        out16: the data gradient may be stored in 16 bits; split_dgrad: it runs on split operands where the forward saved them;
        after_block(): called between _block_bwd and the weight gradient. No weight-gradient launch where conv{i}.weight is not trained
        (bwd.T); dgrad=False: nothing beneath this block wants a gradient — no data gradient, None is returned."""
        dev, P, G, fork = self._device, self._pflat, bwd.G, bwd.fork
        wname, xs = f"visbl.conv{i}.weight", f"x{i - 1}s"
        flops = 2.0 * n * hc * wc * 9 * cin * cout           # the same for the weight gradient and the data gradient
        dy = self._block_bwd(bwd, dbn, ctx, i, n, hc, wc, cout)
        if after_block:
            after_block()
        split = not self._half and xs in ctx           # the forward ran this convolution on split operands and kept them
        if not bwd.T(wname):
            wg = None
            if split and split_dgrad and dgrad:
                dys, ady = self._split_act(f"dy{i}s", dy, None, None, n, hc, wc, cout)
        elif self._half:
            wg, keep = (ops.conv3x3_wgrad_bf16, ctx[f"xh{i - 1}"], dy, G(wname), n, hc, wc, cin, cout), (dy,)
        elif split:
            # the weight gradient and the data gradient read the gradient as 16-bit parts in the padded layout: one split pass
            dys, ady = self._split_act(f"dy{i}s", dy, None, None, n, hc, wc, cout)
            osc_w = self._osc(ady, ctx[xs + "_amax"])
            # osc_w is kept too: the side stream reads it
            wg, keep = (ops.conv3x3_wgrad_split, self._parts, ctx[xs], dys, G(wname), n, hc, wc, cin, cout, osc_w), (dys, osc_w)
        else:
            st_in = ctx[f"st{i - 1}"]
            wg, keep = (ops.conv3x3_wgrad, ctx[f"p{i - 1}"], st_in[2], st_in[3], dy, G(wname), n, hc, wc, cin, cout), (dy,)

        def wgrad():
            if wg is not None:
                fork.run(lambda: self._timed("conv_wgrad", flops, *wg), *keep)
        if not pair:
            wgrad()
        if not dgrad:
            if pair:
                wgrad()
            return None
        if flipped:
            fork.wait(wait_ev)                       # None: an earlier block's wait covered the joint flip launch
        else:
            ops.conv3x3_weight_flip(P(wname), wt, cout, cin)
        o16 = out16 and ops.conv3x3_fwd_bf16p_o16_ok(n, hc, wc, cout, cin)
        dx = torch.empty(n, hc, wc, cin, dtype=self._h16 if o16 else F32, device=dev)
        if self._half:
            wtb = ops.cast_bf16(wt, torch.empty(wt.shape, dtype=self._h16, device=dev))
            self._timed("conv_dgrad", flops, ops.conv3x3_fwd_bf16p_o16 if o16 else ops.conv3x3_fwd_bf16p,
                        dy, wtb, None, False, dx, n, hc, wc, cout, cin)
        elif split and split_dgrad:
            wts, awt = self._split_w(wt, cin * 9, cout)
            self._timed("conv_dgrad", flops, ops.conv3x3_fwd_split, self._parts,
                        dys, wts, None, False, dx, n, hc, wc, cout, cin, self._osc(ady, awt))
        else:
            self._timed("conv_dgrad", flops, ops.conv3x3_fwd, dy, None, None, wt, None, False, dx, n, hc, wc, cout, cin)
        if pair:
            wgrad()                                  # behind the data gradient: runs under the next block's BatchNorm / pool passes
        return dx

    def backward_device(self, ctx, dout, on_bucket=None, after_linear5=None, inputs=None, params=True, reduce=0, frozen=None,
                        fused_w5=None):
        """dout (N,) GPU. Fills the gradient arena (the slot of every TRAINABLE tensor is overwritten). `inputs` = (audio?, visual?): also
        follow the data-gradient chain into the inputs and return (d_audio (N,30,B) | None, d_visual (N,3,H,W) | None) — `reduce`=1:
        d_visual is max_ci |.|, (N,H,W).
        `frozen`: names of the tensors that are not trained (default: those whose nn.Parameter has requires_grad=False, read here, at
        the start of the backward). A frozen tensor gets no gradient: a launch whose only outputs are frozen gradients is not issued,
        what a fused kernel cannot omit goes to scratch (_Bwd.G), and each branch of the data-gradient chain stops below its lowest trainable
        tensor unless an input gradient is asked for. Gradients of trainable tensors are the same bits either way.
        params=False: the inputs-only backward — every tensor counts as frozen, and neither the arena nor any .grad is touched.
        `on_bucket(k)` is called when
        bucket k of ddp.bucket_slices() is complete (0: fusion+audbl+linear5.bias, 1: linear5.weight, 2: rest).
        `after_linear5(fork)`: called once linear5's weight gradient (side stream) and data gradient (main stream) are both
        enqueued — from there on nothing reads linear5.weight or its 16-bit copy again in this step (train_step's early Adam).
        `fused_w5(dz5, p3, scale, shift)` (fp32 engine, train_step's rule epi_fuse_dw_adam): called on the main stream INSTEAD of
        linear5's weight gradient launch and AFTER its data gradient, the last reader of the old weights; it computes the gradient and
        applies it in one launch, and the gradient slot of visbl.linear5.weight is not written.
        Every refusal is raised before the first launch or allocation, as on the C side: a refused call leaves the gradient arena and
        both streams as they were."""
        need_aud, need_vis = inputs if inputs is not None else (False, False)
        need_aud = need_aud and self.audio_included
        train = frozenset()
        if params:
            self._refuse_averaged("a parameter backward")
            frozen = self._frozen_names() if frozen is None else frozenset(frozen)
            self._check_freeze(frozen)
            train = frozenset(s.name for s in self._specs) - frozen
        # the operands the forward left in the cached padded buffers must still be the ones this ctx saved
        if self._half and ctx["padgen"] != (self._padgen["x1"], self._padgen["x2"]):
            raise RuntimeError("precision='bf16': a second training-mode forward overwrote the saved bf16 operands before "
                               "backward ran; call backward after each forward (as the reference's loop does)")
        for i in (3, 2):
            # split operands: the weight gradient of conv{i} is their only reader in backward, and a trained weight means the block runs
            xs = f"x{i - 1}s"
            if not self._half and xs in ctx and f"visbl.conv{i}.weight" in train and ctx[xs + "_gen"] != self._padgen[xs]:
                raise RuntimeError(f"precision='{self.precision}': a second training-mode forward overwrote the saved split operands "
                                   "before backward ran; call backward after each forward (as the reference's loop does)")
        if params:
            self._ensure_garena()
            self._bwd_frozen = frozen
            if self._norm_of_acc:
                self._norm_of_acc = False
        dev = self._device
        n, h, w = ctx["n"], ctx["h"], ctx["w"]
        # small steps: weight / bias gradients and the AudBl branch run on a side stream under the dX chain (_Fork)
        bwd = _Bwd(self, train, _Fork(self, self._fork_ok(n) and dout.is_cuda))
        fork, T, G, any_T = bwd.fork, bwd.T, bwd.G, bwd.any_T
        (h1, w1), (hp1, wp1), (hp2, wp2), (hp3, wp3) = self._sizes(h, w)
        P = self._pflat
        # what each stage of the VisBl chain is needed for: block i's BatchNorm / pool / ReLU backward (b_i) feeds its own parameters and
        # everything beneath; conv_i's data gradient (d_i) feeds block i-1
        need_b1 = need_vis or any_T("visbl.bnorm1", "visbl.conv1")
        need_b2 = need_b1 or any_T("visbl.bnorm2", "visbl.conv2")          # = conv3's data gradient is needed
        need_b3 = need_b2 or any_T("visbl.bnorm3", "visbl.conv3")          # = linear5's data gradient is needed
        train_w5 = T("visbl.linear5.weight")
        need_audbl = self.audio_included and (need_aud or any_T("audbl.linear3", "audbl.conv2", "audbl.conv1"))
        need_cat = need_audbl or need_b3 or train_w5 or T("visbl.linear5.bias")      # the gradient behind `cat` is needed
        d_audio = torch.empty(n, 30, ctx["bins"], dtype=F32, device=dev) if need_aud else None
        d_visual = None
        hs, ms = ctx["hs"], ctx["ms"]
        # Large steps (forked by _large_overlap): the side stream's pieces are paired with main-stream work of the OTHER kind — linear5's
        # Adam (HBM-bound) goes out when conv3's data gradient (MFMA-bound) starts, each weight gradient (MFMA-bound) when its layer's
        # data gradient is enqueued, i.e. under the BatchNorm / pool passes of the next block (HBM-bound). Small steps keep the weight
        # gradient FIRST: there the chain is latency-bound and everything off it should start as early as it can. Same kernels, same
        # results either way. Measured (1 024 frames, alternating runs): fp16x3 178.5 -> 176.9 ms, bf16 70.6 -> 70.6 (GOALNET_OVERLAP_PAIR=0
        # restores the weight-gradient-first order).
        pair = fork.enabled and self._pair(n)
        deferred_l5 = []

        def bucket_done(k):
            if on_bucket:
                fork.join()                     # the bucket's gradients may have been written on the side stream
                on_bucket(k)

        # the data gradients of conv3 / conv2 read the weights flipped (csrc/layout.hip); the flips depend on nothing but the
        # weights, so in a small step both go out FIRST, in one launch on the side stream, off the dX chain (where both data gradients
        # run; where only conv3's does, its block flips its own weight)
        wt3 = torch.empty(512 * 9 * 256, dtype=F32, device=dev) if need_b2 else None
        wt2 = torch.empty(256 * 9 * 64, dtype=F32, device=dev) if need_b1 else None
        flips_ev = None
        flips_early = fork.enabled and need_b1
        if flips_early:
            _, flips_ev = fork.run_marked(lambda: ops.conv3x3_weight_flip2(P("visbl.conv3.weight"), wt3, 512, 256,
                                                                          P("visbl.conv2.weight"), wt2, 256, 64), wt3, wt2)
        # head + fusion MLP (reverse of utils.py:242-258)
        fused_mlp = self._mlp_fused(n) and ms[0] is not None
        dz = torch.empty(n, hs[0].shape[1] if fused_mlp else 128, dtype=F32, device=dev)
        if fused_mlp:
            # one launch: the five layers' dW / db, the dX chain down to the gradient behind `cat`, and linear5's bias gradient
            keys = ("0", "3", "6", "9", "12")
            ops.mlp_bwd(dout, ctx["out"], hs, ms, [P(f"fusion.{k}.weight") for k in keys], [G(f"fusion.{k}.weight") for k in keys],
                        [G(f"fusion.{k}.bias") for k in keys], dz, G("visbl.linear5.bias"), dz.shape[1] - 512)
        elif self.head == "classifier":
            ops.cls_head_bwd(dout.view(n, self.num_classes), ctx["out"], hs[4], P("fusion.12.weight"), ms[4], dz,
                             G("fusion.12.weight"), G("fusion.12.bias"))
        else:
            ops.head_bwd(dout, ctx["out"], hs[4], P("fusion.12.weight"), ms[4], dz, G("fusion.12.weight"), G("fusion.12.bias"))
        chain = True                               # dz is still wanted by something beneath
        lower = ("fusion.6", "fusion.3", "fusion.0")
        for k, (key, li) in enumerate(() if fused_mlp else (("9", 3), ("6", 2), ("3", 1), ("0", 0))):
            x_in, m_in = hs[li], ms[li]
            if any_T(f"fusion.{key}"):
                fork.run(lambda dz=dz, x_in=x_in, key=key: ops.linear_bwd_dw(dz, x_in, G(f"fusion.{key}.weight"), db=G(f"fusion.{key}.bias")), dz)
            if not (need_cat or any_T(*lower[k:])):
                chain = False                      # nothing trainable beneath this layer: the chain ends here
                break
            dprev = torch.empty(n, x_in.shape[1], dtype=F32, device=dev)
            ops.linear_bwd_dx(dz, P(f"fusion.{key}.weight"), dprev, mult=m_in)
            dz = dprev
        chain = chain and need_cat
        voff = dz.shape[1] - 512
        dz5 = dz[:, voff:]                                     # grad wrt linear5 pre-activation (where the chain got this far)

        if chain and need_audbl:
            l1, l2, bins = ctx["l1"], ctx["l2"], ctx["bins"]
            conv_a1 = need_aud or any_T("audbl.conv1")                 # conv1's backward runs
            conv_a2 = conv_a1 or any_T("audbl.conv2")                  # conv2's backward (and linear3's data gradient) runs

            def audbl_bwd():                       # the whole AudBl backward hangs off dz and feeds nothing but its own gradients (and d_audio)
                dza = dz[:, :128]
                a2f = ctx["a2"].view(n, 128 * l2)
                if any_T("audbl.linear3"):
                    ops.linear_bwd_dw(dza, a2f, G("audbl.linear3.weight"), db=G("audbl.linear3.bias"))
                if not conv_a2:
                    return
                da2 = torch.empty(n, 128 * l2, dtype=F32, device=dev)
                ops.linear_bwd_dx(dza, P("audbl.linear3.weight"), da2, mult=None)
                da1 = torch.empty(n, 64, l1, dtype=F32, device=dev) if conv_a1 else None
                # few frames: a Conv1d layer's backward is one launch, its ReLU backward folded into the dz load, where the dz rows of a
                # weight-gradient block fit LDS (n * l1 <= 1536 for conv1, n * l2 <= 3072 for conv2: every n < 64 at 30 bins, n <= 51 at
                # 60); otherwise, as from 64 frames on, ReLU backward + the multi-launch form, which has no such limit
                if ops.conv1d_bwd_small_ok(n, 64, l1, 128):
                    ops.conv1d_bwd_small(ctx["a1"], da2, ctx["a2"], P("audbl.conv2.weight"), da1, G("audbl.conv2.weight"), G("audbl.conv2.bias"), n, 64, l1, 128)
                else:
                    ops.relu_bwd(da2, a2f, da2)
                    ops.conv1d_bwd(ctx["a1"], da2, P("audbl.conv2.weight"), da1, G("audbl.conv2.weight"), G("audbl.conv2.bias"), n, 64, l1, 128)
                if not conv_a1:
                    return
                if ops.conv1d_bwd_small_ok(n, 30, bins, 64):
                    ops.conv1d_bwd_small(ctx["audio"], da1, ctx["a1"], P("audbl.conv1.weight"), d_audio, G("audbl.conv1.weight"), G("audbl.conv1.bias"), n, 30, bins, 64)
                else:
                    ops.relu_bwd(da1, ctx["a1"], da1)
                    ops.conv1d_bwd(ctx["audio"], da1, P("audbl.conv1.weight"), d_audio, G("audbl.conv1.weight"), G("audbl.conv1.bias"), n, 30, bins, 64)
            fork.run(audbl_bwd, dz, d_audio)
        if chain and not fused_mlp and T("visbl.linear5.bias"):
            fork.run(lambda: ops.colsum(dz5, G("visbl.linear5.bias")), dz)
        bucket_done(0)

        # linear5 (utils.py:191): dW straight into the arena, dX = grad wrt bnorm3's output
        k5 = 512 * hp3 * wp3
        bf = self._half
        # precision="bf16" / "fp16": where the 256 x 256 tile serves the data-gradient GEMM, the gradient wrt a BatchNorm output is
        # stored as bf16 (fp32 accumulators rounded once, at the store): its only readers are the two HBM-bound passes of
        # _block_bwd, and the GEMMs behind them consume bf16 anyway
        dz16 = bf and self.grad_bf16
        dbn3 = None
        if chain and (train_w5 or need_b3):
            p3f = ctx["p3"].view(n, k5)
            st3 = ctx["st3"]
            o16_3 = dz16 and ctx["bf5"] and self._bwd16_ok(wp2) and ops.linear_bwd_dx_bf16_o16_ok(n, k5, 512)
            if need_b3:
                dbn3 = torch.empty(n, hp3, wp3, 512, dtype=self._h16 if o16_3 else F32, device=dev)

            def linear5_done():
                if after_linear5 and train_w5:
                    # pair: linear5's Adam starts behind block 3's _block_bwd, beside conv3's data gradient (where that block runs)
                    deferred_l5.append(after_linear5) if (pair and need_b3) else after_linear5(fork)
            if bf and ctx["bf5"]:
                dz5b = ops.cast_bf16(dz5.contiguous(), torch.empty(n, 512, dtype=self._h16, device=dev))
                if train_w5:
                    fork.run(lambda: ops.linear_bwd_dw_bf16(dz5b, ctx["xh3"].view(n, k5), G("visbl.linear5.weight")), dz5b)
                bucket_done(1)
                if not need_b3:
                    pass
                elif o16_3:
                    ops.linear_bwd_dx_bf16_o16(dz5b, ctx["w5b"], dbn3.view(n, k5))
                else:
                    ops.linear_bwd_dx_bf16(dz5b, ctx["w5b"], dbn3.view(n, k5), mult=None)
            elif "x3s" in ctx:
                dz5s, adz = self._split_mat(dz5, n, 512)
                if train_w5:
                    osc_w = self._osc(adz, ctx["x3s_amax"])
                    fork.run(lambda: ops.linear_bwd_dw_split(self._parts, dz5s, ctx["x3s"], G("visbl.linear5.weight"), n, k5, 512, oscale=osc_w), dz5s, osc_w)      # osc_w too: the side stream reads it (kept alive until the join)
                bucket_done(1)
                if need_b3:
                    ops.linear_bwd_dx_split(self._parts, dz5s, ctx["w5s"], dbn3.view(n, k5), n, k5, 512, oscale=self._osc(adz, ctx["w5s_amax"]))
            else:
                fuse5 = fused_w5 is not None and train_w5
                if train_w5 and not fuse5:
                    fork.run(lambda: ops.linear_bwd_dw(dz5, p3f, G("visbl.linear5.weight"), scale=st3[2], shift=st3[3], bnC=512), dz)
                bucket_done(1)
                if need_b3:
                    ops.linear_bwd_dx(dz5, P("visbl.linear5.weight"), dbn3.view(n, k5), mult=None)
                if fuse5:
                    fused_w5(dz5, p3f, st3[2], st3[3])      # updates linear5.weight in place: behind its last reader of the step
            linear5_done()
        else:
            bucket_done(1)

        b2, b3 = (hp1, wp1, 64, 256), (hp2, wp2, 256, 512)          # (hc, wc, cin, cout) of the two 3 x 3 blocks
        dbn2 = dbn1 = None
        if dbn3 is not None:
            # block 3 (utils.py:184-187): the first reader of the flipped weights (waits for the joint early launch). Its data gradient
            # is kept in 16 bits where BLOCK 2's fused backward reads that (_bwd16_ok of block 2's width). pair: linear5's Adam starts
            # behind _block_bwd, beside conv3's data gradient
            dbn2 = self._conv_block_bwd(bwd, 3, dbn3, ctx, n, *b3, wt3, flips_early, flips_ev, pair, out16=dz16 and self._bwd16_ok(wp1),
                                        split_dgrad=True, after_block=lambda: [cb(fork) for cb in deferred_l5], dgrad=need_b2)
        del dbn3
        if dbn2 is not None:
            # block 2 (utils.py:179-182): no wait (conv3's covered the joint flip launch); dbn1 is always fp32, its consumer is block 1's
            # fp32 path; fp16x3: the split gradient is there already (weight gradient) -> 128 x 64 tile, three segments
            dbn1 = self._conv_block_bwd(bwd, 2, dbn2, ctx, n, *b2, wt2, flips_early, None, pair, out16=False,
                                        split_dgrad=self.x3_dgrad2, dgrad=need_b1)
        del dbn2

        if dbn1 is not None:
            # block 1 (utils.py:174-177); conv1's input gradient only where it was asked for (dy1 is fp32 in every precision)
            train_c1 = any_T("visbl.conv1")
            dy1 = self._block_bwd(bwd, dbn1, ctx, 1, n, h1, w1, 64)
            if train_c1:
                ops.conv1_wgrad(ctx["visual"], dy1, G("visbl.conv1.weight"), G("visbl.conv1.bias"), n, h, w)
            if need_vis:
                d_visual = ops.conv1_dgrad(dy1, P("visbl.conv1.weight"), torch.empty((n, h, w) if reduce else (n, 3, h, w), dtype=F32, device=dev),
                                           reduce, n, h, w)
        if len(bwd.dbias) == 2:
            (d3, _), (d2, _) = bwd.dbias[3], bwd.dbias[2]
            fork.run(lambda: ops.partials_sum2(d3, 512, G("visbl.conv3.bias"), d2, 256, G("visbl.conv2.bias")), d3, d2)
        else:
            # one of the two blocks did not run or does not train its bias: the same column sums, one array
            for i, (dp, c) in bwd.dbias.items():
                fork.run(lambda i=i, dp=dp, c=c: ops.partials_sum(dp, ops.stat_parts(8 * n), c, c, G(f"visbl.conv{i}.bias")), dp)
        fork.join()                                 # every gradient is in the arena before anything downstream (Adam, all-reduce) reads it
        if on_bucket:
            on_bucket(2)
        return d_audio, d_visual

    # ------------------------------------------------------------------------------------------
    # drop-in surface: model(audio_input, visual_input)
    # ------------------------------------------------------------------------------------------
    def _to_device_inputs(self, audio_input, visual_input):
        self._require_device()
        if not torch.is_tensor(visual_input):
            raise TypeError("visual_input must be a tensor (N,3,H,W)")
        src_dev = visual_input.device
        vis = visual_input.detach().to(device=self._device, dtype=F32).contiguous()
        aud = None
        if self.audio_included:
            if not torch.is_tensor(audio_input):
                raise TypeError("audio_input must be a tensor (N,30,B) when audio_included=True")
            aud = audio_input.detach().to(device=self._device, dtype=F32).contiguous()
        return aud, vis, src_dev

    def forward(self, audio_input, visual_input):
        """utils.py:260-272. Accepts the CPU tensors the reference's scripts pass (H2D inside) or GPU tensors; the
        (N,1) result is returned on the inputs' device, attached to autograd when grad mode is on."""
        aud, vis, src_dev = self._to_device_inputs(audio_input, visual_input)
        need_grad = torch.is_grad_enabled()
        self._materialize_for(aud, vis)
        if not need_grad:
            out, _ = self.forward_device(aud, vis, save=False)
            return out.view(-1, self.num_classes).to(src_dev)
        params = [getattr(*self._module_of(s.name)) for s in self._specs]
        self._check_freeze([s.name for s, prm in zip(self._specs, params) if not prm.requires_grad])
        # inputs that require grad travel through autograd as they came (any device, any float type); their gradient is returned there
        aud_in = audio_input if (self.audio_included and audio_input.requires_grad) else None
        vis_in = visual_input if visual_input.requires_grad else None
        return _AVMFunction.apply(self, aud, vis, src_dev, aud_in, vis_in, *params)

    def _materialize_for(self, aud, vis):
        """first forward: materialise the Lazy parameters (shapes depend on H, W, B)"""
        if self._materialized:
            return
        (_, _), _, _, (hp3, wp3) = self._sizes(vis.shape[2], vis.shape[3])
        l2 = 0
        if self.audio_included:
            l2 = (((aud.shape[2] - 1) // 2 + 1) - 1) // 2 + 1
        self._materialize(hp3 * wp3, l2)

    # ------------------------------------------------------------------------------------------
    # input gradients on the device: d(sum_i w_i out_i) / d(audio, visual) — saliency, robustness probes, input-space regularisers
    # ------------------------------------------------------------------------------------------
    def _input_backward(self, audio, visual, weights, reduce):
        aud, vis, _ = self._to_device_inputs(audio, visual)
        self._materialize_for(aud, vis)
        out, ctx = self.forward_device(aud, vis, save=True)
        self.last_ctx = ctx if self.keep_ctx else None
        if weights is None:
            dout = torch.ones(out.numel(), dtype=F32, device=self._device)
        else:
            if not torch.is_tensor(weights) or weights.numel() != out.numel():
                raise RuntimeError(f"weights must be a tensor of {out.numel()} elements ((N,), or (N, C) for the classifier head)")
            dout = weights.detach().to(device=self._device, dtype=F32).contiguous().view(-1)
        lscale = self._loss_scale_for(ctx["n"])
        if lscale != 1.0:                                 # fp16: scaled through the 16-bit chain, divided out of the result
            dout = ops.scale_(dout.clone(), lscale)
        d_aud, d_vis = self.backward_device(ctx, dout, inputs=(True, True), params=False, reduce=reduce)
        if lscale != 1.0:
            ops.scale_(d_vis.view(-1), 1.0 / lscale)
            if d_aud is not None:
                ops.scale_(d_aud.view(-1), 1.0 / lscale)
        return d_aud, d_vis

    def input_gradients(self, audio, visual, weights=None):
        """(d_audio (N,30,B) | None, d_visual (N,3,H,W)): the gradient of sum_i weights_i * out_i wrt the inputs, as fp32 GPU tensors, with
        no host synchronisation. `weights`: (N,) — (N, C) for the classifier head — default ones. One forward and an INPUTS-ONLY
        backward: the data-gradient chain alone, no weight-gradient launch, and the gradient arena and every parameter's .grad are left
        exactly as they were. Equal bit for bit to what `model(audio, visual)` followed by autograd gives for the same weights.
        Like every forward here, a train-mode call moves the BatchNorm running statistics and draws dropout."""
        return self._input_backward(audio, visual, weights, 0)

    def saliency(self, audio, visual, weights=None, reduce="absmax"):
        """(aud_map (N,30,B) | None, vis_map): |d_audio| and, with reduce="absmax", vis_map (N,H,W) = max over the colour channels of
        |d_visual| (written by the data-gradient kernel itself, the (N,3,H,W) gradient is never stored); reduce="none": the raw
        (N,3,H,W) gradient of input_gradients(). GPU tensors, no host synchronisation.
        PER-FRAME ATTRIBUTION NEEDS model.eval(): in train mode BatchNorm normalises with the statistics of the batch, so every
        frame's score depends on every frame's pixels and the map of frame i mixes in the other frames. A train-mode call also moves
        the running statistics and draws dropout, as every forward here does."""
        if reduce not in ("absmax", "none"):
            raise ValueError("reduce must be 'absmax' or 'none'")
        d_aud, d_vis = self._input_backward(audio, visual, weights, 1 if reduce == "absmax" else 0)
        return (None if d_aud is None else d_aud.abs_()), d_vis

    # ------------------------------------------------------------------------------------------
    # device-resident fused train step: forward, broadcast MSE, backward, Adam
    # ------------------------------------------------------------------------------------------
    def train_step(self, audio, visual, labels, lr=1e-3, betas=(0.9, 0.999), eps=1e-8, _loop_tick=(0, 0), _scatter=None, *,
                   loss="mse_bcast", loss_param=None, weights=None, optim=None, ema=None, accumulate=1):
        """main.py:187-193 on GPU tensors. Returns (loss (1,), pred (N,)) as GPU tensors, no host sync.
        `accumulate` (EXTENSION): k >= 1 — one optimizer step per WINDOW of k calls. Every call is a micro-step: forward,
        loss, backward into the gradient arena, scatter and the counters' tick as ever, then ONE launch adds gradient / k into the
        arena `_gacc` (accum_of; the window's first call overwrites it). Only the window's last call updates — the same launches, reading
        `_gacc` with grad_scale 1 — and moves the average and the step counter: schedules, the average and the bias corrections count
        windows, the clipping norm is the accumulated gradient's. 1: exactly the step without the argument, no arena. k > 1 switches the
        early Adam and the epilogue-fused update off (as `optim` does), refuses precision="fp16" and an attached grad_sync / stat_sync,
        and k and the frozen set may not change inside a window (accum_position).
        `optim` (EXTENSION): optim.OptimOptions — weight decay, gradient-norm clipping, a learning-rate schedule on
        `lr`. None or trivial options: exactly the step without the argument. Otherwise the update is one launch after backward
        (optim_step_path): no early Adam, no update in linear5's weight-gradient epilogue.
        `ema` (EXTENSION): optim.EmaOptions — the average of the weights in the arena `_ema` (ema_of, averaged()) takes
        this step in: one launch over the trainable ranges behind every update of the step, in front of the counters' launch. None:
        exactly the step without the argument. The average observes: early Adam and the epilogue-fused update run as without it.
        `loss` (EXTENSION): "mse_bcast" is the reference's nn.MSELoss with its (n,1) x (n,) broadcast; "mse", "l1",
        "smooth_l1" (loss_param = beta, default 1) are the per-frame losses mean(w_i l_i) with optional fp32 `weights` (N,); "rank" is the
        pairwise logistic loss over the pairs with y_i > y_j. Up to 16 frames the loss rides in the fused MLP launch, above it is
        ops.frame_loss; everything after dL/dpred is the same for every loss. Global-batch mode keeps the default loss.
        `_loop_tick`: (frames, sub-batches) the caller's loop counters advance by (loop.VideoTrainer); `_scatter(loss, pred)` -> row-copy
        segments (ops.rows_copy_batch form, cursors as they stand BEFORE the tick) that the step's last launch writes before it advances
        the counters (the per-video predictions / losses arrays of loop.VideoTrainer).
        fp32 steps of >= 256 frames in which every tensor trains and no gradient is exchanged (epi_fuse_dw_adam) update
        visbl.linear5.weight inside its weight-gradient GEMM: that tensor's slot of the gradient arena is then NOT written, and
        grad_of("visbl.linear5.weight") returns whatever an earlier backward left there. keep_ctx = True or epi_fuse = False keep it."""
        loss_kind = loss
        ops.loss_spec(loss_kind, loss_param, weights is not None, self.head)       # ValueError before anything is launched
        k = accum_count(accumulate)
        self._check_accumulate(k)                       # GoalnetError before anything is launched
        opt_on = optim_step_path(optim, sharded=bool(getattr(self.grad_sync, "shard_linear5", False)))
        ema_on = ema_step_path(ema, sharded=bool(getattr(self.grad_sync, "shard_linear5", False)))
        self._refuse_averaged("train_step")
        n0 = visual.shape[0]
        if weights is not None:
            if not (torch.is_tensor(weights) and weights.dtype == F32 and weights.numel() == n0):
                raise RuntimeError(f"weights must be a float32 tensor of {n0} elements")
        if loss_kind != "mse_bcast" and self.stat_sync is not None:
            raise GoalnetError("global-batch mode is defined for the broadcast MSE only: loss='mse_bcast'")
        if not torch.is_tensor(labels) or labels.numel() != n0:
            raise RuntimeError(f"labels must be a tensor of {n0} elements, one per frame")
        # the inputs as forward() takes them, the labels as one flat row: any device, any float or integer type, any strides. The kernels
        # read bare pointers and element counts. Contiguous fp32 tensors on the device pass through as they are (no copy, no launch).
        audio, visual, _ = self._to_device_inputs(audio, visual)
        labels = labels.detach().to(device=self._device, dtype=F32).reshape(-1).contiguous()
        if weights is not None:
            weights = weights.detach().to(self._device).reshape(-1).contiguous()
        frozen = self._frozen_names()                   # requires_grad=False: no gradient, no update, no step counted
        self._check_freeze(frozen)
        plain = self._plain_step(frozen)                # every tensor trains under the global step count: today's launches
        loss = torch.empty(1, dtype=F32, device=self._device)
        dout = torch.empty(n0 if self.head == "regression" else (n0, self.num_classes), dtype=F32, device=self._device)
        # the regression head's broadcast MSE is evaluated by the fused MLP launch itself where that launch exists (<= 16 rows)
        fused_loss = (labels, loss, dout) if (self.stat_sync is None and self._mlp_fused(n0)) else None
        # the dropout draw counter advances with the step's other counters, in the one launch at the end
        out, ctx = self.forward_device(audio, visual, save=True, fused_loss=fused_loss, caller_ticks=True,
                                       fused_loss_kind=None if loss_kind == "mse_bcast" else (loss_kind, loss_param, weights))
        n = out.shape[0]
        if ema_on:
            self._ensure_ema()                            # the first step: the average starts from the weights BEFORE any update
        if ctx["loss_done"]:
            pass
        elif loss_kind != "mse_bcast":
            ops.frame_loss(out, labels, loss, dout, loss_kind, loss_param, weights)
        elif self.head == "classifier":
            if self.stat_sync is not None:
                raise GoalnetError("global-batch mode is defined for the regression head's broadcast MSE only")
            ops.cross_entropy(out, labels, loss, dout)          # main.py:69, 189: CrossEntropyLoss(pred, (labels-1).long())
        elif self.stat_sync is not None:
            # the (N, N) broadcast couples every prediction with every label of the batch: evaluate it on the rank-ordered
            # concatenation and keep this rank's slice of dL/dp
            gout = torch.empty(n * self.stat_sync.world, dtype=F32, device=self._device)
            ops.mse_bcast(self.stat_sync.gather(out), self.stat_sync.gather(labels), loss, gout)
            dout = gout[n * self.stat_sync.rank: n * (self.stat_sync.rank + 1)]
        else:
            ops.mse_bcast(out, labels, loss, dout)
        sync = self.grad_sync
        self.last_ctx = ctx if self.keep_ctx else None
        lscale = self._loss_scale_for(n)
        self._arena_grad_scale = lscale
        if lscale != 1.0:
            ops.scale_(dout.view(-1), lscale)               # fp16: every activation gradient downstream carries this factor
        # One GPU, no gradient exchange, no overflow guard to consult: linear5.weight (99.8 % of the parameters at 224 x 224) gets
        # its Adam pass the moment its gradient exists and its last reader of the step (the data gradient) is enqueued — on the
        # side stream, i.e. 36 GB of HBM traffic under the MFMA-bound convolution gradients that follow instead of after them
        # (with frozen or re-thawed tensors the update is ONE launch over the trainable ranges after backward: no early pass)
        early = plain and sync is None and self.precision != "fp16" and self._large_overlap(n) and self._fork_ok(n)
        # The fp32 engine at large sizes runs serial (no fork), so that pass would be fully exposed: there the update of linear5.weight
        # runs in the epilogue of its weight-gradient GEMM instead (ops.linear_bwd_dw_adam, same bits), after the data gradient. The
        # gradient slot of visbl.linear5.weight in the arena is then NOT written: grad_of() of that tensor holds what an earlier,
        # unfused backward left there. keep_ctx = True (a step kept for inspection) or epi_fuse = False keep the gradient.
        fuse5 = epi_fuse_dw_adam(n, plain=plain, synced=sync is not None, precision=self.precision,
                                 train_w5="visbl.linear5.weight" not in frozen, shadowed=self._w5b is not None, inspected=self.keep_ctx,
                                 forced=self.epi_fuse, pieces=epi_fuse_pieces(os.environ.get("GOALNET_F32_EPI_FUSE")))
        if opt_on or k > 1:
            # both shortcuts hard-code plain Adam on this step's own gradient; clipping needs the whole norm first, and a window
            # updates from the accumulated gradient, on its last micro-step only
            fuse5 = False
        early = early and not fuse5 and not opt_on and k == 1
        # (small steps: the same update as a background pass on a third stream was measured slower at every width)
        done_early = []

        def early_adam(fork):
            s5 = self.spec("visbl.linear5.weight")
            lo, hi = s5.offset, s5.offset + s5.numel

            def piece():
                self._adam_state()                   # the first step allocates the moments
                self._adam_piece(lo, hi, lo, lr, betas, eps, 1.0 / lscale)
            fork.run(piece)
            done_early.append((lo, hi))

        def dw_adam(dz5, p3f, scale, shift):
            s5 = self.spec("visbl.linear5.weight")
            lo, hi = s5.offset, s5.offset + s5.numel
            self._adam_state()                       # the first step allocates the moments
            ops.linear_bwd_dw_adam(dz5, p3f, self._arena[lo:hi], self._adam_m[lo:hi], self._adam_v[lo:hi], lr, betas[0], betas[1], eps,
                                   self._state[0], scale=scale, shift=shift, bnC=512, grad_scale=1.0 / lscale, step_bias=1)
            done_early.append((lo, hi))
            self.epi_fused_dw += 1
        self.backward_device(ctx, dout, on_bucket=(lambda k: sync.on_bucket(self, k)) if sync is not None else None,
                             after_linear5=early_adam if early else None, frozen=frozen, fused_w5=dw_adam if fuse5 else None)
        scale = 1.0
        if sync is not None:
            scale = sync.finish(self)
        guard = None
        if self.precision == "fp16":
            # an overflow anywhere in the 16-bit chain reaches the gradients computed last (conv1 ... bnorm3) and first (the
            # fusion MLP sees nothing 16-bit): checking the two small buckets (after the exchange: all ranks agree) is enough
            s5 = self.spec("visbl.linear5.weight")
            if not frozen:
                after = min(s.offset for s in self._specs if s.offset > s5.offset)
                ops.grad_finite_check(self._garena[after:], self._state[0], self._guard[0], self._guard[1])
            else:
                # A pruned backward writes only the trainable slots: read those alone, never a frozen slot or slot padding. Every
                # trainable tensor is checked except linear5.weight (the big one): an overflow of the forward reaches all of them
                # through dL/dpred, one of the 16-bit backward chain reaches what is computed beneath it. Where nothing trains beneath
                # linear5.weight, its own gradient is the only reader of the 16-bit dz5 and is checked too.
                names = [s.name for s in self._specs if s.name not in frozen]
                if any(k.startswith(("visbl.bnorm", "visbl.conv")) for k in names):
                    names = [k for k in names if k != s5.name]
                for lo, hi in self._exact_runs(names):
                    ops.grad_finite_check(self._garena[lo:hi], self._state[0], self._guard[0], self._guard[1])
            guard = self._guard[0]
        # (the early Adam ran on the side stream: backward_device's last act joins it into this stream, so the average, issued by
        # adam_step behind its own launches, reads every updated weight)
        d0 = 1                                            # what the step counter state[0] advances by
        if k == 1:
            self.adam_step(lr, betas, eps, scale / lscale, _tick=False, _guard=guard, _done=done_early, optim=optim if opt_on else None, ema=ema)
        else:
            # a micro-step of a window: gradient / k into the accumulator behind the backward (no exchange and no loss scale here: both
            # are refused above), and on the window's last micro-step the update from the accumulator
            first, last = self._accum_done == 0, self._accum_done == k - 1
            ranges = trainable_ranges(self._specs, frozen, {})
            if len(ranges) > ops.ADAM_RANGES_MAX:
                raise GoalnetError(f"{len(ranges)} trainable ranges: the accumulation pass takes {ops.ADAM_RANGES_MAX}")
            if self._gacc is None:
                self._gacc = torch.zeros(self._arena_numel, dtype=F32, device=self._device)
            if ranges:
                ops.grad_accum_dev_ranges(self._gacc, self._garena, ranges, 1.0 / k, first)
            self._norm_of_acc = True
            if last:
                self.adam_step(lr, betas, eps, 1.0, _tick=False, optim=optim if opt_on else None, ema=ema, _grads=self._gacc)
            else:
                d0 = 0
            self._accum_advance(k, frozen)
        if _scatter is not None:
            ops.rows_scatter_tick(_scatter(loss, out), self._state, d0, ctx["drop_ticks"], _loop_tick[0], _loop_tick[1], bad_step=guard)
        elif guard is not None:
            # a step whose Adam was skipped is not counted (torch's GradScaler does not count it either): the retry runs under
            # the same step count; `_adam_t` on the host counts ATTEMPTED steps
            ops.counters_add4_guarded(self._state, 1, ctx["drop_ticks"], _loop_tick[0], _loop_tick[1], guard)
        else:
            ops.counters_add4(self._state, d0, ctx["drop_ticks"], _loop_tick[0], _loop_tick[1])
        return loss, out

    # ------------------------------------------------------------------------------------------
    # gradient accumulation
    # ------------------------------------------------------------------------------------------
    @property
    def accum_position(self):
        """(micro-steps of the current window done so far, the window's k); (0, k) between windows"""
        return self._accum_done, self._accum_k

    def _check_accumulate(self, k):
        """train_step(accumulate=k)'s refusals, all before anything is launched or allocated"""
        if self._accum_done:
            if k != self._accum_k:
                raise GoalnetError(f"accumulate changed from {self._accum_k} to {k} after {self._accum_done} micro-step(s) of a window: "
                                   "k may not change inside a window")
            if self._frozen_names() != self._accum_frozen:
                raise GoalnetError("the set of frozen tensors changed inside an accumulation window: the accumulator holds the "
                                   "gradients of the set the window started under")
        if k == 1:
            return
        if self.precision == "fp16":
            raise GoalnetError("accumulate > 1 with precision='fp16' is not built: the overflow guard's skipped steps and the loss scale "
                               "would have to act on a whole window (DESIGN.md §4.16)")
        if self.grad_sync is not None or self.stat_sync is not None:
            raise GoalnetError("accumulate > 1 with a grad_sync / stat_sync attached is not built: the exchange would have to be "
                               "skipped on a window's non-final micro-steps (DESIGN.md §4.16)")

    def _accum_advance(self, k, frozen):
        """the host's view of one micro-step of a window of k (train_step, and loop.VideoTrainer after a replay)"""
        self._accum_k, self._accum_frozen = k, frozenset(frozen)
        self._accum_done = (self._accum_done + 1) % k
        self._norm_of_acc = True

    def _refuse_mid_window(self, what):
        if self._accum_done:
            raise GoalnetError(f"{what} after {self._accum_done} of {self._accum_k} micro-steps of an accumulation window: "
                               "finish the window first")

    def accum_of(self, name) -> Optional[torch.Tensor]:
        """The accumulated gradient of a parameter — sum over the window's micro-steps so far of gradient / k — as a view with the
        reference's logical shape, like grad_of (which keeps showing the last micro-step's own gradient); None for a tensor that is
        frozen in this window."""
        if self._gacc is None:
            raise GoalnetError("no accumulated gradient yet: pass accumulate=k > 1 to train_step / VideoTrainer first")
        if self._accum_frozen is not None and name in self._accum_frozen:
            return None
        s = self.spec(name)
        v = self._view(self._gacc, s)
        return v.reshape(s.shape[0], -1) if s.kind == "lin5" else v

    def _adam_segments(self):
        """[(lo, hi)] arena ranges this rank's optimizer owns: everything, or — ddp.GradSync(shard_linear5=True) — everything
        but the foreign slices of visbl.linear5.weight"""
        sync = self.grad_sync
        if sync is None or not sync.sharded(self):
            return [(0, self._arena_numel)]
        s5 = self.spec("visbl.linear5.weight")
        after = min(s.offset for s in self._specs if s.offset > s5.offset)
        slo, shi = sync.shard_range(self)
        return [(0, s5.offset), (slo, shi), (after, self._arena_numel)]

    def _loss_scale_for(self, n: int) -> float:
        if self._loss_scale is not None:
            return float(self._loss_scale) / (1 << self._loss_scale_backoff) if self._loss_scale_backoff else float(self._loss_scale)
        return float(2.0 ** (10 + max(0, math.ceil(math.log2(max(n, 1)))) - self._loss_scale_backoff))

    def overflow_skipped_steps(self) -> int:
        """precision="fp16": optimizer steps skipped so far because a gradient overflowed (one host read-back)"""
        return 0 if self._guard is None else int(self._guard[1].item())

    def update_loss_scale(self) -> bool:
        """precision="fp16": the loss scale is static inside a step (a captured graph bakes it in), so a persistent overflow
        would skip every step silently. Call this where the host synchronises anyway (loop.VideoTrainer does, at its per-video
        read-back): when steps were skipped since the last call the scale is halved (True is returned; graphs keyed on the old
        scale are not replayed again). Skipped steps are not counted as optimizer steps (goalnet_counters_add4_guarded)."""
        k = self.overflow_skipped_steps()
        if k > self._skipped_seen:
            self._skipped_seen = k
            self._loss_scale_backoff += 1
            return True
        return False

    def _adam_state(self):
        segs = self._adam_segments()
        if self._adam_m is not None and self._adam_segs != segs:
            raise GoalnetError("the optimizer state was laid out for another sharding of linear5.weight; attach / detach "
                               "ddp.GradSync(shard_linear5=True) before the first optimizer step, not between steps")
        if self._adam_m is None:
            total = sum(hi - lo for lo, hi in segs)
            self._adam_m = torch.zeros(total, dtype=F32, device=self._device)
            self._adam_v = torch.zeros(total, dtype=F32, device=self._device)
            self._adam_segs = segs
        return segs

    def _adam_piece(self, lo, hi, moff, lr, betas, eps, grad_scale, guard=None, grads=None):
        """the fused Adam on arena[lo:hi] against the moments at [moff, moff + hi - lo) (moff = lo unless the optimizer state is sharded).
        Refreshes the part of the valid 16-bit copy of linear5.weight that lies inside, in the same pass (the kernels do not bump
        versions). `guard` (fp16): the pass is skipped as a whole when this step's gradients overflowed (goalnet_grad_finite_check).
        The step counter is NOT advanced."""
        s5 = self.spec("visbl.linear5.weight")
        p, g = self._arena[lo:hi], (self._garena if grads is None else grads)[lo:hi]      # grads: the accumulator
        m, v = self._adam_m[moff:moff + hi - lo], self._adam_v[moff:moff + hi - lo]
        a, b = max(lo, s5.offset), min(hi, s5.offset + s5.numel)       # the part of linear5.weight inside this piece
        sh = None
        if self._w5b is not None and self._w5b_version == self._w5_version() and a < b:
            sh = self._w5b[a - s5.offset:b - s5.offset]
        if guard is not None:
            ops.adam_step_dev_guarded(p, g, m, v, lr, betas[0], betas[1], eps, self._state[0], guard, shadow=sh,
                                      shadow_begin=(a - lo) if sh is not None else 0, grad_scale=grad_scale, step_bias=1)
        elif sh is not None:
            ops.adam_step_dev_shadow(p, g, m, v, lr, betas[0], betas[1], eps, self._state[0], sh, a - lo, grad_scale, step_bias=1)
        else:
            ops.adam_step_dev(p, g, m, v, lr, betas[0], betas[1], eps, self._state[0], grad_scale, step_bias=1)

    def adam_step(self, lr=1e-3, betas=(0.9, 0.999), eps=1e-8, grad_scale=1.0, _tick=True, _guard=None, _done=(), optim=None, ema=None,
                  _grads=None):
        """torch.optim.Adam defaults over the whole arena in one launch (main.py:70, 193). The step count is the device
        counter state[0] (= completed steps) + 1, so the same captured launch serves every step. With a sharded
        linear5.weight (ddp.py) the pass covers this rank's slice only — three launches — and the optimizer state exists
        only for what the rank owns. `optim` (optim.OptimOptions): non-trivial options run _optim_step instead.
        `ema` (optim.EmaOptions): behind the update, and in front of the launch that advances the step counter, one
        launch folds the updated weights into the average (_ema_update). `_grads`: the arena the update reads in place of the gradient
        arena (train_step's accumulator on a window's last micro-step)."""
        opt_on = optim_step_path(optim, sharded=bool(getattr(self.grad_sync, "shard_linear5", False)))
        ema_on = ema_step_path(ema, sharded=bool(getattr(self.grad_sync, "shard_linear5", False)))
        self._refuse_averaged("adam_step")
        if ema_on:
            self._ensure_ema()                            # the first step: the average starts from the weights BEFORE the update
        frozen = self._bwd_frozen
        self._check_freeze(frozen)
        if self.precision == "fp16":
            # a guard-skipped step is not counted on the device, so the host cannot keep the counts of sat-out steps without a read-back
            if self._fp16_frozen is None:
                self._fp16_frozen = frozen
            elif self._fp16_frozen != frozen:
                raise GoalnetError("precision='fp16': the set of frozen tensors may not change after the first optimizer step")
        if opt_on:
            assert not _done
            return self._optim_step(lr, betas, eps, grad_scale, optim, frozen, _tick, _guard, ema if ema_on else None, _grads)
        segs = self._adam_state()
        self._adam_t += 1
        if not self._plain_step(frozen):
            # frozen tensors (or tensors that sat steps out and train again): ONE launch over the trainable ranges, each under its own
            # step count; the optimizer state keeps the arena's layout, so nothing moves when a tensor is unfrozen
            assert segs == [(0, self._arena_numel)] and not _done
            ranges = trainable_ranges(self._specs, frozen, self._sat_out)
            if len(ranges) > ops.ADAM_RANGES_MAX:
                raise GoalnetError(f"{len(ranges)} trainable ranges: the fused Adam takes {ops.ADAM_RANGES_MAX}")
            s5 = self.spec("visbl.linear5.weight")
            shadow = self._w5b if (s5.name not in frozen and self._w5b is not None and self._w5b_version == self._w5_version()) else None
            if ranges:
                ops.adam_step_dev_ranges(self._arena, self._garena if _grads is None else _grads, self._adam_m, self._adam_v, ranges, lr,
                                         betas[0], betas[1], eps, self._state[0], grad_scale, shadow=shadow, shadow_begin=s5.offset,
                                         bad_step=_guard)
            self._count_sat_out(frozen)
            if ema_on:
                self._ema_update(ema, frozen, _guard)
            if _tick:
                ops.counter_add(self._state[0], 1)
            return
        pieces, off, cur = [], 0, 0                 # (lo, hi, offset of the moments)
        if _done:
            # ranges train_step already updated under backward (the early Adam on linear5.weight): the rest of the arena now
            assert segs == [(0, self._arena_numel)] and _guard is None
            for lo, hi in sorted(_done) + [(self._arena_numel, self._arena_numel)]:
                if cur < lo:
                    pieces.append((cur, lo, cur))
                cur = hi
        else:
            for lo, hi in segs:
                pieces.append((lo, hi, off))
                off += hi - lo
        for lo, hi, moff in pieces:
            self._adam_piece(lo, hi, moff, lr, betas, eps, grad_scale, _guard, _grads)
        if len(segs) > 1:
            shadow_ok = self._w5b is not None and self._w5b_version == self._w5_version()
            self.grad_sync.after_adam(self, self._w5b if shadow_ok else None)
        if ema_on:
            self._ema_update(ema, frozen, _guard)
        if _tick:
            ops.counter_add(self._state[0], 1)

    def _optim_step(self, lr, betas, eps, grad_scale, optim, frozen, _tick, _guard, ema=None, grads=None):
        """adam_step under non-trivial options: the squared norm of the trainable gradients (clipping only; after the gradient exchange,
        so grad_scale carries 1 / world) and ONE launch over the trainable ranges, split where the decay flag changes. The learning
        rate is the schedule's at the device step counter; 16-bit copy and fp16 guard pass through as in _adam_piece. With parameter
        groups or AMSGrad the ranges are group_ranges() — split where the group changes too — and the one launch is
        ops.group_step_dev_ranges over its table of hyper-parameters, with the vmax arena where a group runs under AMSGrad."""
        grouped = bool(optim.groups or optim.amsgrad)     # the launch over a table of hyper-parameters
        if grouped:
            ranges, table = group_ranges(self._specs, frozen, self._sat_out, optim, lr, betas, eps)
        else:
            ranges = optim_ranges(self._specs, frozen, self._sat_out, optim)
        if len(ranges) > ops.ADAM_RANGES_MAX:
            raise GoalnetError(f"{len(ranges)} trainable ranges (split by weight decay): the fused step takes {ops.ADAM_RANGES_MAX}")
        segs = self._adam_state()
        assert segs == [(0, self._arena_numel)]
        self._adam_t += 1
        s5 = self.spec("visbl.linear5.weight")
        shadow = self._w5b if (s5.name not in frozen and self._w5b is not None and self._w5b_version == self._w5_version()) else None
        g = self._garena if grads is None else grads
        if ranges and grouped:
            sumsq = ops.grad_sumsq(g, [r[:4] for r in ranges]) if optim.max_grad_norm is not None else None
            vmax = self._ensure_vmax() if any(table[r[4]][5] for r in ranges) else None
            ops.group_step_dev_ranges(self._arena, g, self._adam_m, self._adam_v, vmax, ranges, table, optim, self._state[0], grad_scale,
                                      sumsq=sumsq, shadow=shadow, shadow_begin=s5.offset, bad_step=_guard)
        elif ranges:
            sumsq = ops.grad_sumsq(g, ranges) if optim.max_grad_norm is not None else None
            ops.optim_step_dev_ranges(self._arena, g, self._adam_m, self._adam_v, ranges, lr, betas[0], betas[1], eps, optim,
                                      self._state[0], grad_scale, sumsq=sumsq, shadow=shadow, shadow_begin=s5.offset, bad_step=_guard)
        self._count_sat_out(frozen)
        if ema is not None:
            self._ema_update(ema, frozen, _guard)
        if _tick:
            ops.counter_add(self._state[0], 1)

    # ------------------------------------------------------------------------------------------
    # AMSGrad's fourth state arena
    # ------------------------------------------------------------------------------------------
    def _ensure_vmax(self):
        """the running maximum of v: whole-arena and zero-filled like _adam_v, allocated by the first AMSGrad step and kept in place
        thereafter — captured graphs hold its address"""
        if self._adam_vmax is None:
            self._adam_vmax = torch.zeros_like(self._adam_v)
        return self._adam_vmax

    def vmax_of(self, name) -> torch.Tensor:
        """AMSGrad's running maximum of exp_avg_sq (torch's max_exp_avg_sq) of a parameter as a view with the reference's logical
        shape, like ema_of; zero for tensors that never ran under AMSGrad."""
        if self._adam_vmax is None:
            raise GoalnetError("no AMSGrad state yet: step with optim.OptimOptions(amsgrad=True) or a ParamGroup(amsgrad=True) first")
        s = self.spec(name)
        v = self._view(self._adam_vmax, s)
        return v.reshape(s.shape[0], -1) if s.kind == "lin5" else v

    # ------------------------------------------------------------------------------------------
    # the weight average
    # ------------------------------------------------------------------------------------------
    def _ensure_ema(self):
        """the average's arena: allocated on first use — in front of that step's first update — as a copy of the WHOLE parameter
        arena, slot padding included, so frozen tensors' averages equal their weights from the start"""
        if self._ema is None:
            self._ema = self._arena.clone()
        return self._ema

    def _ema_update(self, ema, frozen, guard):
        """ONE launch over the trainable ranges (frozen tensors are not in them: their average stays equal to the weight, which does not
        move), issued on the current stream behind every update of this optimizer step and in front of the launch that advances the
        step counter: t = *step + 1 is the step that has just been applied. `guard` (fp16): a step whose Adam was skipped leaves the
        average alone."""
        ranges = trainable_ranges(self._specs, frozen, {})
        if not ranges:
            return
        if len(ranges) > ops.ADAM_RANGES_MAX:
            raise GoalnetError(f"{len(ranges)} trainable ranges: the weight average takes {ops.ADAM_RANGES_MAX}")
        ops.ema_update_dev_ranges(self._arena, self._ensure_ema(), ranges, ema, self._state[0], step_bias=1, bad_step=guard)

    def _refuse_averaged(self, what):
        if self._averaged:
            raise GoalnetError(f"{what} inside `with model.averaged()`: the arena holds the averaged weights there, and an update "
                               "would train the average; leave the block first")

    def ema_of(self, name) -> torch.Tensor:
        """The average of a parameter as a view with the reference's logical shape, like param_of (inside `with model.averaged()`
        the two are exchanged: ema_of then shows the live weights)."""
        if self._ema is None:
            raise GoalnetError("no weight average yet: pass ema=EmaOptions(...) to train_step / adam_step / VideoTrainer first")
        s = self.spec(name)
        v = self._view(self._ema, s)
        return v.reshape(s.shape[0], -1) if s.kind == "lin5" else v

    @contextlib.contextmanager
    def averaged(self):
        """`with model.averaged(): ...` — the parameter arena and the average are exchanged over the whole arena (ops.swap_ranges, one
        launch) on entry and again on exit, which restores both bit for bit. Inside, forward, eval_video, VideoSummarizer and
        state_dict() see the averaged weights, so `torch.save(model.state_dict())` there is a checkpoint of the average that the
        reference's utils.AVM loads. The BatchNorm running buffers are the LIVE ones: they are not averaged (a train-mode forward
        inside the block moves them as it does outside). Cached operands keyed on the weights' version (the 16-bit copy of
        linear5.weight) are re-made on both sides. A swap and not a pointer exchange: the nn.Parameter views and captured graphs hold
        the arena's address. train_step, adam_step, a parameter backward and load_state_dict inside the block raise GoalnetError, as
        does a nested entry."""
        if self._averaged:
            raise GoalnetError("model.averaged() is already active: the block does not nest")
        self._refuse_mid_window("model.averaged()")
        if self._ema is None:
            raise GoalnetError("no weight average yet: pass ema=EmaOptions(...) to train_step / adam_step / VideoTrainer first")
        if self.grad_sync is not None and getattr(self.grad_sync, "shard_linear5", False):
            raise GoalnetError("model.averaged() is not built for ddp.GradSync(shard_linear5=True)")
        whole = [(0, self._arena_numel)]
        ops.swap_ranges(self._arena, self._ema, whole)
        self._load_count += 1
        self._averaged = True
        try:
            yield self
        finally:
            ops.swap_ranges(self._arena, self._ema, whole)
            self._load_count += 1
            self._averaged = False

    # ------------------------------------------------------------------------------------------
    # exact save / resume
    # ------------------------------------------------------------------------------------------
    def _identity(self):
        return {"audio_included": bool(self.audio_included), "head": self.head, "num_classes": int(self.num_classes),
                "precision": self.precision, "hw3": self._hw3, "l2": self._l2}

    def _refuse_sharded_state(self, what):
        if self.grad_sync is not None and getattr(self.grad_sync, "shard_linear5", False):
            raise GoalnetError(f"{what} under ddp.GradSync(shard_linear5=True): saving a sharded optimizer state is not built")

    def training_state(self) -> dict:
        """Everything a run needs to continue as if it had not stopped, as CPU tensors and plain Python values (`torch.save` takes
        it): "model" = state_dict() — the reference's keys and layouts, so the file doubles as a reference checkpoint —, the Adam
        moments (with AMSGrad's "adam_vmax", None before its first step) and the weight average as flat arenas in the arena's own layout, the four device counters and the two fp16 guard
        words, the host mirrors of the step and dropout counts, dropout seed and mode, the per-tensor counts of sat-out steps and the
        frozen set the fp16 path pinned, the loss-scale fields, and what identifies the model (load_training_state checks it). One
        host synchronisation."""
        self._refuse_sharded_state("training_state()")
        self._refuse_averaged("training_state()")
        self._refuse_mid_window("training_state()")
        if not self._materialized:
            raise RuntimeError("training_state() before the first forward / load_state_dict(): parameters are uninitialised")
        if self._state is None:
            self._make_state()

        def cpu(t):
            return None if t is None else t.detach().cpu().clone()
        return {
            "format": STATE_FORMAT,
            **self._identity(),
            "model": self.state_dict(),
            "arena_numel": int(self._arena_numel),
            "adam_m": cpu(self._adam_m), "adam_v": cpu(self._adam_v), "adam_vmax": cpu(self._adam_vmax), "ema": cpu(self._ema),
            "counters": cpu(self._state), "guard": cpu(self._guard),
            "adam_t": int(self._adam_t), "drop_step": int(self._drop_step),
            "dropout_seed": int(self.dropout_seed), "dropout_mode": self.dropout_mode,
            "sat_out": {k: int(v) for k, v in self._sat_out.items()},
            "bwd_frozen": sorted(self._bwd_frozen),
            "fp16_frozen": None if self._fp16_frozen is None else sorted(self._fp16_frozen),
            "loss_scale": self._loss_scale, "loss_scale_user": bool(self._loss_scale_user),
            "loss_scale_backoff": int(self._loss_scale_backoff), "skipped_seen": int(self._skipped_seen),
        }

    def load_training_state(self, state: dict):
        """Restore training_state(): the identity fields must match this model (RuntimeError names the first that does not), the model
        is materialised if needed, and weights, BatchNorm buffers, moments, average, counters, guard words, dropout stream, sat-out
        counts and loss-scale fields are put back — in place where the tensors exist, since captured graphs hold their addresses.
        dropout_mode "given" is not restored (its masks are not part of the state): the model's own mode stays."""
        self._refuse_sharded_state("load_training_state()")
        self._refuse_averaged("load_training_state()")
        self._refuse_mid_window("load_training_state()")
        if not isinstance(state, dict) or state.get("format") != STATE_FORMAT:
            raise RuntimeError(f"load_training_state: not a training state of format {STATE_FORMAT}")
        mine = self._identity()
        for k in ("audio_included", "head", "num_classes", "precision"):
            if state[k] != mine[k]:
                raise RuntimeError(f"load_training_state: the state was saved from a model with {k}={state[k]!r}, this one has {k}={mine[k]!r}")
        for k in ("hw3", "l2"):
            if self._materialized and state[k] != mine[k]:
                raise RuntimeError(f"load_training_state: the state was saved from a model with {k}={state[k]!r}, this one has {k}={mine[k]!r}")
        self.load_state_dict(state["model"])                            # materialises; bumps _load_count
        if state["arena_numel"] != self._arena_numel:
            raise RuntimeError(f"load_training_state: arena of {state['arena_numel']} elements, this model's has {self._arena_numel}")
        if state["adam_m"] is not None:
            if self._adam_m is None:
                self._adam_state()                                      # lays the moments out
            if self._adam_m.numel() != state["adam_m"].numel():
                raise RuntimeError("load_training_state: the optimizer state was laid out for another sharding")
            self._adam_m.copy_(state["adam_m"])
            self._adam_v.copy_(state["adam_v"])
        elif self._adam_m is not None:
            self._adam_m.zero_()
            self._adam_v.zero_()
        vmax = state.get("adam_vmax")                                   # a state from before AMSGrad has no such key: no AMSGrad state yet
        if vmax is not None:
            if self._adam_m is None or vmax.numel() != self._adam_v.numel():
                raise RuntimeError("load_training_state: AMSGrad's arena does not match the moments'")
            self._ensure_vmax().copy_(vmax)
        elif self._adam_vmax is not None:
            self._adam_vmax.zero_()
        if state["ema"] is not None:
            self._ensure_ema().copy_(state["ema"])
        if self._state is None:
            self._make_state()
        self._state.copy_(state["counters"])
        self._guard.copy_(state["guard"])
        self._adam_t, self._drop_step = int(state["adam_t"]), int(state["drop_step"])
        self.dropout_seed = int(state["dropout_seed"])
        if state["dropout_mode"] != "given" and self.dropout_mode != "given":
            self.dropout_mode = state["dropout_mode"]
        self._sat_out = {k: int(v) for k, v in state["sat_out"].items()}
        self._bwd_frozen = frozenset(state["bwd_frozen"])
        self._fp16_frozen = None if state["fp16_frozen"] is None else frozenset(state["fp16_frozen"])
        self._loss_scale, self._loss_scale_user = state["loss_scale"], bool(state["loss_scale_user"])
        self._loss_scale_backoff, self._skipped_seen = int(state["loss_scale_backoff"]), int(state["skipped_seen"])
        self._load_count += 1

    def grad_norm(self) -> torch.Tensor:
        """(1,) float64 on the device, no sync: the L2 norm of the gradients of the tensors that trained in the last backward, as the
        gradient arena holds them (ops.grad_sumsq over the trainable ranges), divided by the loss scale an fp16 train_step left in
        the arena. What max_grad_norm is compared with. After a step that updated linear5.weight in its weight-gradient epilogue
        (train_step's docstring) that tensor's slot holds an earlier backward's gradient. After a train_step(accumulate=k > 1) it is the
        norm of the ACCUMULATED gradient (accum_of), which is what that window's clipping compares."""
        if self._garena is None:
            raise RuntimeError("grad_norm() before any backward: there are no gradients")
        ranges = [(b, c, k, False) for b, c, k in trainable_ranges(self._specs, self._bwd_frozen, self._sat_out)]
        if not ranges:
            return torch.zeros(1, dtype=torch.float64, device=self._device)
        if len(ranges) > ops.ADAM_RANGES_MAX:
            raise GoalnetError(f"{len(ranges)} trainable ranges: one launch takes {ops.ADAM_RANGES_MAX}")
        norm = ops.grad_sumsq(self._gacc if self._norm_of_acc else self._garena, ranges).sqrt_()
        return norm / self._arena_grad_scale if self._arena_grad_scale != 1.0 else norm

    def current_lr(self, lr=1e-3, optim=None, group=None) -> float:
        """the learning rate the next optimizer step runs at under `optim` (optim.OptimOptions; None: `lr`), evaluated by the device from
        its step counter (ops.optim_lr). `group`: the rate of that row of optim.hyper_table() — 0 the default group, i + 1
        optim.groups[i] (ops.group_lr). One read-back."""
        if group is not None and (optim is None or isinstance(group, bool) or not isinstance(group, int) or not 0 <= group <= len(optim.groups)):
            raise ValueError(f"group must be an index into the default group and optim.groups, got {group!r}")
        if optim is None:
            return float(lr)
        self._require_device()
        if self._state is None:
            self._make_state()
        if group is not None:
            return float(ops.group_lr(optim.hyper_table(lr, (0.9, 0.999), 1e-8), group, optim, self._state[0]).item())
        return float(ops.optim_lr(lr, optim, self._state[0]).item())

    def make_optimizer(self, lr=1e-3, betas=(0.9, 0.999), eps=1e-8):
        """`optim.Adam(model.parameters(), lr)` (main.py:70) as one fused pass over the arena: cvml_goalnet_amd.optim.Adam"""
        from .optim import Adam
        return Adam(self.parameters(), lr=lr, betas=betas, eps=eps, model=self)

    def predict_classes(self, scores: torch.Tensor) -> torch.Tensor:
        """head="classifier": `torch.argmax(predictions, axis = 1) + 1` (main.py:97, 190) on the device; (N,) float classes 1..C"""
        s = scores.detach().to(device=self._device, dtype=F32).contiguous()
        return ops.argmax_plus1(s, torch.empty(s.shape[0], dtype=F32, device=self._device))

    def grad_of(self, name) -> Optional[torch.Tensor]:
        """Gradient of a parameter as a strided view with the reference's logical shape (linear5: (512, C*HW) copy); None for a
        tensor that was frozen (requires_grad=False) in the last backward."""
        s = self.spec(name)
        if name in self._bwd_frozen:
            return None                       # frozen in the last backward: no gradient was produced
        v = self._view(self._garena, s)
        v = v.reshape(s.shape[0], -1) if s.kind == "lin5" else v
        # fp16: train_step leaves loss_scale x gradient in the arena (the fused Adam divides it out); the drop-in path unscales
        return v / self._arena_grad_scale if self._arena_grad_scale != 1.0 else v

    def param_of(self, name) -> torch.Tensor:
        s = self.spec(name)
        v = self._view(self._arena, s)
        return v.reshape(s.shape[0], -1) if s.kind == "lin5" else v


class _AVMFunction(torch.autograd.Function):
    """Couples the HIP forward/backward to autograd so `loss.backward()` fills `.grad` of ordinary
    nn.Parameters (SURVEY.md §8(b) "Train step" (i)). Gradients are strided views of the gradient arena."""

    @staticmethod
    def forward(ctx, model, aud, vis, src_dev, aud_in, vis_in, *params):
        out, saved = model.forward_device(aud, vis, save=True)
        ctx.model, ctx.saved, ctx.src_dev = model, saved, src_dev
        ctx.inputs_like = (aud_in, vis_in)
        return out.view(-1, model.num_classes).to(src_dev)

    @staticmethod
    def backward(ctx, gout):
        model, saved = ctx.model, ctx.saved
        # a previous backward's .grad may alias the arena we are about to overwrite (no zero_grad in between)
        for s in model._specs:
            prm = getattr(*model._module_of(s.name))
            if prm.grad is not None and model._garena is not None and \
                    prm.grad.untyped_storage().data_ptr() == model._garena.untyped_storage().data_ptr():
                prm.grad = prm.grad.clone()
        dout = gout.detach().to(device=model._device, dtype=F32).contiguous().view(-1)
        lscale = model._loss_scale_for(saved["n"])
        if lscale != 1.0:                                 # fp16: scaled through the 16-bit chain, unscaled before torch sees .grad
            dout = ops.scale_(dout.clone(), lscale)
        need = (ctx.needs_input_grad[4], ctx.needs_input_grad[5])
        # a parameter with requires_grad=False gets no gradient: autograd says which (needs_input_grad), and backward returns None for it
        frozen = frozenset(s.name for s, k in zip(model._specs, ctx.needs_input_grad[6:]) if not k)
        din = model.backward_device(saved, dout, inputs=need if any(need) else None, frozen=frozen)
        if lscale != 1.0:
            ops.scale_(model._garena, 1.0 / lscale)
            for d in din:
                if d is not None:
                    ops.scale_(d.view(-1), 1.0 / lscale)
        model._arena_grad_scale = 1.0
        ctx.saved = None
        grads = [None if s.name in frozen else model._view(model._garena, s) for s in model._specs]
        # the inputs' gradients in the inputs' own shape, type and device (CPU leaves: one D2H copy)
        din = [None if (d is None or not k) else d.view(like.shape).to(device=like.device, dtype=like.dtype)
               for d, k, like in zip(din, need, ctx.inputs_like)]
        ctx.inputs_like = None
        return (None, None, None, None, *din, *grads)
