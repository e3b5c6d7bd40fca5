"""Device-side version of the reference's per-video sub-batch training loop.

The reference trains one video at a time, ten frames per optimizer step, and synchronises the host twice per
step (`subbatch_loss.item()`, `subbatch_predictions.flatten().tolist()`), `/root/reference/main.py:169-198`:

    while subbatch_ceil != len(batch_frames):
        ... frames[a:b], audios[a:b], labels[a:b]                  # main.py:181-184
        optimizer.zero_grad(); pred = model(audios, frames)        # main.py:187-188
        loss = criterion(pred, labels); loss.backward(); optimizer.step()   # main.py:191-193
        batch_loss += loss.item(); batch_predictions += pred.flatten().tolist()   # main.py:195-196
    batch_loss = batch_loss / iterations                            # main.py:203

`VideoTrainer.train_video` is that loop with the video resident in HBM and ONE HIP-graph launch per sub-batch:
the graph gathers rows [cursor, cursor+n) of the video (one launch), runs forward + broadcast MSE + backward + fused
Adam (`AVM.train_step`, whose last launch advances all four counters) and scatters the predictions and the loss into
per-video device arrays (one launch).
Everything that changes between sub-batches (frame cursor, sub-batch index, Adam step count, dropout draw index)
is a device counter (csrc/stepstate.hip), so the same graph is replayed for every full sub-batch; a shorter last
sub-batch uses a second graph captured for its own size. The host reads results back once per video.

The first sub-batch of each size runs eagerly (it is a real step — it also allocates the optimizer state and the
cached operand buffers); the graph is captured at the second occurrence. Capturing executes nothing, so the
sequence of optimizer steps is exactly the reference's.

The learning rate is a launch argument, so a captured graph bakes in the `lr` it was captured with and the graph key does not carry
it: changing `trainer.lr` after a size's first capture has no effect on that size's replays. A rate that changes over the run is a
schedule: `optim=OptimOptions(schedule=..., warmup_steps=...)` is evaluated on the device from the step counter,
inside every replay, with `lr` as its base rate.

EXTENSION (off by default): `optim=OptimOptions(...)` — weight decay, gradient-norm clipping and learning-rate
schedules on every sub-batch's optimizer step (`AVM.train_step(optim=)`); the graph key carries `optim.signature()`.

EXTENSION (off by default): `ema=EmaOptions(...)` keeps an exponential moving average of the weights behind every
sub-batch's optimizer step (`AVM.train_step(ema=)`, one more launch inside the same graphs; the graph key carries `ema.signature()`).
`state_dict()` / `load_state_dict()` save and restore the run — the model's training state and the trainer's pass index — so that a
resumed run continues bit for bit.

EXTENSION (off by default): `accumulate=k` applies one optimizer step per window of k sub-batches
(`AVM.train_step(accumulate=)`): every sub-batch is a micro-step whose gradient / k is added into a second arena, and the window's last
one updates from it. Windows never span videos: a video's last window may be shorter (j < k sub-batches, run as a window of j) and is
applied at the end of the video (`accum_windows`). The graph key carries the phase (first?, last?, length).

EXTENSION (off by default): `shuffle=True` / `augment={...}` draw a plan per pass on the device — frame order, flip,
shift, contrast, brightness per frame — and the same graphs gather their sub-batches through it; predictions come back in frame order.

EXTENSION (off by default): `audio_augment={...}` / `mixup={...}` draw a second table beside that plan — per frame a
time shift, a time mask, a coefficient mask, a gain and a noise key for its audio row, and a mixup partner with its weight — and the
same graphs gather audio, frames, labels and loss weights through both. Under mixup a frame's prediction is the model's output on
the MIXED input; `eval_video` never augments.
"""
from __future__ import annotations

from typing import Dict, Tuple

import torch

from . import augment as _augment, ops, synth
from .avm import accum_count, accum_windows
from .optim import EmaOptions, OptimOptions

TRAINER_STATE_FORMAT = 1

F32 = torch.float32


def _plain(x):
    """tuples and lists compare alike (a saved state may have passed through a format that knows only lists)"""
    return [_plain(v) for v in x] if isinstance(x, (tuple, list)) else x


class VideoTrainer:
    def __init__(self, model, subbatch_size: int = 10, lr: float = 1e-3, betas=(0.9, 0.999), eps: float = 1e-8,
                 graphs: bool = True, loss: str = "mse_bcast", loss_param=None, shuffle: bool = False, augment=None,
                 seed: int = synth.BASE_SEED, optim=None, ema=None, accumulate: int = 1, audio_augment=None, mixup=None):
        if subbatch_size < 1:
            raise ValueError("subbatch_size must be >= 1")
        # EXTENSION: sub-batches per optimizer step. 1: train_step is called as before.
        self.accumulate = accum_count(accumulate)
        self._phase = (True, True, 1)               # (first?, last?, length) of the micro-step _sub_step is about to issue
        if optim is not None and not isinstance(optim, OptimOptions):
            raise ValueError("optim must be an optim.OptimOptions")
        # EXTENSION: optimizer options of every sub-batch's step. None / trivial: train_step is called as before.
        self.optim = None if (optim is None or optim.trivial) else optim
        self._optim_sig = () if self.optim is None else self.optim.signature()
        self._okw = {} if self.optim is None else {"optim": self.optim}
        # EXTENSION: the weight average every sub-batch's step is folded into. None: train_step is called as before.
        if ema is not None and not isinstance(ema, EmaOptions):
            raise ValueError("ema must be an optim.EmaOptions")
        self.ema = ema
        self._ema_sig = () if ema is None else ema.signature()
        if ema is not None:
            self._okw = dict(self._okw, ema=ema)
        # EXTENSION: a fresh frame order and fresh pixels per pass, drawn on the device into a plan table that the
        # captured graphs read. Off by default: with shuffle=False and no augmentation switched on, _sub_step is today's launches.
        self.augment = _augment.augment_options(augment)        # ValueError: unknown option, value out of range
        self.shuffle = bool(shuffle)
        self.seed = int(seed)
        self.passes = 0                                         # train_video calls so far = the pass index of the next plan
        self._colour = self.augment["contrast"] > 0 or self.augment["brightness"] > 0
        self._augments = self._colour or self.augment["flip_p"] > 0 or self.augment["max_shift"] > 0
        # EXTENSION: audio augmentation and mixup, drawn into a second table beside the plan. Absent, None or all
        # zero: nothing below changes what _sub_step launches.
        self.audio_augment = _augment.audio_augment_options(audio_augment)      # ValueError: unknown option, value out of range
        self.mixup = _augment.mixup_options(mixup)
        self._audio_aug = any(v > 0 for v in self.audio_augment.values())
        self._mix = self.mixup["strength"] > 0 and self.mixup["p"] > 0
        if self._audio_aug and not model.audio_included:
            raise ValueError("audio_augment needs a model with audio_included=True")
        if self._mix and model.head == "classifier":
            raise ValueError("mixup blends labels: it needs the regression head (class labels cannot be blended)")
        self._mix_sig = (tuple(self.audio_augment.items()), tuple(self.mixup.items())) if (self._audio_aug or self._mix) else ()
        self._planned = self.shuffle or self._augments or bool(self._mix_sig)      # sub-batches go through the plan
        ops.loss_spec(loss, loss_param, False, model.head)      # ValueError: unknown name, beta <= 0, the classifier head
        self.loss, self.loss_param = loss, loss_param           # AVM.train_step's loss; the default is the reference's
        self._weighted = False                                  # the video being trained on came with per-frame weights
        self.model = model
        self.subbatch_size = subbatch_size          # main.py:44
        self.lr, self.betas, self.eps = lr, betas, eps
        self.graphs = graphs
        self._graphs: Dict[tuple, torch.cuda.CUDAGraph] = {}        # (sub-batch size, loss scale, trainable ranges, loss, (shuffle, colour, augments), optim signature, ema signature, accumulation phase, (audio_augment, mixup) signatures, training) -> graph
        self._uses_w5b: Dict[tuple, bool] = {}      # that graph reads the bf16 copy of linear5.weight (precision="bf16", n > 16)
        self._shadows: Dict[tuple, bool] = {}       # that graph's fused Adam refreshes the copy (it was live at capture)
        self._seen = set()
        self._pool = None
        self._cap = 0                               # frames the staging tables hold
        self._key = None                            # (H, W, B): shapes the tables / graphs were built for
        self.replays = 0                            # statistics: graph launches vs eager steps
        self.eager_steps = 0

    # ---- staging tables: the whole video in HBM -----------------------------------------------------------------
    def _ensure_tables(self, n_frames: int, hw: Tuple[int, int], bins: int):
        m = self.model
        key = (hw, bins)
        if key == self._key and n_frames <= self._cap:
            return
        dev = m._device
        cap = max(n_frames, 2 * self._cap if key == self._key else 0, 64)
        self._graphs.clear()                        # pointers below are baked into captured graphs
        self._uses_w5b.clear()
        self._shadows.clear()
        self._pool = None
        self._key, self._cap = key, cap
        sb = self.subbatch_size
        self._vid = torch.empty(cap, 3, hw[0], hw[1], dtype=F32, device=dev)
        self._aud = torch.empty(cap, 30, bins, dtype=F32, device=dev) if m.audio_included else None
        self._lab = torch.empty(cap, dtype=F32, device=dev)
        # per-frame loss weights (train_video(weights=...)): only the pointwise losses take any
        self._wts = torch.empty(cap, dtype=F32, device=dev) if self.loss not in ("mse_bcast", "rank") else None
        self._pred = torch.empty(cap, dtype=F32, device=dev)
        self._loss = torch.empty((cap + sb - 1) // sb + 1, dtype=F32, device=dev)
        # the pass plan (augment.py): rewritten eagerly by every train_video, read by the graphs at this address
        self._plan = torch.zeros(cap, 8, dtype=torch.int32, device=dev) if self._planned else None
        # its second table, rewritten and read the same way
        self._plan2 = torch.zeros(cap, 12, dtype=torch.int32, device=dev) if self._mix_sig else None

    def _step_kw(self):
        """train_step's keyword arguments beyond the loss: optimizer options, weight average, and — inside a window of more than one
        micro-step — the window's length"""
        return self._okw if self._phase[2] == 1 else dict(self._okw, accumulate=self._phase[2])

    def _sub_step(self, n: int):
        """gather rows -> train_step -> scatter results -> advance the counters. Pure device work (capturable)."""
        m = self.model
        st = m._state
        dev = m._device
        hw, bins = self._key
        vis = torch.empty(n, 3, hw[0], hw[1], dtype=F32, device=dev)
        lab = torch.empty(n, dtype=F32, device=dev)
        if self._planned:
            return self._sub_step_planned(n, vis, lab)
        segs = [(self._vid, vis, n, st[2], 0, True), (self._lab, lab, n, st[2], 0, True)]
        aud = None
        if m.audio_included:
            aud = torch.empty(n, 30, bins, dtype=F32, device=dev)
            segs.append((self._aud, aud, n, st[2], 0, True))
        lkw = {}
        if self.loss != "mse_bcast":
            wts = None
            if self._weighted:
                wts = torch.empty(n, dtype=F32, device=dev)
                segs.append((self._wts, wts, n, st[2], 0, True))
            lkw = dict(loss=self.loss, loss_param=self.loss_param, weights=wts)
        ops.rows_copy_batch(segs)                                       # frames[a:b], labels[a:b], audios[a:b], weights[a:b]
        # train_step advances all four counters in its last launch: cursor += n, sub-batch index += 1
        if m.head == "classifier":
            loss, pred = m.train_step(aud, vis, lab, self.lr, self.betas, self.eps, _loop_tick=(n, 1), **self._step_kw())
            pred = ops.argmax_plus1(pred, torch.empty(n, dtype=F32, device=dev))        # main.py:190: argmax + 1 is what gets collected
            # predictions.extend(...), losses.append(...) at the positions the step started from
            ops.rows_copy_batch([(self._pred, pred, n, st[2], -n, False), (self._loss, loss, 1, st[3], -1, False)])
            return
        # regression head: that same last launch first writes predictions.extend(...), losses.append(...) at the positions the step
        # started from (main.py:195-196), then moves the counters
        m.train_step(aud, vis, lab, self.lr, self.betas, self.eps, _loop_tick=(n, 1),
                     _scatter=lambda loss, pred: [(self._pred, pred, n, st[2], 0, False), (self._loss, loss, 1, st[3], 0, False)], **lkw, **self._step_kw())

    def _sub_step_planned(self, n: int, vis, lab):
        """_sub_step with the sub-batch taken through the pass plan: frames plan[cursor : cursor + n] in that order, augmented as their
        rows say; labels, audio and weights follow the same order; the predictions go back to their frames' own positions."""
        m = self.model
        st = m._state
        dev = m._device
        if self._mix:
            ops.frames_gather_mix(self._vid, vis, self._plan, self._plan2, n, st[2], 0, self._colour)
        else:
            ops.frames_gather_aug(self._vid, vis, self._plan, n, st[2], 0, self._colour)
        segs = [(self._lab, lab, n, st[2], 0, True, True)]
        aud = None
        if m.audio_included:
            aud = torch.empty(n, 30, self._key[1], dtype=F32, device=dev)
            if self._mix_sig:       # the audio rows through both tables, in a launch of their own
                ops.audio_gather_aug(self._aud, aud, self._plan, self._plan2, n, st[2], 0, gain=self.audio_augment["gain"] > 0,
                                     noise=self.audio_augment["noise"], mix=self._mix)
            else:
                segs.append((self._aud, aud, n, st[2], 0, True, True))
        lkw = {}
        if self.loss != "mse_bcast":
            wts = None
            if self._weighted:
                wts = torch.empty(n, dtype=F32, device=dev)
                segs.append((self._wts, wts, n, st[2], 0, True, True))
            lkw = dict(loss=self.loss, loss_param=self.loss_param, weights=wts)
        if self._mix:               # labels and weights are blended like the inputs
            ops.rows_mix_indexed([s[:5] for s in segs], self._plan, self._plan2)
        else:
            ops.rows_copy_indexed(segs, self._plan)
        # the step's last launch moves the counters; the results are then written at the positions the step started from
        loss, pred = m.train_step(aud, vis, lab, self.lr, self.betas, self.eps, _loop_tick=(n, 1), **lkw, **self._step_kw())
        if m.head == "classifier":
            pred = ops.argmax_plus1(pred, torch.empty(n, dtype=F32, device=dev))        # main.py:190
        ops.rows_copy_indexed([(self._pred, pred, n, st[2], -n, False, True), (self._loss, loss, 1, st[3], -1, False, False)], self._plan)

    def _host_bookkeeping_after_replay(self):
        """What an eager train_step does on the host besides launching kernels."""
        m = self.model
        if self._phase[2] > 1:
            m._accum_advance(self._phase[2], m._bwd_frozen)     # one more micro-step of the window
        elif m._norm_of_acc:
            m._norm_of_acc = False
        if self._phase[1]:                          # a window's last micro-step (every step, without accumulation) updates
            m._adam_t += 1
            m._count_sat_out(m._bwd_frozen)         # the replayed optimizer step: one more that the frozen tensors sat out
        if not m.training:
            return                                  # eval(): no dropout draw, BatchNorm buffers untouched
        if m.dropout_mode == "device":
            m._drop_step += 1
        for i in (1, 2, 3):
            getattr(m.visbl, f"bnorm{i}").num_batches_tracked += 1

    def _run(self, n: int):
        m = self.model
        if not self.graphs or m.grad_sync is not None or m.dropout_mode == "given" or m.kernel_events is not None:
            self._sub_step(n)                       # collectives / supplied masks / per-kernel timing: eager
            self.eager_steps += 1
            return
        # the loss scale is a host scalar baked into the captured launches; the mode picks other kernels (eval(): running-stat
        # BatchNorm, no dropout), so a graph captured in one mode is never replayed in the other
        # Freezing (requires_grad=False) prunes the backward and bakes the fused Adam's ranges with their step counts into the launch:
        # the key carries them (() while everything trains), so a changed trainable set is captured afresh and never replays a stale
        # graph. While the set is stable the counts of its ranges are too — only frozen tensors sit steps out — and replays stay valid.
        # The loss is baked in too (its kind and beta are launch arguments, the weights a gathered segment): the key carries it.
        # (shuffle, colour, any-augment): which gather the graph holds; the draws themselves live in the plan table. The tests read
        # k[0] as the size, k[3] as the loss and k[-1] as the mode, so the new field sits in front of the mode.
        # The optimizer options (weight decay, clip norm, schedule constants) are launch arguments as well: their signature is k[5],
        # () without options. The schedule itself advances inside replays: it reads the device step counter.
        # The weight average's constants are launch arguments too, and its arena's address is baked in: its signature is k[6], ()
        # when off. Which steps copy, average or pass is decided inside replays, from the device step counter.
        # Accumulation: whether the micro-step overwrites or adds to the accumulator, whether it updates, and 1 / length
        # are baked into the launches, so the phase (first?, last?, length) is k[7]; (True, True, 1) without accumulation.
        # Audio augmentation / mixup: which gathers the graph holds, their flags and the noise amplitude are launch
        # arguments, so the two option signatures are k[8], () when both are off; the draws live in the second plan table.
        gkey = (n, m._loss_scale_for(n), m.trainable_signature(), (self.loss, self.loss_param, self._weighted),
                (self.shuffle, self._colour, self._augments), self._optim_sig, self._ema_sig, self._phase, self._mix_sig, m.training)
        g = self._graphs.get(gkey)
        if g is not None and self._uses_w5b.get(gkey) and m._w5b_version != m._w5_version():
            # the captured graph reads the bf16 copy of linear5.weight and keeps it fresh through its own fused Adam, but holds
            # no cast node: a writer outside the graph since the last step (load_state_dict, a stock optimizer, an in-place
            # edit) has left the copy stale. One eager step re-casts it (AVM._w5_bf16) and re-validates the stamp.
            self._sub_step(n)
            self.eager_steps += 1
            return
        if g is not None and not self._shadows.get(gkey) and m._w5b is not None and m._w5b_version == m._w5_version():
            # While the 16-bit copy is live the fused Adam of EVERY step refreshes it beside the fp32 master, also of a <= 16-row step
            # that never reads it. This graph was captured before the copy existed (or while it was stale): its Adam launch has no
            # shadow, so a replay would leave the copy one step behind under a valid version stamp and the next > 16-row step
            # would read it. Capture the size again, now with the shadow.
            del self._graphs[gkey]
            g = None
        if g is None:
            if gkey not in self._seen:              # first step of this size: eager (allocates Adam state, operand buffers)
                self._seen.add(gkey)
                self._sub_step(n)
                self.eager_steps += 1
                return
            saved = (m._adam_t, m._drop_step, [int(getattr(m.visbl, f"bnorm{i}").num_batches_tracked) for i in (1, 2, 3)],
                     m.keep_ctx)
            window = (m._accum_done, m._accum_k, m._accum_frozen)
            sat_out = dict(m._sat_out)
            m.keep_ctx = False
            g = torch.cuda.CUDAGraph()
            torch.cuda.synchronize()
            with torch.cuda.graph(g, pool=self._pool):
                self._sub_step(n)
            if self._pool is None:
                self._pool = g.pool()
            # capturing launched nothing: undo the host-side counters the captured code advanced
            m._adam_t, m._drop_step, nbt, m.keep_ctx = saved
            m._sat_out = sat_out
            m._accum_done, m._accum_k, m._accum_frozen = window
            for i, v in zip((1, 2, 3), nbt):
                getattr(m.visbl, f"bnorm{i}").num_batches_tracked.fill_(v)
            self._graphs[gkey] = g
            self._shadows[gkey] = m._w5b is not None and m._w5b_version == m._w5_version()
            self._uses_w5b[gkey] = self._shadows[gkey] and m.last_used_w5b
        g.replay()
        self._host_bookkeeping_after_replay()
        self.replays += 1

    # ---- exact save / resume --------------------------------------------------------------------------
    def _signatures(self):
        # (windows end with the video, so a state taken between two videos needs nothing about them; "accumulate" is listed only when
        # on, which keeps a default trainer's state what it was)
        acc = {} if self.accumulate == 1 else {"accumulate": self.accumulate}
        if self._mix_sig:       # listed only when on, as "accumulate" is
            acc["plan2"] = self._mix_sig
        return {**acc, "loss": (self.loss, self.loss_param), "plan": (self.shuffle, tuple(sorted(self.augment.items()))),
                "optim": self._optim_sig, "ema": self._ema_sig, "subbatch_size": self.subbatch_size,
                "step": (float(self.lr), tuple(float(b) for b in self.betas), float(self.eps))}

    def state_dict(self) -> dict:
        """The run so far, for `torch.save`: the model's training_state() plus the index of the next pass plan, the plan seed and the
        signatures of loss, shuffle / augment, optimizer options and weight average. Take it between two videos. One host sync."""
        return {"format": TRAINER_STATE_FORMAT, "model_state": self.model.training_state(), "passes": int(self.passes),
                "seed": int(self.seed), "signatures": self._signatures()}

    def load_state_dict(self, state: dict):
        """Continue the run a state_dict() was taken from: the next train_video is the one that run would have made next, bit for bit.
        ValueError where this trainer's loss, shuffle / augment, optimizer options, weight average, sub-batch size or step constants
        differ from the saved ones — a changed configuration is not an exact resume —; the model's own mismatches raise
        RuntimeError (AVM.load_training_state). The captured graphs stay valid: everything is restored in place."""
        if not isinstance(state, dict) or state.get("format") != TRAINER_STATE_FORMAT:
            raise ValueError(f"not a VideoTrainer state of format {TRAINER_STATE_FORMAT}")
        mine = self._signatures()
        for k, v in state["signatures"].items():
            if k not in mine or _plain(mine[k]) != _plain(v):
                raise ValueError(f"this trainer's {k} differs from the saved run's: {mine.get(k)!r} vs {v!r}")
        self.model.load_training_state(state["model_state"])
        self.passes = int(state["passes"])
        self.seed = int(state["seed"])

    # ---- validation pass ---------------------------------------------------------------------------------------------
    def eval_video(self, val_audios, val_frames, val_labels, weights=None):
        """main.py:218-226 for one video: the whole video in ONE forward under no_grad, then nn.MSELoss with its (n,1) x (n,)
        broadcast — or the trainer's `loss`, with optional per-frame `weights` (N,) for its pointwise kinds.
        The forward follows the model's mode: in train mode (the reference's, it never calls .eval()) BatchNorm uses batch statistics and updates its running buffers and dropout is live; after model.eval() BatchNorm uses the running
        statistics, nothing is updated and dropout is off. Returns (loss (1,), predictions (N,)) as GPU tensors; nothing has
        been synchronised."""
        m = self.model
        weights = self._check_weights(weights, val_frames.shape[0] if torch.is_tensor(val_frames) else 0)
        m._require_device()
        aud, vis, _ = m._to_device_inputs(val_audios, val_frames)
        lab = torch.as_tensor(val_labels).detach().to(device=m._device, dtype=F32).reshape(-1).contiguous()
        if lab.numel() != vis.shape[0]:
            raise RuntimeError(f"{lab.numel()} labels for {vis.shape[0]} frames")
        with torch.no_grad():
            out, _ = m.forward_device(aud, vis, save=False)
        loss = torch.empty(1, dtype=F32, device=m._device)
        if m.head == "classifier":
            ops.cross_entropy(out, lab, loss, None)                     # main.py:96-97
            return loss, ops.argmax_plus1(out, torch.empty(lab.numel(), dtype=F32, device=m._device))
        if self.loss != "mse_bcast":
            ops.frame_loss(out, lab, loss, None, self.loss, self.loss_param, None if weights is None else weights.to(m._device))
            return loss, out
        ops.mse_bcast(out, lab, loss, None)
        return loss, out

    def _check_weights(self, weights, n_frames):
        """per-frame loss weights of one video: ValueError where the trainer's loss takes none, RuntimeError on a wrong shape / dtype"""
        if weights is None:
            return None
        ops.loss_spec(self.loss, self.loss_param, True, self.model.head)
        if not (torch.is_tensor(weights) and weights.dtype == F32 and weights.numel() == n_frames):
            raise RuntimeError(f"weights must be a float32 tensor of {n_frames} elements")
        return weights.detach().reshape(-1).contiguous()

    # ---- the loop ------------------------------------------------------------------------------------------------
    def train_video(self, batch_audios, batch_frames, batch_labels, weights=None, plan_index=None):
        """One video (main.py:169-203). batch_frames (N,3,H,W), batch_audios (N,30,B) or a list of None,
        batch_labels (N,), weights (N,) float32 or None (the trainer's pointwise losses) — CPU or GPU tensors.
        Returns (losses (S,), predictions (N,)) as GPU tensors with S = ceil(N / subbatch_size); nothing has been synchronised. `losses.mean()` is main.py:203's batch_loss.
        With shuffle / augment on, the pass follows the plan of index `self.passes` (or `plan_index`, to resume a run): sub-batch s
        holds the frames plan[s * sb : (s + 1) * sb] names, `losses` is in sub-batch order and `predictions` in FRAME order.
        With audio_augment / mixup on, a second table of the same pass index carries the audio draws and the mixup partners
        (DESIGN.md §4.18). Under mixup `predictions[src_i]` is the model's output on the MIXED input of frame src_i — lambda of its
        own sample plus 1 - lambda of its partner's —, not on the frame itself: use `eval_video`, which never augments, for
        predictions of the video. ValueError, before anything is launched, if audio_augment's time_mask exceeds the audio bins."""
        if plan_index is not None and (isinstance(plan_index, bool) or not isinstance(plan_index, int) or not 0 <= plan_index < (1 << 28)):
            raise ValueError(f"plan_index must be an integer in [0, 2^28), got {plan_index!r}")
        m = self.model
        index = self.passes if plan_index is None else plan_index
        if self._mix_sig:       # before anything is allocated or launched
            if index >= (1 << 26):
                raise ValueError(f"audio_augment / mixup take pass indices below 2^26, got {index}")
            if self._audio_aug and torch.is_tensor(batch_audios) and batch_audios.dim() == 3 and self.audio_augment["time_mask"] > batch_audios.shape[2]:
                raise ValueError(f"audio_augment: time_mask = {self.audio_augment['time_mask']} is longer than the {batch_audios.shape[2]} "
                                 "audio bins of this video")
        weights = self._check_weights(weights, batch_frames.shape[0] if torch.is_tensor(batch_frames) else 0)
        m._require_device()
        if not torch.is_tensor(batch_frames) or batch_frames.dim() != 4 or batch_frames.shape[1] != 3:
            raise RuntimeError("batch_frames must be a (N,3,H,W) tensor")
        n_frames = batch_frames.shape[0]
        if n_frames < 1:
            raise RuntimeError("empty video")
        if batch_labels.numel() != n_frames:
            raise RuntimeError(f"{batch_labels.numel()} labels for {n_frames} frames")
        bins = 0
        if m.audio_included:
            if not torch.is_tensor(batch_audios) or batch_audios.dim() != 3 or batch_audios.shape[:2] != (n_frames, 30):
                raise RuntimeError("batch_audios must be (N,30,B) when audio_included=True")
            bins = batch_audios.shape[2]
        self._ensure_tables(n_frames, tuple(batch_frames.shape[2:]), bins)
        self._vid[:n_frames].copy_(batch_frames, non_blocking=True)
        self._lab[:n_frames].copy_(batch_labels.reshape(-1), non_blocking=True)
        self._weighted = weights is not None
        if weights is not None:
            self._wts[:n_frames].copy_(weights, non_blocking=True)
        if m.audio_included:
            self._aud[:n_frames].copy_(batch_audios, non_blocking=True)
        if m._state is None:
            m._make_state()
        m._state[2:4].zero_()                       # subbatch_offset, iterations (main.py:173-175)
        self.passes = index + 1
        if self._planned:
            ops.epoch_plan(self._plan, n_frames, self.seed, index, self.shuffle, **self.augment)
        if self._mix_sig:
            ops.epoch_plan2(self._plan2, self._plan, n_frames, self.seed, index, 30, max(bins, 1), **self.audio_augment, **self.mixup)
        if m.precision == "fp16":
            # the previous video's results have been read back by now (main.py:203): a cheap place to notice skipped steps and
            # halve the loss scale (AVM.update_loss_scale) — a static scale would otherwise stall training silently
            m.update_loss_scale()
        subs = 0
        for rows, pos, length in accum_windows(n_frames, self.subbatch_size, self.accumulate):
            self._phase = (pos == 0, pos == length - 1, length)
            self._run(rows)
            subs += 1
        return self._loss[:subs].clone(), self._pred[:n_frames].clone()
