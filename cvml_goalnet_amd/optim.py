"""`Adam` — `torch.optim.Adam(model.parameters(), lr=...)` (/root/reference/main.py:70, 187, 193) as ONE fused pass over the AVM's flat
parameter arena instead of torch's per-tensor passes over 30 strided views.

    optimizer = cvml_goalnet_amd.optim.Adam(model.parameters(), lr=0.001)      # was: optim.Adam(params = model.parameters(), lr = lr)
    optimizer.zero_grad(); loss.backward(); optimizer.step()                   # main.py:187-193, unchanged

Same defaults and the same arithmetic as torch's single-tensor Adam (betas (0.9, 0.999), eps 1e-8, no weight decay, no amsgrad,
bias-corrected; `goalnet_adam_step_dev`, csrc/small.hip). The parameters must be those of ONE `AVM` (they are views of its arena, and
autograd leaves their gradients in its gradient arena: `_AVMFunction.backward`); like the stock optimizer it may be constructed before
the first forward (Lazy parameters). Parameters with `requires_grad=False` are left alone, moments and step count included (pass all
parameters or only the trainable ones). `zero_grad()` only drops the `.grad` references: the gradient arena is overwritten by every
backward. State (`exp_avg`, `exp_avg_sq`, step) lives in the model (`AVM._adam_m`, `_adam_v`, the device step counter).

EXTENSION: `OptimOptions` — weight decay (coupled as `torch.optim.Adam(weight_decay=)`, decoupled as
`torch.optim.AdamW`), clipping by the global gradient norm (`torch.nn.utils.clip_grad_norm_`) and a learning-rate schedule that the
device evaluates from its step counter — for `AVM.train_step(optim=)`, `AVM.adam_step(optim=)`, `loop.VideoTrainer(optim=)` and the
drop-in `Adam(weight_decay=, max_grad_norm=, options=)` / `AdamW`. No AMSGrad, no per-tensor rates.

EXTENSION: `EmaOptions` — an exponential moving average of the weights in a third arena, one launch behind every
optimizer step, for the same four places (`ema=`); read it with `AVM.ema_of(name)` or evaluate / save under `with model.averaged():`.
"""
from __future__ import annotations

import dataclasses
import math
from typing import Optional, Tuple

import torch

from .avm import AVM

SCHEDULES = ("constant", "cosine", "step")


def _is_int(x):
    return isinstance(x, int) and not isinstance(x, bool)


@dataclasses.dataclass(frozen=True)
class OptimOptions:
    """What the fused step does beyond torch.optim.Adam's defaults. Everything off by default: `trivial`, and the step is then exactly
    the one without options.
      weight_decay, decoupled   g += wd * p before Adam (False: torch.optim.Adam) or p *= 1 - lr_t * wd (True: torch.optim.AdamW)
      no_decay                  name substrings of the tensors that get no decay, e.g. ("bias", "bnorm")
      max_grad_norm             None, or the cap on the L2 norm of all trainable gradients (torch.nn.utils.clip_grad_norm_)
      schedule                  "constant" | "cosine" (total_steps, min_lr) | "step" (step_period, gamma), after `warmup_steps` of
                                linear warm-up; lr_at() is the closed form, the device evaluates the same from its step counter"""
    weight_decay: float = 0.0
    decoupled: bool = False
    no_decay: Tuple[str, ...] = ()
    max_grad_norm: Optional[float] = None
    schedule: str = "constant"
    warmup_steps: int = 0
    total_steps: Optional[int] = None
    min_lr: float = 0.0
    step_period: Optional[int] = None
    gamma: float = 0.1

    def __post_init__(self):
        def real(x):
            return isinstance(x, (int, float)) and not isinstance(x, bool) and math.isfinite(x)
        if not real(self.weight_decay) or self.weight_decay < 0:
            raise ValueError(f"weight_decay must be a finite number >= 0, got {self.weight_decay!r}")
        if isinstance(self.no_decay, str) or not all(isinstance(s, str) and s for s in self.no_decay):
            raise ValueError("no_decay is a tuple of non-empty name substrings")
        object.__setattr__(self, "no_decay", tuple(self.no_decay))
        object.__setattr__(self, "decoupled", bool(self.decoupled))
        if self.max_grad_norm is not None and (not real(self.max_grad_norm) or self.max_grad_norm <= 0):
            raise ValueError(f"max_grad_norm must be None or a finite number > 0, got {self.max_grad_norm!r}")
        if self.schedule not in SCHEDULES:
            raise ValueError(f"schedule must be one of {SCHEDULES}, got {self.schedule!r}")
        if not _is_int(self.warmup_steps) or self.warmup_steps < 0:
            raise ValueError(f"warmup_steps must be an integer >= 0, got {self.warmup_steps!r}")
        if not real(self.min_lr) or self.min_lr < 0:
            raise ValueError(f"min_lr must be a finite number >= 0, got {self.min_lr!r}")
        if self.schedule == "cosine":
            if not _is_int(self.total_steps) or self.total_steps <= self.warmup_steps:
                raise ValueError("the cosine schedule needs an integer total_steps > warmup_steps")
        elif self.total_steps is not None and (not _is_int(self.total_steps) or self.total_steps < 0):
            raise ValueError(f"total_steps must be None or an integer >= 0, got {self.total_steps!r}")
        if self.schedule == "step":
            if not _is_int(self.step_period) or self.step_period < 1:
                raise ValueError("the step schedule needs an integer step_period >= 1")
            if not real(self.gamma) or self.gamma <= 0:
                raise ValueError(f"gamma must be a finite number > 0, got {self.gamma!r}")
        elif self.step_period is not None and (not _is_int(self.step_period) or self.step_period < 1):
            raise ValueError(f"step_period must be None or an integer >= 1, got {self.step_period!r}")

    @property
    def trivial(self) -> bool:
        """nothing is switched on: the step is the one without options, launch for launch"""
        return self.weight_decay == 0 and self.max_grad_norm is None and self.schedule == "constant" and self.warmup_steps == 0

    def signature(self) -> tuple:
        """hashable: everything a captured step bakes in about the options (() when trivial)"""
        if self.trivial:
            return ()
        return (float(self.weight_decay), self.decoupled, self.no_decay, None if self.max_grad_norm is None else float(self.max_grad_norm),
                self.schedule, self.warmup_steps, self.total_steps, float(self.min_lr), self.step_period, float(self.gamma))

    def decays(self, name: str) -> bool:
        """weight decay applies to the tensor of this name"""
        return self.weight_decay > 0 and not any(s in name for s in self.no_decay)

    def lr_at(self, base_lr: float, e: int) -> float:
        """the learning rate of the step that starts from `e` completed steps (step t = e + 1 runs at the rate after t - 1 scheduler
        ticks, torch's convention) — the expression of csrc/optim.hip's sched_lr, operation for operation"""
        lr, w = float(base_lr), self.warmup_steps
        if e < w:
            return lr * float(e + 1) / float(w)
        if self.schedule == "cosine":
            T, e1 = self.total_steps - w, e - w
            return self.min_lr + (lr - self.min_lr) * (1.0 + math.cos(math.pi * float(min(e1, T)) / float(T))) / 2.0
        if self.schedule == "step":
            return lr * math.pow(self.gamma, float((e - w) // self.step_period))
        return lr


@dataclasses.dataclass(frozen=True)
class EmaOptions:
    """An exponential moving average of the weights, kept on the device behind every optimizer step. With t the
    1-based count of applied optimizer steps:
      start_step   up to here the average is a copy of the weights (it tracks them); averaging begins with step start_step + 1
      every        afterwards every `every`-th step averages, the others leave the average alone
      decay        e += (1 - d) (p - e) with d = decay, or
      warmup       d = min(decay, (1 + k) / (10 + k)) after k averaging updates: a young average forgets its start quickly
    weight_at() is the closed form; the device evaluates the same from its step counter."""
    decay: float = 0.999
    warmup: bool = False
    every: int = 1
    start_step: int = 0

    def __post_init__(self):
        d = self.decay
        if not isinstance(d, (int, float)) or isinstance(d, bool) or not math.isfinite(d) or not 0.0 <= d < 1.0:
            raise ValueError(f"decay must be a finite number in [0, 1), got {d!r}")
        if not isinstance(self.warmup, (bool, int)):
            raise ValueError(f"warmup must be a bool, got {self.warmup!r}")
        if not _is_int(self.every) or self.every < 1:
            raise ValueError(f"every must be an integer >= 1, got {self.every!r}")
        if not _is_int(self.start_step) or self.start_step < 0:
            raise ValueError(f"start_step must be an integer >= 0, got {self.start_step!r}")
        object.__setattr__(self, "decay", float(d))
        object.__setattr__(self, "warmup", bool(self.warmup))

    def signature(self) -> tuple:
        """hashable: everything a captured step bakes in about the average"""
        return (self.decay, self.warmup, self.every, self.start_step)

    def weight_at(self, t: int) -> Optional[float]:
        """what optimizer step t (1-based) does to the average: 1.0 = a copy of the weights, None = nothing is written, otherwise
        the fp64 value of 1 - d that the kernel rounds to fp32 — the expression of csrc/ema.hip's ema_plan, operation for operation"""
        if t <= self.start_step:
            return 1.0
        u = t - self.start_step
        if u % self.every != 0:
            return None
        k = u // self.every - 1
        d = self.decay
        if self.warmup:
            d = min(d, float(1 + k) / float(10 + k))
        return 1.0 - d


def _ema(ema):
    if ema is not None and not isinstance(ema, EmaOptions):
        raise ValueError("ema must be an optim.EmaOptions")
    return ema


def _options(options, weight_decay, max_grad_norm, decoupled):
    if options is not None:
        if not isinstance(options, OptimOptions):
            raise ValueError("options must be an OptimOptions")
        if weight_decay is not None or max_grad_norm is not None:
            raise ValueError("pass weight_decay / max_grad_norm either as keywords or inside options, not both")
        if options.weight_decay > 0 and options.decoupled != decoupled:
            raise ValueError(f"options.decoupled must be {decoupled} for this optimizer")
        return options
    return OptimOptions(weight_decay=0.0 if weight_decay is None else weight_decay, decoupled=decoupled, max_grad_norm=max_grad_norm)


class Adam(torch.optim.Optimizer):
    _decoupled = False

    def __init__(self, params, lr=1e-3, betas=(0.9, 0.999), eps=1e-8, model: AVM = None, weight_decay=None, max_grad_norm=None,
                 options: Optional[OptimOptions] = None, ema: Optional[EmaOptions] = None):
        params = list(params)
        if not 0.0 <= lr or not 0.0 <= eps or not (0.0 <= betas[0] < 1.0 and 0.0 <= betas[1] < 1.0):
            raise ValueError("invalid Adam hyper-parameters")
        self.options = _options(options, weight_decay, max_grad_norm, self._decoupled)       # ValueError before anything is launched
        self.ema = _ema(ema)
        super().__init__(params, dict(lr=lr, betas=betas, eps=eps))
        self._model = model

    def _find_model(self):
        if self._model is None:
            raise RuntimeError("cvml_goalnet_amd.optim.Adam: pass model=<the AVM> (or use AVM.make_optimizer()) — the parameters of one AVM "
                               "live in one flat arena and are stepped together")
        return self._model

    @torch.no_grad()
    def step(self, closure=None):
        loss = None
        if closure is not None:
            with torch.enable_grad():
                loss = closure()
        m = self._find_model()
        if m._garena is None:
            raise RuntimeError("step() before any backward: there are no gradients")
        if len(self.param_groups) != 1:
            raise RuntimeError("one parameter group: the arena is updated in one pass")
        g = self.param_groups[0]
        # as torch.optim.Adam skips a parameter whose grad is None, the pass skips the tensors that were frozen (requires_grad=False)
        # in the last backward: the optimizer holds either all parameters or exactly the trainable ones
        every = {id(getattr(*m._module_of(s.name))) for s in m._specs}
        trainable = {id(getattr(*m._module_of(s.name))) for s in m._specs if s.name not in m._bwd_frozen}
        if {id(p) for p in g["params"]} not in (every, trainable):
            raise RuntimeError("cvml_goalnet_amd.optim.Adam steps ALL parameters of its AVM (model.parameters()), or all that have "
                               "requires_grad=True (filter(lambda p: p.requires_grad, model.parameters()))")
        m.adam_step(g["lr"], tuple(g["betas"]), g["eps"], optim=None if self.options.trivial else self.options, ema=self.ema)
        return loss

    def zero_grad(self, set_to_none: bool = True):
        for g in self.param_groups:
            for p in g["params"]:
                p.grad = None


class AdamW(Adam):
    """`torch.optim.AdamW(model.parameters(), lr, weight_decay=0.01)`: Adam with decoupled weight decay, p *= 1 - lr_t * wd before the
    update, on the same fused pass."""
    _decoupled = True

    def __init__(self, params, lr=1e-3, betas=(0.9, 0.999), eps=1e-8, model: AVM = None, weight_decay=None, max_grad_norm=None,
                 options: Optional[OptimOptions] = None, ema: Optional[EmaOptions] = None):
        if options is None and weight_decay is None:
            weight_decay = 1e-2                     # torch.optim.AdamW's default
        super().__init__(params, lr=lr, betas=betas, eps=eps, model=model, weight_decay=weight_decay, max_grad_norm=max_grad_norm,
                         options=options, ema=ema)
