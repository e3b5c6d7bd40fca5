"""Fine-tuning (requires_grad=False on AVM parameters): the frozen sets, the freeze schedule and its oracle, and the
device runners that tests/test_gpu_freeze.py uses. Split as tests/_mode_case.py is, so that the comparison can be run — and broken on
purpose — without a GPU (tests/test_freeze_host.py):

  frozen_set(set_id, names)   the sets F1 .. F6 of the tests
  oracle_schedule(...)        avm_ref.forward + torch.autograd.grad on the CPU, updated by torch.optim.Adam(foreach=False) with .grad = None
                              for the frozen tensors: torch itself supplies the per-parameter step count
  compare_schedule(...)       a device run (or a stand-in) against that, under the criterion of
                              test_gpu_avm.test_dropin_surface_cpu_tensors_autograd_and_stock_adam: predictions / loss within 2e-5, every
                              parameter within 2e-6 + the accumulated Adam-sensitivity slack; frozen tensors have no gradient and do not move
  frozen_step(...) / run_schedule_*(...)   the device side

The schedule is three PHASES — all trainable, F1, all trainable — of one optimizer step per sub-batch of SUB frames of the same video:
one sub-batch per phase in the golden (10 frames), three in the device test (30 frames, so that loop.VideoTrainer captures and replays
a graph in every phase). Dropout is the counter-based stream of seed synth.BASE_SEED: draw k of the device is
synth.make_drop_masks(n, step=k) on the CPU."""
import functools

import torch

from cvml_goalnet_amd import synth
from oracle import avm_ref

DEV = "cuda:0"
H = 40
LR = 1e-3
SUB = 10
SCHEDULE = ("none", "F1", "none")

_RULES = {
    "none": lambda k: False,
    "F1": lambda k: k.startswith("visbl."),
    "F2": lambda k: not k.startswith("fusion.12."),
    "F3": lambda k: k == "visbl.linear5.weight",
    "F4": lambda k: k.startswith("fusion."),                       # trainable tensors lie beneath frozen layers
    "F5": lambda k: k.endswith(".bias") or ".bnorm" in k,          # every bias and every BatchNorm weight / bias: many ranges
    "F6": lambda k: k.startswith("audbl."),
}


def frozen_set(set_id, names):
    return frozenset(k for k in names if _RULES[set_id](k))


def apply_flags(model, frozen):
    for k, p in model.named_parameters():
        p.requires_grad = k not in frozen


# ---- the oracle ------------------------------------------------------------------------------------------------------------------
def schedule_inputs(frames):
    return (torch.from_numpy(synth.make_audio(frames)), torch.from_numpy(synth.make_visual(frames, H, H)),
            torch.from_numpy(synth.make_labels(frames)))


def start_params():
    return {k: torch.from_numpy(v.copy()) for k, v in synth.make_params(H, H, 30, True).items()}


def oracle_schedule(p0, aud, vis, lab, schedule=SCHEDULE, dropout=True, per_tensor_count=True):
    """One dict per optimizer step: loss, pred, grads (trainable tensors only), params after the step, frozen. per_tensor_count=False
    is the WRONG optimizer the host test must see rejected: one global step count (avm_ref.adam_step), so that a tensor that sat a step
    out is bias-corrected as if it had not."""
    p = {k: torch.nn.Parameter(v.clone()) for k, v in p0.items()}
    b = avm_ref.init_buffers()
    opt = torch.optim.Adam(list(p.values()), lr=LR, foreach=False)
    state, steps, draw = {}, [], 0
    for set_id in schedule:
        frozen = frozen_set(set_id, p)
        train = [k for k in p if k not in frozen]
        for a in range(0, vis.shape[0], SUB):
            masks = [torch.from_numpy(m) for m in synth.make_drop_masks(min(SUB, vis.shape[0] - a), step=draw)] if dropout else None
            draw += 1
            pred = avm_ref.forward(p, b, aud[a:a + SUB], vis[a:a + SUB], masks, True)
            loss = avm_ref.mse_bcast(pred, lab[a:a + SUB])
            grads = dict(zip(train, torch.autograd.grad(loss, [p[k] for k in train])))
            with torch.no_grad():
                if per_tensor_count:
                    for k, q in p.items():
                        q.grad = grads.get(k)                     # None for a frozen tensor: torch.optim.Adam skips it, count included
                    opt.step()
                else:
                    avm_ref.adam_step(p, grads, state, lr=LR)
            steps.append({"loss": float(loss.detach()), "pred": pred.detach().view(-1).clone(), "grads": {k: g.clone() for k, g in grads.items()},
                          "params": {k: q.detach().clone() for k, q in p.items()}, "frozen": frozen})
    return steps


def compare_schedule(dev_steps, ref_steps, p0):
    """the criterion of the module docstring; `dev_steps` has the layout of oracle_schedule's result ("grads" may hold None)"""
    assert len(dev_steps) == len(ref_steps)
    slack, prev = {}, p0
    for i, (d, r) in enumerate(zip(dev_steps, ref_steps)):
        assert (d["pred"] - r["pred"]).abs().max().item() < 2e-5, f"step {i}: predictions"
        assert abs(d["loss"] - r["loss"]) < 2e-5 * max(1.0, abs(r["loss"])), f"step {i}: loss"
        for k, rp in r["params"].items():
            mine = d["params"][k].reshape(rp.shape)
            if k in r["frozen"]:
                assert d["grads"].get(k) is None, f"step {i}: {k} is frozen and has a gradient"
                assert torch.equal(mine, prev[k].reshape(rp.shape)), f"step {i}: {k} is frozen and moved"
            else:
                og = r["grads"][k]
                gerr = (d["grads"][k].reshape(og.shape) - og).abs()
                slack[k] = slack.get(k, 0.0) + LR * torch.clamp(8.0 * gerr / (og.abs() + 1e-8), max=2.0)
            over = ((mine - rp).abs() - (2e-6 + slack.get(k, 0.0))).max().item()
            assert over <= 0, f"step {i}: {k} exceeds its Adam-sensitivity bound by {over:.3e}"
        prev = d["params"]


# ---- the device: one step under a frozen set (bit-identity, pruning, poison) -----------------------------------------------------------
def load_model(fx, audio=True, precision="fp32", mode="train"):
    from cvml_goalnet_amd import AVM
    m = AVM(audio_included=audio, device=DEV, seed=synth.BASE_SEED, precision=precision)
    sd = {k: v.clone() for k, v in fx["p"].items()}
    sd.update({k: v.clone() for k, v in fx["b"].items()})
    m.load_state_dict(sd)
    if mode == "train":
        m.set_dropout_masks(fx["masks"])
    else:
        m.eval()
    return m


def frozen_step(fx, set_id, audio=True, precision="fp32", mode="train", poison=False, before_step=None):
    """one train_step with the tensors of `set_id` frozen -> everything the comparisons read, as GPU tensors. poison: the gradient
    arena holds NaN everywhere when the step starts. before_step(model): hook (the call counters of the pruning test)."""
    m = load_model(fx, audio, precision, mode)
    frozen = frozen_set(set_id, fx["p"])
    apply_flags(m, frozen)
    arena0 = m._arena.clone()
    if poison:
        m._ensure_garena()
        m._garena.fill_(float("nan"))
    if before_step:
        before_step(m)
    loss, pred = m.train_step(fx["aud"].to(DEV) if audio else None, fx["vis"].to(DEV), fx["lab"].to(DEV), lr=LR)
    torch.cuda.synchronize()
    grads = {s.name: (None if m.grad_of(s.name) is None else m.grad_of(s.name).clone()) for s in m._specs}
    bufs = {k: v.clone() for k, v in m.named_buffers()}
    return {"model": m, "frozen": frozen, "loss": loss.clone(), "pred": pred.clone(), "grads": grads, "arena0": arena0, "bufs": bufs}


@functools.lru_cache(maxsize=None)
def unfrozen_step(n, audio=True, precision="fp32", mode="train"):
    """the all-trainable step of a cell: computed once, shared by every frozen set, never modified"""
    from _mode_case import fixture
    return frozen_step(fixture("regression", audio, mode, n), "none", audio, precision, mode)


def flat(model, arena, name):
    s = model.spec(name)
    return arena[s.offset:s.offset + s.numel]


def assert_frozen_step_equals_unfrozen(fz, ref):
    """test 1 of the issue: bit-identity of everything trainable, and frozen tensors with their moments exactly where they were"""
    m, r = fz["model"], ref["model"]
    assert torch.equal(fz["pred"], ref["pred"]) and torch.equal(fz["loss"], ref["loss"])
    for k, v in ref["bufs"].items():
        assert torch.equal(fz["bufs"][k], v), k
    for s in m._specs:
        k = s.name
        if k in fz["frozen"]:
            assert fz["grads"][k] is None, f"{k} is frozen and has a gradient"
            assert torch.equal(flat(m, m._arena, k), flat(m, fz["arena0"], k)), f"{k} is frozen and moved"
            for mom in (m._adam_m, m._adam_v):                    # before the first step the moments are zero
                assert not flat(m, mom, k).any().item(), f"a moment of the frozen {k} moved"
        else:
            assert torch.equal(fz["grads"][k], ref["grads"][k]), f"gradient of {k}"
            assert torch.equal(flat(m, m._arena, k), flat(r, r._arena, k)), f"{k} after the step"
            assert torch.equal(flat(m, m._adam_m, k), flat(r, r._adam_m, k)) and torch.equal(flat(m, m._adam_v, k), flat(r, r._adam_v, k)), k
    assert not m._sat_out or set(m._sat_out) == set(fz["frozen"])


# ---- the device: the freeze schedule through the three training surfaces ---------------------------------------------------------------
def _schedule_model(p0):
    from cvml_goalnet_amd import AVM
    m = AVM(audio_included=True, device=DEV, seed=synth.BASE_SEED)       # dropout_mode "device": draw k = synth.make_drop_masks(step=k)
    sd = {k: v.clone() for k, v in p0.items()}
    sd.update(avm_ref.init_buffers())
    m.load_state_dict(sd)
    return m


def _record(m, loss, pred, frozen):
    sd = m.state_dict()
    return {"loss": float(loss), "pred": pred.detach().view(-1).cpu(), "frozen": frozen,
            "grads": {s.name: (None if m.grad_of(s.name) is None else m.grad_of(s.name).cpu()) for s in m._specs},
            "params": {s.name: sd[s.name] for s in m._specs}}


def run_schedule_train_step(p0, aud, vis, lab, schedule=SCHEDULE):
    m, steps = _schedule_model(p0), []
    aud, vis, lab = aud.to(DEV), vis.to(DEV), lab.to(DEV)
    for set_id in schedule:
        frozen = frozen_set(set_id, p0)
        apply_flags(m, frozen)
        for a in range(0, vis.shape[0], SUB):
            loss, pred = m.train_step(aud[a:a + SUB], vis[a:a + SUB], lab[a:a + SUB], lr=LR)
            steps.append(_record(m, loss, pred, frozen))
    return m, steps


def run_schedule_trainer(p0, aud, vis, lab, schedule=SCHEDULE):
    """loop.VideoTrainer with graphs: per phase one video = eager step, capture + replay, replay. Results per VIDEO (losses, predictions)."""
    from cvml_goalnet_amd.loop import VideoTrainer
    m, out = _schedule_model(p0), []
    tr = VideoTrainer(m, subbatch_size=SUB, lr=LR)
    for set_id in schedule:
        apply_flags(m, frozen_set(set_id, p0))
        out.append(tr.train_video(aud, vis, lab))
    torch.cuda.synchronize()
    return m, tr, out


def run_schedule_dropin(p0, aud, vis, lab, schedule=SCHEDULE):
    """the autograd drop-in with model.make_optimizer(); dL/dpred comes from the project's own broadcast-MSE kernel, the one train_step
    uses, so that the run can be compared bit for bit with the other two surfaces"""
    from cvml_goalnet_amd import ops
    m, out = _schedule_model(p0), []
    opt = m.make_optimizer(lr=LR)
    aud, vis, lab = aud.to(DEV), vis.to(DEV), lab.to(DEV)
    for set_id in schedule:
        apply_flags(m, frozen_set(set_id, p0))
        for a in range(0, vis.shape[0], SUB):
            opt.zero_grad()
            pred = m(aud[a:a + SUB], vis[a:a + SUB])
            loss = torch.empty(1, dtype=torch.float32, device=DEV)
            dout = torch.empty(pred.shape[0], dtype=torch.float32, device=DEV)
            ops.mse_bcast(pred.detach().view(-1).contiguous(), lab[a:a + SUB].contiguous(), loss, dout)
            pred.backward(dout.view(-1, 1))
            opt.step()
            out.append((loss, pred.detach().view(-1)))
    torch.cuda.synchronize()
    return m, out
