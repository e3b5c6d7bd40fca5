"""GPU: exact save / resume. Run A trains three videos of 25 frames through loop.VideoTrainer with shuffling,
augmentation, decoupled weight decay, clipping, a cosine schedule with warm-up and a weight average, and takes state_dict() after the
first video. A fresh model and trainer B load that state — through torch.save / torch.load into a buffer — and train videos 2 and 3.
A and B then agree BIT FOR BIT in the parameter arena, both moments, the average, the device counters and guard words, the BatchNorm
buffers, and the losses and predictions of both videos: the dropout stream, the plan index, the schedule position, the per-tensor
counts of sat-out steps and the fp16 loss-scale fields all came across."""
import io

import pytest
import torch

pytestmark = pytest.mark.gpu

if not torch.cuda.is_available():
    pytest.skip("no GPU", allow_module_level=True)

from _abi_guard import bits_equal                                   # noqa: E402
from _freeze_case import start_params                               # noqa: E402
from cvml_goalnet_amd import AVM, EmaOptions, OptimOptions, synth   # noqa: E402
from cvml_goalnet_amd.loop import VideoTrainer                      # noqa: E402
from oracle import avm_ref                                          # noqa: E402

DEV = "cuda:0"
H = 40
LR = 1e-3
OPTIM = OptimOptions(weight_decay=0.01, decoupled=True, max_grad_norm=0.05, schedule="cosine", warmup_steps=3, total_steps=20)
EMA = EmaOptions(decay=0.9, warmup=True, start_step=2)
AUGMENT = {"flip_p": 0.5, "max_shift": 2, "contrast": 0.2, "brightness": 0.1}


def _video(salt, frames=25):
    seed = synth.BASE_SEED + salt
    return (torch.from_numpy(synth.make_audio(frames, seed=seed)), torch.from_numpy(synth.make_visual(frames, H, H, seed=seed)),
            torch.from_numpy(synth.make_labels(frames, seed=seed)))


def _trainer(model, optim=OPTIM, ema=EMA):
    return VideoTrainer(model, subbatch_size=10, lr=LR, shuffle=True, augment=AUGMENT, seed=1234, optim=optim, ema=ema)


def _start(precision):
    m = AVM(audio_included=True, device=DEV, seed=synth.BASE_SEED + 5, precision=precision)
    sd = start_params()
    sd.update(avm_ref.init_buffers())
    m.load_state_dict(sd)
    return m


def _through_a_buffer(state):
    buf = io.BytesIO()
    torch.save(state, buf)
    buf.seek(0)
    return torch.load(buf)


def _assert_same_run(a, b, outs_a, outs_b):
    for what in ("_arena", "_adam_m", "_adam_v", "_ema", "_state", "_guard"):
        assert bits_equal(getattr(a, what), getattr(b, what)), f"{what} differs between the continuous and the resumed run"
    bufs_b = dict(b.named_buffers())
    for k, v in a.named_buffers():
        assert torch.equal(v.cpu(), bufs_b[k].cpu()), k
    for i, ((la, pa), (lb, pb)) in enumerate(zip(outs_a, outs_b)):
        assert bits_equal(la, lb) and bits_equal(pa, pb), f"losses / predictions of video {i + 2}"
    assert (a._adam_t, a._drop_step, a._sat_out, a._loss_scale_backoff, a._skipped_seen) == \
        (b._adam_t, b._drop_step, b._sat_out, b._loss_scale_backoff, b._skipped_seen)


@pytest.mark.parametrize("variant", ["fp32", "fp32-frozen-block", "fp16-after-a-skipped-step"])
def test_a_resumed_run_is_the_continuous_run(variant):
    precision = "fp16" if variant.startswith("fp16") else "fp32"
    a = _start(precision)
    if variant == "fp16-after-a-skipped-step":
        v0 = _video(9, 10)
        a.loss_scale = 2.0 ** 60                                          # every 16-bit activation gradient overflows: the step is skipped
        a.train_step(v0[0].to(DEV), v0[1].to(DEV), v0[2].to(DEV), lr=LR, optim=OPTIM, ema=EMA)
        a.loss_scale = None
        assert a.overflow_skipped_steps() == 1 and a._state[0].item() == 0
    if variant == "fp32-frozen-block":
        a.audbl.requires_grad_(False)                                     # sits video 1 out, trains again afterwards
    ta = _trainer(a)
    ta.train_video(*_video(1))
    torch.cuda.synchronize()
    state = _through_a_buffer(ta.state_dict())
    a.audbl.requires_grad_(True)
    outs_a = [ta.train_video(*_video(2)), ta.train_video(*_video(3))]
    torch.cuda.synchronize()

    b = AVM(audio_included=True, device=DEV, precision=precision)        # fresh: another dropout seed, nothing materialised
    tb = _trainer(b)
    tb.load_state_dict(state)
    assert tb.passes == 1 and b._adam_t == a._adam_t - 6 and b.dropout_seed == a.dropout_seed
    if variant == "fp32-frozen-block":
        assert b._sat_out and all(v == 3 for v in b._sat_out.values()), "three optimizer steps sat out by every AudBl tensor"
    if variant == "fp16-after-a-skipped-step":
        assert b._guard.tolist() == [0, 1] and b._loss_scale_backoff == 1 and b._skipped_seen == 1, "back-off and guard words came across"
    outs_b = [tb.train_video(*_video(2)), tb.train_video(*_video(3))]
    torch.cuda.synchronize()
    _assert_same_run(a, b, outs_a, outs_b)
    assert a._state[0].item() == 9 and tb.passes == ta.passes == 3
    assert not bits_equal(a._ema, a._arena)


def test_mismatches_are_refused():
    a = _start("fp32")
    ta = _trainer(a)
    ta.train_video(*_video(1, 10))
    state = _through_a_buffer(ta.state_dict())
    with pytest.raises(ValueError, match="optim"):
        _trainer(AVM(audio_included=True, device=DEV), optim=OptimOptions(weight_decay=0.02, decoupled=True)).load_state_dict(state)
    with pytest.raises(ValueError, match="ema"):
        _trainer(AVM(audio_included=True, device=DEV), ema=None).load_state_dict(state)
    other = AVM(audio_included=True, device=DEV, head="classifier")
    with pytest.raises(RuntimeError, match="head"):
        other.load_training_state(state["model_state"])
    assert not other._materialized, "refused before anything was loaded"
    with pytest.raises(RuntimeError, match="precision"):
        AVM(audio_included=True, device=DEV, precision="bf16").load_training_state(state["model_state"])
