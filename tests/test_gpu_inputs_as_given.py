"""GPU: train_step on inputs as callers hand them over — strided views, float64, channels_last, integer labels, label columns.

The kernels read bare pointers and element counts. AVM.forward and VideoTrainer normalise what they are given; AVM.train_step now does
the same (audio and visual by the route of forward, labels to one flat contiguous fp32 row), and the wrappers that checked `numel` only
refuse anything but contiguous fp32 before a launch.

  * TWINS: two identically loaded models; model A steps on the awkward twin, model B on twin.float().contiguous(). Loss, predictions and
    every arena (parameters, gradients, both Adam moments) and BatchNorm buffer after the step are bit-identical. Sizes: n = 10 (the
    fused MLP evaluates the loss in its own launch), n = 20 (ops.mse_bcast), the classifier head at n = 10 (ops.cross_entropy); B = 30.
    Every twin owns at least as many bytes from its data_ptr() as a contiguous fp32 tensor of its shape (asserted), so a step that
    trusted the tensor would compute wrong numbers from inside an allocation, never read outside one.
  * WRAPPER CHECKS: with ops.lib replaced by a proxy that fails the test when a launching entry point is reached, every bad argument
    raises RuntimeError; the same proxy passes a good call through, so it does see launches."""
import pytest
import torch

pytestmark = pytest.mark.gpu

import eval_ref  # noqa: E402
from cvml_goalnet_amd import AVM, ops, synth  # noqa: E402
from oracle import avm_ref  # noqa: E402

DEV = "cuda:0"
H = 40
B = 30
LR = 1e-3

KINDS = {"fused-mlp-n10": ("regression", 10), "mse-bcast-n20": ("regression", 20), "classifier-n10": ("classifier", 10)}


def _model(head):
    params = eval_ref.classifier_params(H, True) if head == "classifier" else synth.make_params(H, H, B, True)
    m = AVM(audio_included=True, device=DEV, seed=synth.BASE_SEED, head=head)
    sd = {k: torch.from_numpy(v.copy()) for k, v in params.items()}
    sd.update(avm_ref.init_buffers())
    m.load_state_dict(sd)
    return m


def _base(n):
    return (torch.from_numpy(synth.make_audio(n, B)).to(DEV), torch.from_numpy(synth.make_visual(n, H, H)).to(DEV),
            torch.from_numpy(synth.make_labels(n, seed=synth.BASE_SEED + 1)).to(DEV))


# ---- the twins: (audio, visual, labels) -> the same values in an awkward container -----------------------------------------------------
def _aud_wide(a, v, y):
    wide = torch.full((a.shape[0], 30, B + 7), 1e4, device=DEV)       # what a reader that ignores the strides picks up instead
    wide[:, :, :B] = a
    return wide[:, :, :B], v, y


def _aud_transposed(a, v, y):
    return a.transpose(1, 2).contiguous().transpose(1, 2), v, y         # (n, B, 30) in memory


def _inputs_f64(a, v, y):
    return a.double(), v.double(), y


def _vis_channels_last(a, v, y):
    return a, v.contiguous(memory_format=torch.channels_last), y


def _lab_column(a, v, y):
    table = torch.full((y.numel(), 3), 7.0, device=DEV)
    table[:, 0] = y
    return a, v, table[:, 0]


def _lab_f64(a, v, y):
    return a, v, y.double()


def _lab_int64(a, v, y):
    assert torch.equal(y, y.round())
    return a, v, y.long()


def _lab_n_by_1(a, v, y):
    return a, v, y.reshape(-1, 1)


TWINS = {"audio-wide-slice": _aud_wide, "audio-transposed": _aud_transposed, "audio-visual-float64": _inputs_f64,
         "visual-channels-last": _vis_channels_last, "labels-table-column": _lab_column, "labels-float64": _lab_f64,
         "labels-int64": _lab_int64, "labels-n-by-1": _lab_n_by_1}


def _owned_bytes(t):
    return t.untyped_storage().nbytes() - t.storage_offset() * t.element_size()


def _snapshot(m, loss, pred):
    torch.cuda.synchronize()
    out = {"loss": loss.clone(), "pred": pred.clone(), "arena": m._arena.clone(), "grads": m._garena.clone(), "adam_m": m._adam_m.clone(),
           "adam_v": m._adam_v.clone()}
    out.update({"sd." + k: v.clone() for k, v in m.state_dict().items()})
    return out


@pytest.mark.parametrize("kind", list(KINDS))
@pytest.mark.parametrize("twin", list(TWINS))
def test_train_step_on_an_awkward_twin_equals_the_step_on_its_contiguous_fp32_copy(twin, kind):
    head, n = KINDS[kind]
    base = _base(n)
    given = TWINS[twin](*base)
    plain = tuple(t.float().contiguous() for t in given)
    awkward = 0
    for g, p, b in zip(given, plain, base):
        assert torch.equal(p.reshape(b.shape), b), "the twin holds the values of the plain input"
        assert _owned_bytes(g) >= g.numel() * 4, "a twin owns at least the bytes of a contiguous fp32 tensor of its shape"
        awkward += int(g.dtype != torch.float32 or not g.is_contiguous() or g.dim() != b.dim())
    assert awkward >= 1, "the twin differs from a fresh contiguous fp32 tensor"
    ma, mb = _model(head), _model(head)
    assert ma._mlp_fused(n) == (kind == "fused-mlp-n10")
    got = _snapshot(ma, *ma.train_step(*given, lr=LR))
    want = _snapshot(mb, *mb.train_step(*plain, lr=LR))
    assert got.keys() == want.keys()
    for k in want:
        assert torch.equal(got[k], want[k]), f"{k}: the step on the {twin} twin differs from the step on its contiguous fp32 copy"
    assert torch.isfinite(want["loss"]).all() and want["grads"].abs().max().item() > 0


def test_contiguous_fp32_inputs_pass_through_without_a_copy(monkeypatch):
    """the normalisation is a no-op on what the captured graphs and the timed path hand over: forward_device receives the caller's own
    storage, and the fused MLP its labels"""
    a, v, y = _base(10)
    m = _model("regression")
    seen = {}
    real = m.forward_device

    def spy(audio, visual, save, **kw):
        seen["ptrs"] = (audio.data_ptr(), visual.data_ptr(), kw["fused_loss"][0].data_ptr())
        return real(audio, visual, save, **kw)
    monkeypatch.setattr(m, "forward_device", spy)
    m.train_step(a, v, y, lr=LR)
    torch.cuda.synchronize()
    assert seen["ptrs"] == (a.data_ptr(), v.data_ptr(), y.data_ptr())


def test_train_step_refuses_a_wrong_number_of_labels():
    a, v, y = _base(10)
    m = _model("regression")
    with pytest.raises(RuntimeError, match="labels must be a tensor of 10 elements"):
        m.train_step(a, v, y[:9], lr=LR)


# ---- wrapper checks: a bad argument never reaches the device -------------------------------------------------------------------------
class _NoLaunch:
    """stands in for the loaded library: size / predicate queries pass through, any other entry point fails the test — unless `allow`"""

    def __init__(self, real):
        self.real, self.allow, self.reached = real, False, []

    def __getattr__(self, name):
        fn = getattr(self.real, name)
        if name.endswith("_ws_bytes") or name.endswith("_ok") or name == "goalnet_last_error":
            return fn

        def entry(*args):
            self.reached.append(name)
            if not self.allow:
                pytest.fail(f"{name} was reached with a bad argument in play")
            return fn(*args)
        return entry


def _nan(*shape, dtype=torch.float32):
    return torch.full(shape, float("nan"), device=DEV, dtype=dtype)


def _strided(*shape):
    """a view with the right shape and a row stride 7 elements too long"""
    return torch.zeros(*shape[:-1], shape[-1] + 7, device=DEV)[..., :shape[-1]]


def test_wrappers_refuse_strided_and_float64_arguments_before_any_launch(monkeypatch):
    proxy = _NoLaunch(ops.lib())
    monkeypatch.setattr(ops, "lib", lambda: proxy)
    n, bins, l1 = 4, 30, 15
    z = lambda *s: torch.zeros(*s, device=DEV)                                 # noqa: E731
    x, w, b, y = z(n, 30, bins), z(64, 30, 3), z(64), _nan(n, 64, l1)
    dz, dx, dw, db = z(n, 64, l1), _nan(n, 30, bins), _nan(64, 30, 3), _nan(64)
    bad_x = (_strided(n, 30, bins), x.transpose(1, 2).contiguous().transpose(1, 2), x.double())
    calls = []
    for bx in bad_x:
        calls.append(lambda bx=bx: ops.conv1d_fwd(bx, w, b, y, True, n, 30, bins, 64))
        calls.append(lambda bx=bx: ops.conv1d_bwd(bx, dz, w, dx, dw, db, n, 30, bins, 64))
        calls.append(lambda bx=bx: ops.conv1d_bwd_small(bx, dz, y, w, dx, dw, db, n, 30, bins, 64))
    calls += [
        lambda: ops.conv1d_fwd(x, w.double(), b, y, True, n, 30, bins, 64),
        lambda: ops.conv1d_fwd(x, w, b, _strided(n, 64, l1), True, n, 30, bins, 64),
        lambda: ops.conv1d_bwd(x, dz.double(), w, dx, dw, db, n, 30, bins, 64),
        lambda: ops.conv1d_bwd(x, _strided(n, 64, l1), w, None, dw, db, n, 30, bins, 64),
        lambda: ops.conv1d_bwd(x, dz, w, _strided(n, 30, bins), dw, db, n, 30, bins, 64),
        lambda: ops.conv1d_bwd(x, dz, w, dx, dw, db.double(), n, 30, bins, 64),
        lambda: ops.conv1d_bwd_small(x, dz, y.double(), w, dx, dw, db, n, 30, bins, 64),
        lambda: ops.conv1d_bwd_small(x, _strided(n, 64, l1), y, w, dx, dw, db, n, 30, bins, 64),
        lambda: ops.conv1d_bwd_small(x, dz, y, w, dx.double(), dw, db, n, 30, bins, 64),
    ]
    # conv1 of VisBl: (N, 3, H, W) contiguous in, (N, Ho, Wo, 64) out
    h = wd = 7
    ho = (h + 3) // 3 + 1
    v, w1, b1, y1 = z(2, 3, h, wd), z(64, 27), z(64), _nan(2, ho, ho, 64)
    dy1, dw1, db1 = z(2, ho, ho, 64), _nan(64, 27), _nan(64)
    v_cl = z(2, 3, h, wd).contiguous(memory_format=torch.channels_last)
    assert not v_cl.is_contiguous()
    calls += [
        lambda: ops.conv1_fwd(v.double(), w1, b1, y1, 2, h, wd),
        lambda: ops.conv1_fwd(v_cl, w1, b1, y1, 2, h, wd),
        lambda: ops.conv1_fwd(v, w1, b1, y1.double(), 2, h, wd),
        lambda: ops.conv1_wgrad(v.double(), dy1, dw1, db1, 2, h, wd),
        lambda: ops.conv1_wgrad(v_cl, dy1, dw1, db1, 2, h, wd),
        lambda: ops.conv1_wgrad(v, dy1.double(), dw1, db1, 2, h, wd),
        lambda: ops.conv1_wgrad(v, _strided(2, ho, ho, 64), dw1, db1, 2, h, wd),
    ]
    # the two losses
    m = 6
    pred, lab, loss, dpred = z(m), torch.ones(m, device=DEV), _nan(1), _nan(m)
    table = torch.ones(m, 3, device=DEV)
    scores, dscores = torch.full((m, 5), 1.8, device=DEV), _nan(m, 5)
    calls += [
        lambda: ops.mse_bcast(pred, table[:, 0], loss, dpred),
        lambda: ops.mse_bcast(pred, lab.double(), loss, dpred),
        lambda: ops.mse_bcast(table[:, 1], lab, loss, dpred),
        lambda: ops.mse_bcast(pred, lab, loss, dpred.double()),
        lambda: ops.cross_entropy(scores, table[:, 0], loss, dscores),
        lambda: ops.cross_entropy(scores, lab.double(), loss, dscores),
        lambda: ops.cross_entropy(scores.double(), lab, loss, dscores),
        lambda: ops.cross_entropy(scores, lab, loss, _strided(m, 5)),
    ]
    for i, call in enumerate(calls):
        with pytest.raises(RuntimeError):
            call()
        assert not proxy.reached, f"bad call {i} reached {proxy.reached}"
    torch.cuda.synchronize()
    for t in (y, dx, dw, db, y1, dw1, db1, loss, dpred, dscores):
        assert torch.isnan(t).all(), "a refused call wrote nothing"
    # the proxy is not blind: the same wrappers with good arguments do reach their entry points through it
    proxy.allow = True
    ops.mse_bcast(pred, lab, loss, dpred)
    ops.conv1d_fwd(x, w, b, y, True, n, 30, bins, 64)
    torch.cuda.synchronize()
    assert proxy.reached == ["goalnet_mse_bcast", "goalnet_conv1d_fwd"] and torch.isfinite(loss).all() and torch.isfinite(y).all()
