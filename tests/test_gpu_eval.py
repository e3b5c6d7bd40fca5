"""GPU: `model.eval()` — BatchNorm on the running statistics (buffers untouched), no dropout, gradients through frozen statistics
(tests/eval_ref.py states the contract). Checked against the reference's own eval-mode fixtures (tests/golden/avm_eval_*.npz), the
fp64 restatement, and the existing kernels the new ones replace (csrc/pool_bn.hip: goalnet_pool_bn_eval_fwd,
goalnet_bn_bwd_finalize_eval, goalnet_bn_bwd_reduce_small_eval)."""
import warnings

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import _width_classes as WC  # noqa: E402
import eval_ref  # noqa: E402
from _golden import Golden  # noqa: E402
from cvml_goalnet_amd import AVM, ops, synth  # noqa: E402
from cvml_goalnet_amd.loop import VideoTrainer  # noqa: E402
from test_eval_golden import golden_buffers, head_of  # noqa: E402
from test_gpu_avm import NEAR_TIE, _is_reduction_grad, _weight_of, hip_taps, routing_disagreements  # noqa: E402

DEV = "cuda:0"
LR = 1e-3
BUFS = [f"visbl.bnorm{i}.{k}" for i in (1, 2, 3) for k in ("running_mean", "running_var", "num_batches_tracked")]


def params_of(h, audio, head="regression"):
    return eval_ref.classifier_params(h, audio) if head == "classifier" else synth.make_params(h, h, 30, audio)


def make_model(h, audio, head="regression", precision="fp32", bufs=None):
    m = AVM(audio_included=audio, device=DEV, seed=synth.BASE_SEED, head=head, precision=precision)
    sd = {k: torch.from_numpy(v) for k, v in params_of(h, audio, head).items()}
    sd.update(bufs if bufs is not None else eval_ref.running_stats())
    m.load_state_dict(sd)
    m.dropout_mode = "device"
    return m


def inputs(n, h, audio):
    vis = torch.from_numpy(synth.make_visual(n, h, h))
    aud = torch.from_numpy(synth.make_audio(n)) if audio else None
    return aud, vis, torch.from_numpy(synth.make_labels(n))


def buffers_of(m):
    sd = m.state_dict()
    return {k: sd[k].detach().cpu().clone() for k in BUFS}


class Counter:
    """counting wrapper around an ops function (proves which kernels a forward selected)"""

    def __init__(self, monkeypatch, name):
        self.calls, fn = 0, getattr(ops, name)

        def wrapped(*a, **k):
            self.calls += 1
            return fn(*a, **k)
        monkeypatch.setattr(ops, name, wrapped)


# ---- 1 + 7: the eval forward under no_grad against the reference's eval fixtures ---------------------------------------------
@pytest.mark.parametrize("case", ["avm_eval_a1_n10_h40", "avm_eval_a0_n7_h52", "avm_eval_a1_n2_h224", "avm_eval_cls_a1_n10_h40"])
def test_eval_forward_no_grad_matches_reference_eval_goldens(case):
    g = Golden(case)
    head = head_of(g)
    m = make_model(g.h, g.audio, head, bufs=golden_buffers(g))
    m.eval()
    aud, vis, _ = inputs(g.n, g.h, g.audio)
    before = buffers_of(m)
    drop0 = m._drop_step
    with torch.no_grad():
        out = m(aud, vis)
    torch.cuda.synchronize()
    g.check("s0.pred", out if head == "classifier" else out.view(-1, 1), rtol=0.0, atol=2e-5)
    g.check("s0.act.logit", m.last_logit, rtol=0.0, atol=2e-5)
    after = buffers_of(m)
    for k in BUFS:
        assert torch.equal(before[k], after[k]), f"{k} changed under eval()"
    assert int(after["visbl.bnorm1.num_batches_tracked"]) == 7
    assert m._drop_step == drop0 and (m._state is None or int(m._state[1]) == drop0)


# ---- 2: gradients through frozen statistics: autograd + stock Adam, the fused optimizer, and train_step --------------------
def _rerouted(g, aud, vis):
    """max-pool windows the device routes differently from ATen's fp32 forward (test_gpu_avm.routing_disagreements): each must be
    a near-tie; the gradients of the layers in front of such a window then carry one element at O(1) of its share."""
    m = make_model(g.h, g.audio, bufs=golden_buffers(g))
    m.eval()
    _, ctx = m.forward_device(aud.to(DEV) if aud is not None else None, vis.to(DEV), save=True)
    torch.cuda.synchronize()
    inter = {}
    with torch.no_grad():
        eval_ref.forward({k: torch.from_numpy(v) for k, v in params_of(g.h, g.audio).items()}, golden_buffers(g), aud, vis,
                         g.audio, inter=inter)
    nd, worst = routing_disagreements(inter, hip_taps(ctx))
    print(f"[parity] eval: {nd} max-pool windows routed differently from ATen; largest top-2 gap {worst:.2e} of max|y|")
    assert worst <= NEAR_TIE, "max-pool argmax differs from ATen's where the window is NOT a near-tie"
    return nd


def _check_grads_and_adam(g, m, what, rerouted):
    failures = []
    slack = {}
    for k in g.keys("s0.grad."):
        name = k.split("grad.", 1)[1]
        mine = g.flat(m.grad_of(name))
        idx, ref = g.samples(k)
        scale = max(g.absmax(k), 1e-30)
        err = np.abs(mine[idx] - ref)
        floor = 2e-5 * g.absmax("s0.grad." + _weight_of(name)) if _is_reduction_grad(name) else 0.0
        # a near-tie routed the other way (asserted by _rerouted) moves the conv layers' gradients by ~1e-3 of their scale
        rt = 2e-3 if (rerouted and ".conv" in name and name.startswith("visbl.")) else 1e-4
        if err.max() > rt * scale + floor:
            failures.append(f"{what} {k}: err {err.max():.3e} > {rt * scale + floor:.3e}")
        slack[name] = LR * np.minimum(2.0, 8.0 * err / (np.abs(ref) + 1e-8))
    sd = m.state_dict()
    for k in g.keys("s0.param."):
        name = k.split("param.", 1)[1]
        idx, ref = g.samples(k)
        err = np.abs(g.flat(sd[name])[idx] - ref)
        tol = 2e-6 + slack[name]
        if (err > tol).any():
            failures.append(f"{what} {k} (after Adam): err {err.max():.3e}")
    assert not failures, "\n".join(failures)


@pytest.mark.parametrize("path", ["stock_adam", "fused_adam", "train_step"])
def test_eval_backward_and_adam_match_reference_eval_goldens(path):
    g = Golden("avm_eval_a1_n10_h40")
    m = make_model(g.h, g.audio, bufs=golden_buffers(g))
    opt = torch.optim.Adam(m.parameters(), lr=LR) if path == "stock_adam" else m.make_optimizer(lr=LR)
    m.eval()
    aud, vis, lab = inputs(g.n, g.h, g.audio)
    before = buffers_of(m)
    if path == "train_step":
        loss, pred = m.train_step(aud.to(DEV), vis.to(DEV), lab.to(DEV), lr=LR)
    else:
        opt.zero_grad()
        with warnings.catch_warnings():
            warnings.simplefilter("ignore")
            pred = m(aud, vis)
            loss = torch.nn.MSELoss()(pred, lab)
        assert pred.requires_grad
        loss.backward()
        opt.step()
    torch.cuda.synchronize()
    g.check("s0.pred", pred.detach().view(-1, 1), rtol=0.0, atol=2e-5)
    g.check("s0.loss", loss.detach().reshape(1), rtol=2e-5)
    _check_grads_and_adam(g, m, path, _rerouted(g, aud, vis))
    after = buffers_of(m)
    for k in BUFS:
        assert torch.equal(before[k], after[k]), f"{k} changed under eval()"


# ---- 3: train -> eval -> train is bit-identical to train -> train; the dropout counter does not move in eval mode --------------
def test_train_eval_train_toggle_is_bit_exact():
    n, h = 10, 40
    aud, vis, lab = inputs(n, h, True)
    a, v, y = aud.to(DEV), vis.to(DEV), lab.to(DEV)
    ref, tog = make_model(h, True), make_model(h, True)
    outs = {}
    for name, m in (("ref", ref), ("tog", tog)):
        l0, p0 = m.train_step(a, v, y, lr=LR)
        if name == "tog":
            m.eval()
            d0, s0 = m._drop_step, int(m._state[1])
            b0 = buffers_of(m)
            with torch.no_grad():
                for _ in range(3):
                    m(aud, vis)
            m(aud, vis).sum().backward()                      # with grad too: the backward writes only the gradient arena
            assert m._drop_step == d0 and int(m._state[1]) == s0
            for k, t in buffers_of(m).items():
                assert torch.equal(t, b0[k]), k
            m.train()
        l1, p1 = m.train_step(a, v, y, lr=LR)
        torch.cuda.synchronize()
        outs[name] = (l0, p0, l1, p1)
    for x, z in zip(outs["ref"], outs["tog"]):
        assert torch.equal(x, z)
    assert torch.equal(ref._arena, tog._arena)
    assert torch.equal(ref._adam_m, tog._adam_m) and torch.equal(ref._adam_v, tog._adam_v)
    sr, st = ref.state_dict(), tog.state_dict()
    for k in BUFS:
        assert torch.equal(sr[k], st[k]), k
    assert ref._state.tolist() == tog._state.tolist() and ref._drop_step == tog._drop_step == 2


# ---- 4: every precision against the fp64 restatement, at shapes where the eval kernels are the selected ones -----------------
CRIT = {"fp32": 2e-5, "bf16x6": 2e-5, "fp16x3": 2e-5, "bf16": 1e-3, "fp16": 2.5e-4}   # max |logit error| (16-bit: test_gpu_avm / _fp16)


@pytest.mark.parametrize("precision", ["bf16", "fp16", "bf16x6", "fp16x3"])
@pytest.mark.parametrize("n", [10, 32])
def test_eval_forward_per_precision_vs_fp64(precision, n, monkeypatch):
    h = 40
    m = make_model(h, True, precision=precision)
    m.eval()
    pool = Counter(monkeypatch, "pool_bn_eval_fwd")
    stats = Counter(monkeypatch, "pool_bnstats_fwd")
    aud, vis, _ = inputs(n, h, True)
    with torch.no_grad():
        out = m(aud, vis)
    torch.cuda.synchronize()
    assert pool.calls == 3 and stats.calls == 0
    inter = {}
    p64 = {k: torch.from_numpy(v).double() for k, v in params_of(h, True).items()}
    ref = eval_ref.forward(p64, eval_ref.running_stats(), aud, vis, True, inter=inter)
    e = (m.last_logit.cpu().double() - inter["logit"].view(-1)).abs().max().item()
    print(f"[parity] eval {precision} n={n}: logit error vs fp64 {e:.2e}")
    assert e <= CRIT[precision]
    assert (out.cpu().double() - ref).abs().max().item() <= 4 * CRIT[precision]


def test_eval_grads_bf16_large_path_vs_fp64():
    """n > 16 under precision="bf16": bf16 p2 / p3, the bf16 linear5 operand, the fused bf16 BatchNorm / pool backward"""
    n, h = 32, 40
    m = make_model(h, True, precision="bf16")
    m.eval()
    aud, vis, lab = inputs(n, h, True)
    m.train_step(aud.to(DEV), vis.to(DEV), lab.to(DEV), lr=0.0)
    torch.cuda.synchronize()
    p64 = {k: torch.from_numpy(v).double().requires_grad_(True) for k, v in params_of(h, True).items()}
    eval_ref.loss_of(eval_ref.forward(p64, eval_ref.running_stats(), aud, vis, True), lab).backward()
    for k, t in p64.items():
        if _is_reduction_grad(k):
            continue
        mine = m.grad_of(k).cpu().double().reshape(t.shape)
        l2 = ((mine - t.grad).norm() / t.grad.norm().clamp_min(1e-30)).item()
        # not under the device's max-pool routing / ReLU gates (test_gpu_bench_shapes does that): gate flips under bf16 activation
        # noise alone reach ~1e-1, arithmetic errors would be far beyond
        assert l2 <= 0.15, f"{k}: relative L2 {l2:.3f}"


# ---- 5: kernel units against the existing kernels -----------------------------------------------------------------------------
def _tied(shape, gen):
    """values on a coarse grid (exact ties in most pooling windows), some negative (the ReLU'd conv output has none, but the
    kernels must follow ATen's comparisons anyway)"""
    return (torch.randint(-2, 6, shape, generator=gen).float() * 0.25)


@pytest.mark.parametrize("c,wc,kind", [(64, 14, "f32"), (256, 37, "f32"), (512, 12, "f32"), (64, 170, "f32"), (64, 200, "f32"),
                                       (256, 37, "bf16"), (512, 20, "fp16"), (256, 23, "bf16_y16"), (64, 170, "fp16_y16"),
                                       *WC.EVAL_FWD_ROWS])
def test_pool_bn_eval_fwd_equals_pool_bnstats_fwd(c, wc, kind):
    n, hc = 2, 9
    gen = torch.Generator().manual_seed(c + wc)
    y = _tied((n, hc, wc, c), gen).to(DEV)
    h16 = torch.float16 if "fp16" in kind else torch.bfloat16
    pt = torch.float32 if kind == "f32" else h16
    if kind.endswith("_y16"):
        y = y.to(h16)
    gamma = (torch.rand(c, generator=gen) * 2 - 1).to(DEV)                  # negative gammas included
    beta = torch.randn(c, generator=gen).to(DEV)
    rm = (torch.rand(c, generator=gen) * 3 - 1.5).to(DEV)
    rv = (torch.rand(c, generator=gen) * 3.75 + 0.25).to(DEV)
    rm0, rv0 = rm.clone(), rv.clone()
    hp, wp = hc - 2, wc - 2
    p_ref = torch.empty(n, hp, wp, c, dtype=pt, device=DEV); i_ref = torch.empty(n, hp, wp, c, dtype=torch.uint8, device=DEV)
    parts = torch.empty(ops.stat_parts(8 * n) * 2 * c, dtype=torch.float64, device=DEV)
    ops.pool_bnstats_fwd(y, p_ref, i_ref, parts, n, hc, wc, c)
    p = torch.full_like(p_ref, 7.0); idx = torch.full_like(i_ref, 0xAB)
    st = torch.full((4, c), 9.0, device=DEV)
    ops.pool_bn_eval_fwd(y, p, idx, gamma, beta, rm, rv, eval_ref.BN_EPS, st, n, hc, wc, c)
    p2 = torch.full_like(p_ref, 7.0)
    ops.pool_bn_eval_fwd(y, p2, None, gamma, beta, rm, rv, eval_ref.BN_EPS, torch.empty(4, c, device=DEV), n, hc, wc, c)
    torch.cuda.synchronize()
    assert torch.equal(p.view(torch.int16) if pt != torch.float32 else p, p_ref.view(torch.int16) if pt != torch.float32 else p_ref)
    assert torch.equal(idx, i_ref) and torch.equal(p2.float(), p_ref.float())
    assert torch.equal(rm, rm0) and torch.equal(rv, rv0)
    inv = 1.0 / torch.sqrt(rv0.double() + eval_ref.BN_EPS)
    want = torch.stack([rm0.double(), inv, gamma.double() * inv, beta.double() - rm0.double() * gamma.double() * inv])
    assert (st.double() - want).abs().max().item() <= 1e-6 * max(1.0, want.abs().max().item())
    # the 16-bit operand the eval forward feeds conv3 / linear5: fmaf(p, scale, shift) rounded, as the existing cast kernels compute it
    if pt != torch.float32 and c % 32 == 0:
        xb = ops.bn_apply_bf16(p, st[2], st[3], torch.empty(p.shape, dtype=h16, device=DEV), c)
        want16 = torch.addcmul(st[3].view(1, 1, 1, c), p.float(), st[2].view(1, 1, 1, c)).to(h16)
        torch.cuda.synchronize()
        assert (xb.float() - want16.float()).abs().max().item() <= 2 ** -7 * want16.float().abs().max().item()


@pytest.mark.parametrize("c,small", [(64, True), (256, False), (512, False), (256, True)])
def test_bn_bwd_eval_finalize_vs_fp64(c, small):
    n, hc, wc = 2, 12, 12
    gen = torch.Generator().manual_seed(c)
    npix = n * (hc - 2) * (wc - 2)
    dz = torch.randn(n, hc - 2, wc - 2, c, generator=gen).to(DEV)
    p = torch.rand(n, hc - 2, wc - 2, c, generator=gen).to(DEV) * 3
    gamma = (torch.rand(c, generator=gen) * 2 - 1).to(DEV)
    mean = (torch.rand(c, generator=gen) * 2 - 1).to(DEV)
    invstd = (torch.rand(c, generator=gen) + 0.5).to(DEV)
    dgamma, dbeta, coef3 = torch.empty(c, device=DEV), torch.empty(c, device=DEV), torch.full((3 * c,), 5.0, device=DEV)
    if small:
        ops.bn_bwd_reduce_small_eval(dz, p, mean, invstd, gamma, dgamma, dbeta, coef3, n, hc, wc, c)
    else:
        parts = torch.empty(ops.stat_parts(npix // 64) * 2 * c, dtype=torch.float64, device=DEV)
        ops.bn_bwd_reduce(dz, p, mean, invstd, parts, npix, c)
        ops.bn_bwd_finalize_eval(parts, gamma, invstd, c, dgamma, dbeta, coef3)
    torch.cuda.synchronize()
    d, x = dz.cpu().double().reshape(-1, c), p.cpu().double().reshape(-1, c)
    xhat = (x - mean.cpu().double()) * invstd.cpu().double()
    assert torch.allclose(dbeta.cpu().double(), d.sum(0), rtol=1e-5, atol=1e-4)
    assert torch.allclose(dgamma.cpu().double(), (d * xhat).sum(0), rtol=1e-5, atol=1e-4)
    a = gamma.cpu().double() * invstd.cpu().double()
    assert torch.allclose(coef3[:c].cpu().double(), a, rtol=1e-6, atol=0)
    assert torch.count_nonzero(coef3[c:]).item() == 0


# ---- 6: VideoTrainer: graphs keyed on the mode; eval_video follows the model's mode ------------------------------------------
@pytest.mark.parametrize("precision", ["fp32", "bf16", "fp16"])
def test_video_trainer_in_eval_mode_equals_eager_eval_steps(precision):
    n, h = 23, 40
    vid = [(torch.from_numpy(synth.make_audio(n, seed=synth.BASE_SEED + s)),
            torch.from_numpy(synth.make_visual(n, h, h, seed=synth.BASE_SEED + s)),
            torch.from_numpy(synth.make_labels(n, seed=synth.BASE_SEED + s))) for s in (1, 2)]
    eager, graphed = make_model(h, True, precision=precision), make_model(h, True, precision=precision)
    tr = VideoTrainer(graphed, subbatch_size=10, lr=LR)

    def eager_video(aud, vis, lab):
        ls, ps = [], []
        for a in range(0, n, 10):
            b = min(a + 10, n)
            loss, pred = eager.train_step(aud[a:b].to(DEV), vis[a:b].to(DEV), lab[a:b].to(DEV), lr=LR)
            ls.append(loss); ps.append(pred)
        return torch.cat(ls), torch.cat(ps)

    for _ in range(2):                                        # train mode: sizes 10 and 3 are captured on their second occurrence
        el, ep = eager_video(*vid[0])
        gl, gp = tr.train_video(*vid[0])
        assert torch.equal(el, gl) and torch.equal(ep, gp)
    train_keys = set(tr._graphs)
    assert train_keys and all(k[-1] is True for k in train_keys)
    eager.eval(); graphed.eval()
    # eval_video: the running-statistics forward of the trained model, against the fp64 restatement on its own state
    loss, pred = tr.eval_video(*vid[1])
    sd = graphed.state_dict()
    p64 = {k: v.cpu().double() for k, v in sd.items() if k not in BUFS}
    ref = eval_ref.forward(p64, {k: sd[k].cpu() for k in BUFS}, vid[1][0], vid[1][1], True)
    # |d pred| <= |d logit| (4 sigmoid' <= 1): the logit criterion of the precision bounds the prediction (fp32: 2e-5, as ever)
    assert (pred.cpu().double().view(-1, 1) - ref).abs().max().item() < CRIT[precision]
    b0 = buffers_of(graphed)
    replays0 = tr.replays
    for _ in range(2):                                        # eval mode: new graphs, never the train-mode ones
        el, ep = eager_video(*vid[1])
        gl, gp = tr.train_video(*vid[1])
        torch.cuda.synchronize()
        assert torch.equal(el, gl) and torch.equal(ep, gp)
    assert tr.replays > replays0
    assert {k for k in tr._graphs if k[-1] is False}, "no eval-mode graph was captured"
    se, sg = eager.state_dict(), graphed.state_dict()
    for k in se:
        assert torch.equal(se[k], sg[k]), k
    for k, t in buffers_of(graphed).items():
        assert torch.equal(t, b0[k]), k
    assert graphed._drop_step == eager._drop_step
