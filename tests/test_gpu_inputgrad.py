"""GPU, model level: gradients with respect to the INPUTS — `visual.requires_grad_(); model(a, visual).sum().backward()` as with the
reference, AVM.input_gradients and AVM.saliency.

fp32 against the reference's golden vectors (tests/golden/avm_inputgrad_*.npz, written from utils.AVM by make_golden_inputgrad.py: the
gradient of sum_i w_i pred_i, w = linspace(0.5, 1.5, N)) through the autograd surface with CPU leaf tensors, under
tests/test_gpu_avm.py's routing policy: the golden samples are compared only when the device's max-pool taps agree with ATen's;
otherwise (and in any case) the live oracle runs under the device's taps, and every window routed differently must be a near-tie
(NEAR_TIE). Bound: the project's gradient criterion, <= 1e-4 max|g|. The sharp check has the form of
test_gpu_avm.py::test_gradients_within_reference_rounding_of_fp64_truth. Then the composition properties: parameter gradients
unchanged by the inputs' gradients, the inputs-only backward bit-equal to autograd's and leaving the arena alone, per-frame
attribution under eval(), saliency = abs().amax(1), CPU and GPU leaves alike. The other precisions / heads: one cell each of
tests/_inputgrad_case.py."""
import functools

import pytest
import torch

pytestmark = pytest.mark.gpu

import eval_ref  # noqa: E402
import _inputgrad_case as IC  # noqa: E402
from _abi_guard import bits_equal  # noqa: E402
from _golden import Golden  # noqa: E402
from _mode_case import cell_id, fixture_of  # noqa: E402
from cvml_goalnet_amd import AVM, ops, synth  # noqa: E402
from oracle import avm_ref  # noqa: E402
from test_gpu_avm import NEAR_TIE, hip_taps, routing_disagreements  # noqa: E402
from test_gpu_bench_shapes import F32_FACTOR  # noqa: E402

DEV = "cuda:0"
CASES = ["avm_inputgrad_a1_n3_h40", "avm_inputgrad_eval_a1_n3_h40", "avm_inputgrad_a0_n2_h41"]


def _model(h, audio, evalmode):
    m = AVM(audio_included=audio, device=DEV, seed=synth.BASE_SEED)
    sd = {k: torch.from_numpy(v) for k, v in synth.make_params(h, h, 30, audio).items()}
    sd.update(eval_ref.running_stats() if evalmode else avm_ref.init_buffers())
    m.load_state_dict(sd)
    m.dropout_mode = "off"                       # the fixtures were written with dropout p = 0
    if evalmode:
        m.eval()
    return m


def _saved_of(out):
    """the context _AVMFunction saved for this output (behind the copy to the inputs' device)"""
    node = out.grad_fn
    while node is not None and not hasattr(node, "saved"):
        node = node.next_functions[0][0]
    assert node is not None and node.saved is not None
    return node.saved


@functools.lru_cache(maxsize=None)
def _golden_run(case):
    """the reference's call sequence on CPU leaves, once per case: everything the tests below compare, as CPU tensors"""
    g = Golden(case)
    evalmode = bool(g.z["meta|eval"][0])
    m = _model(g.h, g.audio, evalmode)
    vis = torch.from_numpy(synth.make_visual(g.n, g.h, g.h)).requires_grad_()
    aud = torch.from_numpy(synth.make_audio(g.n)).requires_grad_() if g.audio else [None] * g.n
    w = torch.linspace(0.5, 1.5, g.n)
    out = m(aud, vis)
    assert out.device.type == "cpu" and out.shape == (g.n, 1) and out.requires_grad
    taps = hip_taps(_saved_of(out))
    (out.view(-1) * w).sum().backward()
    assert vis.grad is not None and vis.grad.device.type == "cpu" and vis.grad.shape == vis.shape and vis.grad.dtype == torch.float32
    if g.audio:
        assert aud.grad is not None and aud.grad.device.type == "cpu" and aud.grad.shape == aud.shape
    return {"g": g, "eval": evalmode, "w": w, "taps": taps, "pred": out.detach(), "d_vis": vis.grad, "d_aud": aud.grad if g.audio else None}


def _oracle(r, dtype, taps, inter=None):
    g = r["g"]
    p = {k: torch.from_numpy(v).to(dtype) for k, v in synth.make_params(g.h, g.h, 30, g.audio).items()}
    b = eval_ref.running_stats() if r["eval"] else avm_ref.init_buffers()
    b = {k: (v.to(dtype) if v.is_floating_point() else v.clone()) for k, v in b.items()}
    vis = torch.from_numpy(synth.make_visual(g.n, g.h, g.h)).to(dtype).requires_grad_()
    aud = torch.from_numpy(synth.make_audio(g.n)).to(dtype).requires_grad_() if g.audio else None
    pred = avm_ref.forward(p, b, aud, vis, None, g.audio, inter, pool_taps=taps, training=not r["eval"])
    (pred.view(-1) * r["w"].to(dtype)).sum().backward()
    return pred.detach(), vis.grad, None if aud is None else aud.grad


@pytest.mark.parametrize("case", CASES)
def test_autograd_input_gradients_match_reference_goldens(case):
    r = _golden_run(case)
    g = r["g"]
    inter = {}
    _oracle(r, torch.float32, None, inter)
    nd, worst = routing_disagreements(inter, r["taps"])
    del inter
    if nd:
        print(f"[inputgrad] {case}: {nd} max-pool windows routed differently from ATen; largest top-2 gap {worst:.2e} of max|y|")
        assert worst <= NEAR_TIE, "max-pool argmax differs from ATen's where the window is NOT a near-tie"
    else:
        # (a) the reference's golden vectors: valid while the routing decisions agree with the reference's
        e = [g.check("s0.pred", r["pred"], rtol=0.0, atol=2e-5), g.check("s0.igrad.visual", r["d_vis"], rtol=1e-4)]
        if g.audio:
            e.append(g.check("s0.igrad.audio", r["d_aud"], rtol=1e-4))
        print(f"[inputgrad] {case}: vs the golden samples (of max|ref|): pred {e[0]:.2e}, d_visual {e[1]:.2e}" + (f", d_audio {e[2]:.2e}" if g.audio else ""))
    # (b) the live oracle under the device's routing decisions: every element
    o_pred, o_vis, o_aud = _oracle(r, torch.float32, r["taps"] if nd else None)
    assert (r["pred"] - o_pred).abs().max().item() < 2e-5
    for name, mine, og in (("d_visual", r["d_vis"], o_vis), ("d_audio", r["d_aud"], o_aud)):
        if og is None:
            continue
        scale = og.abs().max().item()
        err = (mine - og).abs().max().item()
        print(f"[inputgrad] {case}: {name} vs the live oracle {err / scale:.2e} of max|g| {scale:.3e}")
        assert err <= 1e-4 * scale, f"{name}: {err:.3e} > 1e-4 x {scale:.3e}"
    assert bool((r["d_vis"] != 0).all()), "every pixel belongs to exactly one window: none is without a gradient"


@pytest.mark.parametrize("case", CASES)
def test_input_gradients_within_reference_rounding_of_fp64_truth(case):
    """the input gradients are as close to the fp64 oracle (under the device's max-pool routing) as the reference's own fp32
    arithmetic is (x F32_FACTOR["fp32"]), or within 2e-6 of their magnitude. e_ref was 3.4e-7 .. 7.2e-7 of max|g| on the CPU."""
    r = _golden_run(case)
    inter64 = {}
    p64, v64, a64 = _oracle(r, torch.float64, r["taps"], inter64)
    nd, worst = routing_disagreements(inter64, r["taps"])
    del inter64
    print(f"[inputgrad] {case} fp64 truth: {nd} windows routed differently from the fp64 argmax (largest gap {worst:.2e} of max|y|)")
    assert worst <= NEAR_TIE
    p32, v32, a32 = _oracle(r, torch.float32, r["taps"])
    e_ref, e_hip = (p32.double() - p64).abs().max().item(), (r["pred"].double() - p64).abs().max().item()
    print(f"[inputgrad] {case} fp64 truth: pred error reference-fp32 {e_ref:.2e}, HIP {e_hip:.2e}")
    assert e_hip <= max(F32_FACTOR["fp32"] * e_ref, 2e-6)
    bad = []
    for name, mine, g32, g64 in (("d_visual", r["d_vis"], v32, v64), ("d_audio", r["d_aud"], a32, a64)):
        if g64 is None:
            continue
        scale = g64.abs().max().item()
        e_ref = (g32.double() - g64).abs().max().item()
        e_hip = (mine.double() - g64).abs().max().item()
        print(f"[inputgrad] {case} fp64 truth: {name:9s} max|g| {scale:.2e}  e_ref {e_ref:.2e} ({e_ref / scale:.2e})  e_hip {e_hip:.2e} ({e_hip / scale:.2e})")
        if not e_hip <= max(F32_FACTOR["fp32"] * e_ref, 2e-6 * scale):
            bad.append(name)
    assert not bad, f"HIP input gradients further from the fp64 truth than the reference's fp32 path: {bad}"


# ---- composition ----------------------------------------------------------------------------------------------------------------------
N, H = 3, 40


def _inputs(n=N, h=H, dev=DEV):
    return torch.from_numpy(synth.make_audio(n)).to(dev), torch.from_numpy(synth.make_visual(n, h, h)).to(dev)


def _param_grads(m):
    return {s.name: m.grad_of(s.name).clone() for s in m._specs}


@pytest.mark.parametrize("evalmode", [False, True], ids=["train", "eval"])
def test_one_backward_gives_both_and_parameter_gradients_are_unchanged(evalmode):
    m = _model(H, True, evalmode)
    w = torch.linspace(0.5, 1.5, N, device=DEV)
    aud, vis = _inputs()
    (m(aud, vis).view(-1) * w).sum().backward()
    plain = _param_grads(m)
    m2 = _model(H, True, evalmode)
    a2, v2 = aud.clone().requires_grad_(), vis.clone().requires_grad_()
    out = m2(a2, v2)
    (out.view(-1) * w).sum().backward()
    assert v2.grad is not None and v2.grad.is_cuda and v2.grad.shape == vis.shape and a2.grad.shape == aud.shape
    both = _param_grads(m2)
    for k in plain:
        assert bits_equal(plain[k], both[k]), f"{k}: parameter gradient changed when the inputs asked for theirs"
    assert all(getattr(*m2._module_of(s.name)).grad is not None for s in m2._specs), "one backward gives both"
    # autograd accumulates: a second backward through a fresh forward doubles .grad (x + x is exact)
    first = v2.grad.clone()
    m3 = _model(H, True, evalmode)
    (m3(a2, v2).view(-1) * w).sum().backward()
    assert bits_equal(v2.grad, first + first)
    # torch.autograd.grad on the inputs alone
    m4 = _model(H, True, evalmode)
    v4 = vis.clone().requires_grad_()
    (gv,) = torch.autograd.grad((m4(aud, v4).view(-1) * w).sum(), v4)
    assert bits_equal(gv, first) and v4.grad is None


@pytest.mark.parametrize("evalmode", [False, True], ids=["train", "eval"])
def test_input_gradients_equal_autograd_and_leave_every_parameter_gradient_alone(evalmode, monkeypatch):
    w = torch.linspace(0.5, 1.5, N, device=DEV)
    aud, vis = _inputs()
    m = _model(H, True, evalmode)
    a1, v1 = aud.clone().requires_grad_(), vis.clone().requires_grad_()
    calls = []
    spied = [k for k in vars(ops) if ("wgrad" in k or "_bwd_dw" in k) and callable(getattr(ops, k)) and not k.endswith(("_ok", "_bytes"))]
    assert {"conv1_wgrad", "conv3x3_wgrad", "linear_bwd_dw"} <= set(spied)
    for k in spied:
        monkeypatch.setattr(ops, k, (lambda f, k: lambda *a, **kw: (calls.append(k), f(*a, **kw))[1])(getattr(ops, k), k))
    (m(a1, v1).view(-1) * w).sum().backward()
    assert {"conv1_wgrad", "conv3x3_wgrad", "linear_bwd_dw"} <= set(calls), "the spy sees the weight-gradient launches of a full backward"
    # sentinel in the arena and in every .grad
    m2 = _model(H, True, evalmode)
    m2._ensure_garena()
    m2._garena.copy_(torch.arange(m2._garena.numel(), device=DEV, dtype=torch.float32).mul_(1e-3).sin_())
    arena0 = m2._garena.clone()
    grads0 = {}
    for s in m2._specs:
        prm = getattr(*m2._module_of(s.name))
        prm.grad = torch.full_like(prm, 0.5 + 0.001 * len(grads0))
        grads0[s.name] = prm.grad.clone()
    del calls[:]
    d_aud, d_vis = m2.input_gradients(aud, vis, w)
    torch.cuda.synchronize()
    assert calls == [], f"the inputs-only backward issued weight-gradient launches: {calls}"
    assert bits_equal(m2._garena, arena0), "the gradient arena was written"
    for s in m2._specs:
        assert bits_equal(getattr(*m2._module_of(s.name)).grad, grads0[s.name]), f"{s.name}.grad was written"
    assert d_vis.is_cuda and d_vis.shape == vis.shape and d_aud.shape == aud.shape
    assert bits_equal(d_vis, v1.grad) and bits_equal(d_aud, a1.grad), "input_gradients differs from the autograd path"
    # weights default to ones
    m3 = _model(H, True, evalmode)
    v3 = vis.clone().requires_grad_()
    m3(aud, v3).sum().backward()
    m4 = _model(H, True, evalmode)
    assert bits_equal(m4.input_gradients(aud, vis)[1], v3.grad)


def test_eval_mode_attributes_each_frame_to_itself_and_saliency_is_absmax():
    m = _model(H, True, True)
    aud, vis = _inputs()
    e0 = torch.zeros(N, device=DEV)
    e0[0] = 1.0
    d_aud, d_vis = m.input_gradients(aud, vis, e0)
    assert bool((d_vis[0] != 0).all()) and bool((d_aud[0] != 0).any())
    assert bool((d_vis[1:] == 0).all()) and bool((d_aud[1:] == 0).all()), "eval(): d out[0] / d frame[1:] is exactly 0"
    w = torch.linspace(0.5, 1.5, N, device=DEV)
    d_aud, d_vis = m.input_gradients(aud, vis, w)
    a_map, v_map = m.saliency(aud, vis, w)
    assert v_map.shape == (N, H, H) and bits_equal(v_map, d_vis.abs().amax(1))
    assert bits_equal(a_map, d_aud.abs())
    a_raw, v_raw = m.saliency(aud, vis, w, reduce="none")
    assert bits_equal(v_raw, d_vis) and bits_equal(a_raw, d_aud.abs())
    with pytest.raises(RuntimeError):
        m.input_gradients(aud, vis, torch.ones(N + 1, device=DEV))
    # train mode couples the frames through BatchNorm (the docstring's warning)
    mt = _model(H, True, False)
    assert bool((mt.input_gradients(aud, vis, e0)[1][1:] != 0).any())


def test_cpu_leaves_and_gpu_leaves_give_the_same_gradients():
    w = torch.linspace(0.5, 1.5, N)
    got = []
    for dev in ("cpu", DEV):
        m = _model(H, True, True)
        aud, vis = _inputs(dev=dev)
        aud.requires_grad_(), vis.requires_grad_()
        out = m(aud, vis)
        assert out.device == vis.device
        (out.view(-1) * w.to(dev)).sum().backward()
        assert vis.grad.device == vis.device and aud.grad.device == aud.device
        got.append((aud.grad.cpu(), vis.grad.cpu()))
    assert bits_equal(got[0][0], got[1][0]) and bits_equal(got[0][1], got[1][1])


def test_float64_leaf_gets_a_float64_gradient():
    m = _model(H, True, True)
    aud, vis = _inputs(dev="cpu")
    v64 = vis.double().requires_grad_()
    m(aud, v64).sum().backward()
    assert v64.grad.dtype == torch.float64 and v64.grad.shape == vis.shape


# ---- the other modes: one cell each ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cell", IC.CELLS + IC.SHAPE_CELLS, ids=cell_id)
def test_input_gradients_of_the_other_modes(cell):
    fx = fixture_of(cell)
    w = IC.weights_of(cell)
    dev, m = IC.run_device(cell, fx, w)
    assert dev["d_vis"].shape == (cell.n, 3, *cell.hw)
    IC.compare(cell, fx, dev, w)
    # the autograd surface of the same cell gives the same bits (fp16: the loss scale divided back out on both paths)
    m2 = IC.make_model(cell, fx)
    vis = fx["vis"].to(DEV).requires_grad_()
    aud = None if fx["aud"] is None else fx["aud"].to(DEV).requires_grad_()
    out = m2(aud if cell.audio else [None] * cell.n, vis)
    (out * w.to(DEV).reshape(cell.n, -1)).sum().backward()
    assert bits_equal(vis.grad.cpu(), dev["d_vis"]) and (aud is None or bits_equal(aud.grad.cpu(), dev["d_aud"]))
    for s in m2._specs:
        assert torch.isfinite(m2.grad_of(s.name)).all(), f"{s.name}: the parameter gradients of the same backward are finite (unscaled)"
