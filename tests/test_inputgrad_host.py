"""CPU: input gradients (csrc/conv1.hip goalnet_conv1_dgrad, AVM.input_gradients / AVM.saliency) — what can be pinned without a GPU.

  * the argument contract of goalnet_conv1_dgrad, which returns before any launch (no GPU is needed and none is touched);
  * the golden fixtures tests/golden/avm_inputgrad_*.npz (written from the reference by tests/golden/make_golden_inputgrad.py)
    re-checked against oracle/avm_ref.forward under CPU autograd, as tests/test_oracle_golden.py does for the parameter gradients;
  * the index formula in the kernel's header (stride = kernel = 3: one window and one tap per pixel) against autograd of F.conv2d;
  * the two properties the API's docstrings lean on: every pixel has a gradient, and per-frame attribution holds in eval mode only.
"""
import pytest
import torch
import torch.nn.functional as F

import eval_ref
import test_abi_contract_host as C
from _golden import Golden
from cvml_goalnet_amd import _lib, synth
from oracle import avm_ref

INPUTGRAD_CASES = ["avm_inputgrad_a1_n3_h40", "avm_inputgrad_eval_a1_n3_h40", "avm_inputgrad_a0_n2_h41"]

# goalnet_conv1_dgrad joins the table of tests/test_abi_contract_host.py (the pattern of tests/test_rankcorr_host.py): one valid call
# with fake addresses and the mutations that must be refused. That file's rows became test cases when it was collected, so this row's
# mutations run below, through that file's own helpers.
# arguments: 0 dy_nhwc, 1 w_ohwi, 2 out, 3 reduce, 4 N, 5 H, 6 W, 7 stream
C.ROWS.setdefault("goalnet_conv1_dgrad", C.auto(
    "goalnet_conv1_dgrad", {3: 0, 4: 2, 5: 40, 6: 41},
    shape=[(3, 2), (3, -1), (4, 0), (5, 0), (6, -3)], align=[(0, 4), (0, 8)],
    extra=[({4: 1 << 22, 5: 224, 6: 224}, C.E_SHAPE)]))            # 2^22 x 76 x 76 output pixels: past the 32-bit pixel index
ROW = C.ROWS["goalnet_conv1_dgrad"]


def _mutations():
    for i in ROW["null"]:
        yield "null", i, None, C.E_NULL
    for i, v in ROW["shape"]:
        yield "shape", i, v, C.E_SHAPE
    for i, v in ROW["align"]:
        yield "align", i, v, C.E_ALIGN
    for k, (changes, code) in enumerate(ROW["extra"]):
        yield "extra", k, changes, code


@pytest.mark.parametrize("kind,index,value,code", list(_mutations()), ids=lambda v: str(v))
def test_conv1_dgrad_bad_argument_is_refused_before_any_launch(kind, index, value, code):
    args = list(ROW["args"])
    if kind == "extra":
        for i, v in value.items():
            args[i] = v
    else:
        args[index] = value
    C._refused(_lib.load(), "goalnet_conv1_dgrad", args, code, f"{kind}: argument {index} = {value}")


def test_conv1_dgrad_row_covers_every_pointer_and_the_abi_version_stays():
    types = _lib.PROTOTYPES["goalnet_conv1_dgrad"][1]
    assert len(ROW["args"]) == len(types) == 8
    assert set(ROW["null"]) == {i for i, t in enumerate(types[:-1]) if t is _lib.P} == {0, 1, 2}, "no pointer is nullable"
    assert {i for i, _ in ROW["align"]} == {0}, "dy is read as float4; out is written by scalar stores and needs no alignment"
    lib = _lib.load()
    assert lib.goalnet_abi_version() == _lib.ABI_VERSION == 7
    # the messages name what was wrong
    assert lib.goalnet_conv1_dgrad(4096, 8192, 12288, 3, 2, 40, 40, None) == C.E_SHAPE and b"reduce" in lib.goalnet_last_error()
    assert lib.goalnet_conv1_dgrad(4096 + 4, 8192, 12288, 0, 2, 40, 40, None) == C.E_ALIGN and b"aligned" in lib.goalnet_last_error()


def _oracle_input_grads(name, dtype=torch.float32, taps=None, inter=None):
    g = Golden(name)
    evalmode = bool(g.z["meta|eval"][0])
    p = {k: torch.from_numpy(v).to(dtype) for k, v in synth.make_params(g.h, g.h, 30, g.audio).items()}
    b = eval_ref.running_stats() if evalmode else avm_ref.init_buffers()
    b = {k: (v.to(dtype) if v.is_floating_point() else v.clone()) for k, v in b.items()}
    vis = torch.from_numpy(synth.make_visual(g.n, g.h, g.h)).to(dtype).requires_grad_()
    aud = torch.from_numpy(synth.make_audio(g.n)).to(dtype).requires_grad_() if g.audio else None
    pred = avm_ref.forward(p, b, aud, vis, None, g.audio, inter, pool_taps=taps, training=not evalmode)
    (pred.view(-1) * torch.linspace(0.5, 1.5, g.n, dtype=dtype)).sum().backward()
    return g, pred.detach(), vis.grad, None if aud is None else aud.grad


@pytest.mark.parametrize("case", INPUTGRAD_CASES)
def test_oracle_input_gradients_match_reference_goldens(case):
    torch.set_num_threads(8)
    g, pred, dvis, daud = _oracle_input_grads(case)
    assert dvis.shape == (g.n, 3, g.h, g.h)
    # the fixtures were produced by the reference with the same ATen build: expect (near) bit equality
    g.check("s0.pred", pred, rtol=1e-6)
    g.check("s0.igrad.visual", dvis, rtol=1e-5)
    assert ("s0.igrad.audio" in g.keys("s0.igrad.")) == g.audio
    if g.audio:
        assert daud.shape == (g.n, 30, 30)
        g.check("s0.igrad.audio", daud, rtol=1e-5)
    # stride = kernel = 3 with pad 3 covers every real pixel exactly once: no pixel is without a gradient
    assert bool((dvis != 0).all())


def test_fp32_oracle_is_within_rounding_of_its_fp64_run():
    """the reference's own error, the yardstick of the GPU tests' sharp check: 3.4e-7 .. 7.2e-7 of max|g| when the fixtures were made.
    Under the SAME pool routing: max-pool routing is discontinuous, so the fp64 run takes the fp32 run's argmax positions."""
    for case in INPUTGRAD_CASES:
        inter = {}
        _, _, v32, a32 = _oracle_input_grads(case, inter=inter)
        taps = {i: avm_ref.natural_taps(inter[f"visbl.relu{i}"].detach())[0] for i in (1, 2, 3)}
        _, _, v64, a64 = _oracle_input_grads(case, torch.float64, taps=taps)
        for tag, x, y in (("visual", v32, v64), ("audio", a32, a64)):
            if x is None:
                continue
            e = (x.double() - y).abs().max().item() / y.abs().max().item()
            print(f"{case} {tag}: fp32 oracle is {e:.2e} of max|g| from the fp64 run")
            assert e < 1e-5


def test_per_frame_attribution_holds_in_eval_mode_only():
    """d pred[0] / d frame[1:] is exactly 0 under eval(); in train mode BatchNorm couples the frames (AVM.saliency's docstring)"""
    n, h = 3, 40
    p = {k: torch.from_numpy(v) for k, v in synth.make_params(h, h, 30, True).items()}
    aud = torch.from_numpy(synth.make_audio(n))
    for training, bufs in ((False, eval_ref.running_stats()), (True, avm_ref.init_buffers())):
        vis = torch.from_numpy(synth.make_visual(n, h, h)).requires_grad_()
        pred = avm_ref.forward(p, bufs, aud, vis, None, True, None, training=training)
        pred.view(-1)[0].backward()
        assert bool((vis.grad[0] != 0).any())
        assert bool((vis.grad[1:] == 0).all()) == (not training)


def conv1_dgrad_formula(dy_nhwc, w_oihw, H, W):
    """the header of conv1_dgrad_kernel, literally: dx[n][ci][h][w] = sum_co dy[n][(h+3)/3][(w+3)/3][co] * w[co][ci][(h+3)%3][(w+3)%3]"""
    hh, ww = torch.arange(H) + 3, torch.arange(W) + 3
    d = dy_nhwc[:, hh // 3][:, :, ww // 3]                                    # (N, H, W, 64)
    wt = w_oihw[:, :, hh % 3][:, :, :, ww % 3]                                # (64, 3, H, W)
    return torch.einsum("nhwo,ochw->nchw", d, wt)


@pytest.mark.parametrize("n,h,w", [(1, 40, 40), (3, 41, 52), (2, 42, 40), (1, 7, 5), (1, 1, 2)])
def test_one_window_and_one_tap_per_pixel_is_the_conv2d_data_gradient(n, h, w):
    gen = torch.Generator().manual_seed(1234 + h * w)
    ho, wo = (h + 3) // 3 + 1, (w + 3) // 3 + 1
    x = torch.randn(n, 3, h, w, dtype=torch.float64, generator=gen).requires_grad_()
    wt = torch.randn(64, 3, 3, 3, dtype=torch.float64, generator=gen)
    dy = torch.randn(n, 64, ho, wo, dtype=torch.float64, generator=gen)
    y = F.conv2d(x, wt, stride=3, padding=3)
    assert y.shape == dy.shape
    (y * dy).sum().backward()
    mine = conv1_dgrad_formula(dy.permute(0, 2, 3, 1).contiguous(), wt, h, w)
    assert (mine - x.grad).abs().max().item() <= 1e-12 * x.grad.abs().max().item()


@pytest.mark.parametrize("index", [4, 2], ids=["fp32-classifier-eval", "bf16-train"])
def test_the_mode_comparison_passes_the_oracle_and_catches_a_wrong_device(index):
    """tests/_inputgrad_case.compare, the judge of the GPU test of the other modes, run without a GPU: handed the oracle's own input
    gradients and decisions (_mode_case.oracle_as_device) it passes; handed those of frames in another order it fails"""
    import _inputgrad_case as IC
    c = IC.CELLS[index]
    fx = IC.fixture_of(c)
    w = IC.weights_of(c)
    IC.compare(c, fx, IC.oracle_device(c, fx, w), w)
    with pytest.raises(AssertionError):
        IC.compare(c, fx, IC.oracle_device(c, fx, w, vis=fx["vis"].roll(1, 0)), w, log=lambda *_: None)


@pytest.mark.parametrize("index", [0, 1], ids=["fp32-41x52", "bf16-64x40"])
def test_the_mode_comparison_on_non_square_frames_passes_the_oracle_and_catches_a_wrong_device(index):
    """the two cells on frames with H != W: the oracle passes; frames in another order fail, and so does a device that ran on frames
    mirrored along W (its d_visual has the right shape and the right size everywhere, on the wrong pixels)"""
    import _inputgrad_case as IC
    c = IC.SHAPE_CELLS[index]
    fx = IC.fixture_of(c)
    w = IC.weights_of(c)
    assert c.hw[0] != c.hw[1] and fx["vis"].shape == (c.n, 3, *c.hw)
    dev = IC.oracle_device(c, fx, w)
    assert dev["d_vis"].shape == (c.n, 3, *c.hw)
    IC.compare(c, fx, dev, w)
    for vis in (fx["vis"].roll(1, 0), fx["vis"].flip(3)):
        with pytest.raises(AssertionError):
            IC.compare(c, fx, IC.oracle_device(c, fx, w, vis=vis), w, log=lambda *_: None)


def test_python_side_errors_come_before_any_device_work(monkeypatch):
    from cvml_goalnet_amd import AVM, GoalnetError
    monkeypatch.setattr(torch.cuda, "is_available", lambda: False)
    m = AVM(audio_included=True)
    with pytest.raises(ValueError):
        m.saliency(torch.zeros(2, 30, 30), torch.zeros(2, 3, 40, 40), reduce="mean")
    with pytest.raises(GoalnetError):                                          # no GPU: no CPU fallback
        m.input_gradients(torch.zeros(2, 30, 30), torch.zeros(2, 3, 40, 40))
