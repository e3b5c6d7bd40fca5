"""Input gradients of one mode cell against the CPU oracle: d(sum_i w_i out_i) / d(audio, visual) of tests/_mode_case.py's fixtures.

Three parts, as in tests/_mode_case.py, so that the comparison can be run — and broken on purpose — without a GPU
(tests/test_inputgrad_host.py):

  oracle_input_grads(...)   the oracle's input gradients in any dtype under GIVEN max-pool taps and ReLU gates
  run_device(...)           AVM.input_gradients on the device -> a dict of CPU tensors (what it decided and computed)
  compare(...)              that dict against the oracle under the adopted decisions; oracle_device(...) builds the same dict from
                            _mode_case.oracle_as_device, which is how the host tests exercise compare()

Criteria: none is new. fp32-grade cells (fp32, bf16x6, fp16x3): each input gradient no further from the fp64 oracle under the device's
decisions than max(F32_FACTOR[precision] x e_ref, 2e-6 max|g|), e_ref = the fp32 oracle's own distance from it. bf16 / fp16: relative L2
against the fp32 oracle under the device's decisions <= TOL16[precision][1], the bound visbl.conv1.weight's gradient meets from the same
dy1; d_audio is held to the same bound (AudBl computes in fp32 in every mode; it sees the 16-bit chain only through the fusion
layers' gradient, as audbl.*'s weight gradients do). Every adopted decision goes through decisions() and judge()."""
import torch

from _decisions import decisions, judge, report_lines, storage_noise
from _mode_case import Cell, _clone, cell_id, fixture_of, h16_of, oracle_as_device  # noqa: F401
from oracle import avm_ref
from test_gpu_bench_shapes import F32_FACTOR, TOL16, _gates_first, _mlp_gates_first, _taps_first

DEV = "cuda:0"
FP32_GRADE = ("fp32", "bf16x6", "fp16x3")

# one cell per mode beyond the fp32 goldens, N = 10 frames of 40 x 40: the two split-operand precisions, the two 16-bit ones (fp16 with its
# automatic loss scale), the classifier head with (N, 5) weights, and a model without audio; train and eval mode both appear
CELLS = (
    Cell("bf16x6", "regression", True, "train", 10),
    Cell("fp16x3", "regression", True, "eval", 10),
    Cell("bf16", "regression", True, "train", 10),
    Cell("fp16", "regression", True, "eval", 10),
    Cell("fp32", "classifier", True, "eval", 10),
    Cell("fp32", "regression", False, "train", 10),
)

# two of them on frames with H != W (tests/_mode_case.py: SHAPE_CELLS): conv1's data gradient with another remainder along each axis
# (41 % 3 = 2, 52 % 3 = 1) and d_visual returned as (N, 3, H, W) on a frame taller than wide, under the fp32 and the bf16 chain
SHAPE_CELLS = (
    Cell("fp32", "regression", False, "train", 10, (41, 52)),
    Cell("bf16", "regression", True, "train", 10, (64, 40)),
)


def weights_of(c, classes=5):
    """frame weights linspace(0.5, 1.5, N) — for the classifier head (N, C), every class with its own sign and size"""
    w = torch.linspace(0.5, 1.5, c.n)
    if c.head != "classifier":
        return w
    return w[:, None] * torch.tensor([1.0, -0.5, 0.25, -1.5, 0.75])[None, :classes]


def oracle_input_grads(c, fx, weights, dtype=torch.float32, taps=None, gates=None, vis=None):
    """(d_audio | None, d_visual, pred) of the oracle in `dtype` under the given decisions"""
    p = {k: v.to(dtype) for k, v in fx["p"].items()}
    b = {k: (v.to(dtype) if v.is_floating_point() else v.clone()) for k, v in fx["b"].items()}
    masks = None if fx["masks"] is None else [m.to(dtype) for m in fx["masks"]]
    v = (fx["vis"] if vis is None else vis).to(dtype).clone().requires_grad_()
    a = None if fx["aud"] is None else fx["aud"].to(dtype).clone().requires_grad_()
    pred = avm_ref.forward(p, b, a, v, masks, c.audio, None, pool_taps=taps, head=c.head, relu_gates=gates, training=c.mode == "train")
    (pred.reshape(c.n, -1) * weights.to(dtype).reshape(c.n, -1)).sum().backward()
    return (None if a is None else a.grad), v.grad, pred.detach()


def oracle_device(c, fx, weights, vis=None):
    """the dict run_device() returns, computed by the fp32 oracle with its own decisions (`vis`: another visual input — a wrong device)"""
    dev = oracle_as_device(c, fx, vis=vis)
    d_aud, d_vis, pred = oracle_input_grads(c, fx, weights, vis=vis)
    return {"taps": dev["taps"], "gates": dev["gates"], "d_aud": d_aud, "d_vis": d_vis, "pred": pred.reshape(c.n, -1)}


def compare(c, fx, dev, weights, log=print):
    """`dev` against the oracle under the decisions `dev` carries; asserts at the end, returns the figures it printed"""
    f32 = c.precision in FP32_GRADE
    train = c.mode == "train"
    tag = f"[inputgrad] {cell_id(c)}"
    taps = dev["taps"]
    gates = {k: v for k, v in dev["gates"].items() if not f32 or k in (1, 2, 3)}      # as _mode_case.compare: 16-bit cells adopt the MLP gates too
    failures = []
    inter = {}
    p, b = _clone(fx["p"]), _clone(fx["b"])
    with torch.no_grad():
        avm_ref.forward(p, _clone(b), fx["aud"], fx["vis"], fx["masks"], c.audio, inter, head=c.head, training=train)
    found = decisions(inter, taps, gates, fx["masks"], mlp=not f32)
    noise = None if f32 else storage_noise(p, b, fx["aud"], fx["vis"], fx["masks"], inter, h16_of(c), head=c.head, training=train)
    del inter
    for line in report_lines(found, noise):
        log(f"{tag} decisions, {line}")
    failures += judge(found, noise)

    a32, v32, pred32 = oracle_input_grads(c, fx, weights, torch.float32, taps, gates)
    perr = (dev["pred"].reshape(c.n, -1) - pred32.reshape(c.n, -1)).abs().max().item()
    ptol = 2e-5 if f32 else TOL16[c.precision][2]
    if perr > ptol:
        failures.append(f"predictions {perr:.3e} from the oracle's > {ptol}")
    figures = {}
    if f32:
        a64, v64, _ = oracle_input_grads(c, fx, weights, torch.float64, taps, gates)
        for name, mine, g32, g64 in (("d_visual", dev["d_vis"], v32, v64), ("d_audio", dev["d_aud"], a32, a64)):
            if g64 is None:
                assert mine is None
                continue
            assert mine.shape == g64.shape, (name, mine.shape, g64.shape)
            scale = g64.abs().max().item()
            e_ref = (g32.double() - g64).abs().max().item()
            e_hip = (mine.double() - g64).abs().max().item()
            log(f"{tag} {name}: max|g| {scale:.3e}  e_ref {e_ref:.3e} ({e_ref / scale:.2e} of max|g|)  e_hip {e_hip:.3e} ({e_hip / scale:.2e})")
            figures[name] = e_hip / scale
            if not e_hip <= max(F32_FACTOR[c.precision] * e_ref, 2e-6 * scale):
                failures.append(f"{name} is {e_hip:.3e} from the fp64 oracle, the oracle's fp32 path {e_ref:.3e} (max|g| {scale:.3e})")
    else:
        for name, mine, g32 in (("d_visual", dev["d_vis"], v32), ("d_audio", dev["d_aud"], a32)):
            if g32 is None:
                assert mine is None
                continue
            assert mine.shape == g32.shape, (name, mine.shape, g32.shape)
            l2 = ((mine.double() - g32.double()).norm() / g32.double().norm().clamp_min(1e-30)).item()
            log(f"{tag} {name}: relative L2 {l2:.3e} (bound {TOL16[c.precision][1]}), max|g| {g32.abs().max().item():.3e}")
            figures[name] = l2
            if not l2 <= TOL16[c.precision][1]:
                failures.append(f"{name}: {c.precision}-mode relative L2 error {l2:.3e} > {TOL16[c.precision][1]}")
    assert not failures, f"{cell_id(c)}:\n" + "\n".join(failures)
    return figures


def make_model(c, fx):
    from cvml_goalnet_amd import AVM, synth
    m = AVM(audio_included=c.audio, device=DEV, seed=synth.BASE_SEED, head=c.head, precision=c.precision)
    sd = _clone(fx["p"])
    sd.update(_clone(fx["b"]))
    m.load_state_dict(sd)
    if c.mode == "train":
        m.set_dropout_masks(fx["masks"])
    else:
        m.dropout_mode = "device"              # live dropout: eval() itself must switch it off
        m.eval()
    return m


def device_decisions(ctx, n):
    gates = _gates_first(ctx, n)
    gates.update(_mlp_gates_first(ctx, n, ctx["hs"][0].shape[1] - 512))
    return _taps_first(ctx, n), gates


def run_device(c, fx, weights):
    """AVM.input_gradients of the cell on the GPU -> the dict compare() reads"""
    m = make_model(c, fx)
    m.keep_ctx = True
    aud = None if fx["aud"] is None else fx["aud"].to(DEV)
    d_aud, d_vis = m.input_gradients(aud, fx["vis"].to(DEV), weights.to(DEV))
    torch.cuda.synchronize()
    ctx, m.last_ctx = m.last_ctx, None
    if c.precision == "fp16":
        assert m._loss_scale_for(c.n) > 1.0, "the cell is here for the automatic loss scale"
    assert (d_aud is None) == (not c.audio) and d_vis.is_cuda and d_vis.dtype == torch.float32
    taps, gates = device_decisions(ctx, c.n)
    return {"taps": taps, "gates": gates, "d_aud": None if d_aud is None else d_aud.cpu(), "d_vis": d_vis.cpu(),
            "pred": ctx["out"].cpu().reshape(c.n, -1)}, m
