"""CPU: judges of the device's DISCONTINUOUS decisions — max-pool taps, ReLU gates of the conv blocks, ReLU gates of linear5 and the
fusion MLP (the multipliers saved for backward) — against the oracle's own. Plain functions of CPU tensors: the GPU tests hand them
what the device decided, tests/test_decisions_host.py hands them synthetic decisions derived from the oracle's.

The parity tests run the oracle's backward under the device's decisions (oracle/avm_ref.py: _ForcedMaxPool, relu_gates), so a wrong
decision moves the oracle with it. Each adopted decision is therefore checked here: where it differs from the oracle's own, the oracle's
value must be within a stated bound of the discontinuity — the top-2 gap of the window for a tap, |y| at the argmax for a conv gate,
|pre-activation| for an MLP gate. The bound is the fp32 rounding floor NEAR_TIE x max|y| of the layer, and in the 16-bit modes the
layer's 16-bit activation noise `b`, measured from the REFERENCE (storage_noise), never from the device."""
import torch

from oracle import avm_ref

NEAR_TIE = 1e-5   # a gap below 1e-5 x max|activation| of the layer is within the convolution's fp32 rounding (tests/test_gpu_avm.py)
MLP_LAYERS = ("visbl.linear5", "fusion.0", "fusion.3", "fusion.6", "fusion.9")      # inter / relu_gates keys; drop_masks[0..4] in this order
STORED_16 = ("visbl.conv2", "visbl.conv3", "visbl.bnorm1", "visbl.bnorm2", "visbl.bnorm3",
             "visbl.conv2.weight", "visbl.conv3.weight", "visbl.linear5.weight")


def saved_mult_check(name, mult, pre, dropmask, band):
    """mult_out of a linear forward against `pre` (fp64 pre-activation, bias included) and the dropout multipliers (None: the bare gate):
    exactly (pre > 0) * dropmask on every element with |pre| > band * max|pre| — an element further from zero than the output's allowed
    error cannot legitimately have the other sign — and exactly 0 or the mask's value everywhere. At most 0.1 % of the elements may lie
    inside the excluded band: a property of the fp64 reference alone (expected share ~band)."""
    mult = mult.detach().cpu().double()
    dm = torch.ones_like(pre) if dropmask is None else dropmask.detach().cpu().double()
    assert mult.shape == pre.shape == dm.shape
    safe = pre.abs() > band * pre.abs().max()
    share = 1.0 - safe.double().mean().item()
    assert share <= 1e-3, f"{name}: {share:.2e} of the reference's pre-activations lie inside the excluded band: change the seed"
    assert ((mult == 0) | (mult == dm)).all(), f"{name}: a saved multiplier is neither 0 nor the dropout multiplier"
    want = (pre > 0).double() * dm
    bad = (mult != want) & safe
    print(f"[parity] {name}: saved multiplier checked on {int(safe.sum())} of {safe.numel()} elements ({safe.numel() - int(safe.sum())} inside the band)")
    assert not bad.any(), (f"{name}: {int(bad.sum())} saved multipliers differ from (pre > 0) * dropmask away from zero; "
                           f"largest |pre| there {pre[bad].abs().max().item():.3e} of max|pre| {pre.abs().max().item():.3e}")


def tap_flips(y_relu, taps):
    """windows of one max-pool whose given argmax tap differs from ATen's on y_relu: (count, largest top-2 gap among them)"""
    nat, gap, _ = avm_ref.natural_taps(y_relu)
    diff = nat != taps
    return int(diff.sum()), float(gap[diff].max()) if diff.any() else 0.0


def conv_gate_flips(y, taps, gate):
    """windows whose given ReLU gate at the given argmax differs from y > 0 there: (count, largest |y| at the argmax among them)"""
    at = avm_ref._ForcedMaxPool.apply(y, taps)
    diff = (at > 0) != gate
    return int(diff.sum()), float(at[diff].abs().max()) if diff.any() else 0.0


def mlp_gate_flips(pre, gate, dropmult):
    """units whose given gate differs from pre > 0, among those the dropout keeps (where its multiplier is 0 the saved multiplier is 0
    whatever the gate): (count, largest |pre| among them)"""
    diff = (pre > 0) != gate
    if dropmult is not None:
        diff &= dropmult != 0
    return int(diff.sum()), float(pre[diff].abs().max()) if diff.any() else 0.0


def decisions(inter, taps, gates, drop_masks, mlp=True):
    """every disagreement between the given decisions and the oracle's own (`inter` of a plain oracle forward), per layer:
    {(kind, layer): (count, worst distance from the discontinuity, max|y| of the layer)} with kind in "tap", "gate", "mlp" """
    out = {}
    for i in (1, 2, 3):
        y = inter[f"visbl.conv{i}"].detach()
        scale = float(y.abs().max())
        yr = inter[f"visbl.relu{i}"].detach()
        out[("tap", f"visbl.conv{i}")] = tap_flips(yr, taps[i]) + (float(yr.abs().max()),)
        out[("gate", f"visbl.conv{i}")] = conv_gate_flips(y, taps[i], gates[i]) + (scale,)
    if mlp:
        for li, key in enumerate(MLP_LAYERS):
            pre = inter[key].detach()
            out[("mlp", key)] = mlp_gate_flips(pre, gates[key], None if drop_masks is None else drop_masks[li]) + (float(pre.abs().max()),)
    return out


def storage_noise(p, b, audio, visual, drop_masks, inter, dtype, head="regression", training=True):
    """b_layer of every layer with a decision: twice the largest change of its pre-activation when the oracle's forward is run once more
    with every tensor that a 16-bit mode stores in 16 bits (the conv outputs y — hence the pooled p — of blocks 2 and 3,
    the BatchNorm-applied GEMM operands of conv2, conv3 and linear5, and those GEMMs' weight operands) rounded through `dtype` where it
    is stored. `inter`: the plain forward on the same inputs (same `head`, same `training`). The factor 2: the device's fp32 accumulation order and its own routing
    flips come on top of the storage rounding that this emulation models."""
    rounded = {}
    with torch.no_grad():
        avm_ref.forward(p, {k: v.clone() for k, v in b.items()}, audio, visual, drop_masks, audio is not None, rounded,
                        head=head, store=lambda name, x: x.to(dtype).to(x.dtype) if name in STORED_16 else x, training=training)
    keys = [f"visbl.conv{i}" for i in (1, 2, 3)] + list(MLP_LAYERS)
    return {k: 2.0 * float((rounded[k] - inter[k]).abs().max()) for k in keys}


def judge(found, noise=None):
    """one rule for every disagreement: a tap's top-2 gap <= 2 x bound, a gate's |y| (or |pre|) <= bound, with bound = the layer's fp32
    rounding floor NEAR_TIE x max|y| or, where given, its 16-bit activation noise (whichever is larger: block 1 and the fusion layers
    compute in fp32 in every mode). Without `noise` (the fp32-grade modes) taps too are held to the floor itself, as they always were.
    Returns the list of failures."""
    failures = []
    for (kind, layer), (count, worst, scale) in found.items():
        floor = NEAR_TIE * scale
        bound = floor if noise is None else max(floor, (2.0 if kind == "tap" else 1.0) * noise[layer])
        if count and worst > bound:
            what = {"tap": "max-pool window routed differently where its top-2 gap is", "gate": "ReLU gate at a window's argmax differs where |y| is",
                    "mlp": "saved ReLU gate differs from the oracle's pre-activation sign where |pre| is"}[kind]
            failures.append(f"{layer}: {what} {worst:.3e} > {bound:.3e} (max|y| of the layer {scale:.3e}; {count} disagreements)")
    return failures


def report_lines(found, noise=None):
    """one line per layer for the [parity] log: disagreements, the worst one and (16-bit modes) b_layer, all relative to max|y|"""
    lines = []
    layers = []
    for _, layer in found:
        if layer not in layers:
            layers.append(layer)
    for layer in layers:
        kinds = [kind for kind in ("tap", "gate", "mlp") if (kind, layer) in found]
        parts = [f"{kind} {found[(kind, layer)][0]} (worst {found[(kind, layer)][1] / max(found[(kind, layer)][2], 1e-30):.2e})" for kind in kinds]
        tail = "" if noise is None else f"; b_layer / max|y| = {noise[layer] / max(found[(kinds[-1], layer)][2], 1e-30):.2e}"
        lines.append(f"{layer}: disagreements (worst one over max|y|) " + ", ".join(parts) + tail)
    return lines


def totals(found, kind):
    """(number of disagreements of one kind over all layers, the worst one relative to its layer's max|y|): the figures the fp32 engine's
    tests have always printed and asserted"""
    rows = [v for k, v in found.items() if k[0] == kind]
    return sum(v[0] for v in rows), max([v[1] / max(v[2], 1e-30) for v in rows if v[0]], default=0.0)
