"""GPU: the whole hot path (AVM forward, broadcast MSE, backward, Adam) against
  (a) the golden vectors captured from the reference itself (tests/golden/*.npz), and
  (b) the CPU oracle run live on the same seeded inputs,
through the drop-in surface (`model(audio, visual)`, autograd, stock torch.optim.Adam) and through the fused
device-resident `train_step`. fp32 tolerances: outputs <= 1e-5 relative to the (1,5) range,
gradients / updated parameters per-tensor relative 1e-4 of the tensor's max. Dropout: masks regenerated from
the seed formula on both sides ("mask" cases) or p = 0; BatchNorm: train mode, as the reference."""
import warnings

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from _golden import GOLDEN_CASES_BIG, GOLDEN_CASES_SMALL, Golden  # noqa: E402
from cvml_goalnet_amd import AVM, ops, synth  # noqa: E402
from oracle import avm_ref  # noqa: E402

DEV = "cuda:0"


def load_model(h, audio, bins=30, dropout="device"):
    params = synth.make_params(h, h, bins, audio)
    m = AVM(audio_included=audio, device=DEV, seed=synth.BASE_SEED)
    sd = {k: torch.from_numpy(v) for k, v in params.items()}
    sd.update(avm_ref.init_buffers())
    m.load_state_dict(sd)
    m.dropout_mode = dropout
    return m, params


def inputs(n, h, audio, bins=30):
    vis = torch.from_numpy(synth.make_visual(n, h, h))
    aud = torch.from_numpy(synth.make_audio(n, bins)) if audio else [None] * n
    lab = torch.from_numpy(synth.make_labels(n))
    return aud, vis, lab


LR = 1e-3


def _is_reduction_grad(name):
    """Bias / BatchNorm-affine gradients are plain sums over N*H*W terms that largely cancel (a conv bias in
    front of a BatchNorm has a mathematically ZERO gradient unless a pooling window's maximum is clipped by the
    ReLU): the reference's own fp32 value is rounding noise there. They get an absolute floor tied to the same
    layer's weight gradient; test_gradients_within_reference_rounding_of_fp64_truth is the sharp check."""
    return name.endswith(".bias") or ".bnorm" in name


def _weight_of(name):
    if ".bnorm" in name:
        return name.replace("bnorm", "conv").rsplit(".", 1)[0] + ".weight"
    return name.rsplit(".", 1)[0] + ".weight"


def hip_taps(ctx):
    """argmax positions the device used in its three max-pools, as (N,C,Hp,Wp) uint8 CPU tensors"""
    out = {}
    for i in (1, 2, 3):
        n, hp, wp, c = ctx[f"idx{i}"].shape                              # stored slice-major by the kernels (ops.idx_to_nhwc)
        out[i] = ops.idx_to_nhwc(ctx[f"idx{i}"], n, hp, wp, c).cpu().permute(0, 3, 1, 2).contiguous()
    return out


NEAR_TIE = 1e-5   # a top-2 gap below 1e-5 x max|activation| of the layer is within the convolution's fp32 rounding


def routing_disagreements(inter, taps):
    """Compare the device's max-pool argmax with ATen's on the oracle's activations. Returns (count, worst top-2 gap
    relative to the layer's max |activation|). Max-pool routing is discontinuous: a disagreement is legitimate only
    where the two largest values of the window differ by less than the rounding error of the convolution that
    produced them (a K = 576..2304 fp32 accumulation: ~1e-6 of the output scale) — oracle/avm_ref.py:_ForcedMaxPool."""
    count, worst = 0, 0.0
    for i in (1, 2, 3):
        y = inter[f"visbl.relu{i}"].detach()
        nat, gap, pooled = avm_ref.natural_taps(y)
        diff = nat != taps[i]
        if diff.any():
            count += int(diff.sum())
            worst = max(worst, float(gap[diff].max()) / float(y.abs().max()))
    return count, worst


@pytest.mark.parametrize("case", GOLDEN_CASES_SMALL + GOLDEN_CASES_BIG)
def test_fused_train_steps_match_reference_goldens(case):
    g = Golden(case)
    model, params = load_model(g.h, g.audio, bins=g.bins, dropout="device" if g.drop else "off")
    model.keep_ctx = True
    aud, vis, lab = inputs(g.n, g.h, g.audio, g.bins)
    audg = aud.to(DEV) if g.audio else None
    visg, labg = vis.to(DEV), lab.to(DEV)
    big = g.h > 100
    p = {k: torch.from_numpy(v.copy()) for k, v in params.items()}     # live oracle state (fp32, as the reference)
    b = avm_ref.init_buffers()
    state = {}
    report, failures = [], []
    slack_g, slack_o = {}, {}     # Adam sensitivity bounds vs golden samples / vs live oracle tensors
    rerouted = False
    for s in range(g.steps):
        loss, pred = model.train_step(audg, visg, labg)
        torch.cuda.synchronize()
        pre = f"s{s}."
        taps = hip_taps(model.last_ctx)
        model.last_ctx = None
        if not rerouted:
            report.append((g.check(pre + "pred", pred, rtol=0.0, atol=2e-5), pre + "pred"))
            report.append((g.check(pre + "loss", loss, rtol=2e-5), pre + "loss"))
            report.append((g.check(pre + "act.logit", model.last_logit, rtol=0.0, atol=2e-5), pre + "logit"))
        masks = [torch.from_numpy(m) for m in synth.make_drop_masks(g.n, step=s)] if g.drop else None
        inter = {}
        with torch.no_grad():
            avm_ref.forward(p, {k: v.clone() for k, v in b.items()}, aud if g.audio else None, vis, masks, g.audio, inter)
        nd, worst_ulps = routing_disagreements(inter, taps)
        del inter
        if nd:
            print(f"[parity] {case} step {s}: {nd} max-pool windows routed differently from ATen; largest top-2 gap {worst_ulps:.2e} of max|y|")
            assert worst_ulps <= NEAR_TIE, "max-pool argmax differs from ATen's where the window is NOT a near-tie"
            rerouted = True
        sd = model.state_dict()
        # ---- (a) the reference's golden vectors: valid while the routing decisions agree with the reference's
        if not rerouted:
            for k in g.keys(pre + "grad."):
                name = k.split("grad.", 1)[1]
                mine = g.flat(model.grad_of(name))
                idx, ref = g.samples(k)
                scale = max(g.absmax(k), 1e-30)
                err = np.abs(mine[idx] - ref)
                floor = 2e-5 * g.absmax(pre + "grad." + _weight_of(name)) if _is_reduction_grad(name) else 0.0
                report.append((float(err.max()) / scale, k))
                # steps >= 1 start from parameters that differ from the reference's by the Adam kicks described above
                rt = 1e-4 + 2e-3 * s
                if err.max() > rt * scale + floor:
                    failures.append(f"{k}: err {err.max():.3e} > tol {rt * scale + floor:.3e} (max|g| {scale:.3e})")
                # first-order sensitivity of an Adam update to a gradient error: lr * |dg| / (|g| + eps), at most 2 lr
                slack_g[name] = slack_g.get(name, 0.0) + LR * np.minimum(2.0, 8.0 * err / (np.abs(ref) + 1e-8))
            for k in g.keys(pre + "param."):
                name = k.split("param.", 1)[1]
                idx, ref = g.samples(k)
                err = np.abs(g.flat(sd[name])[idx] - ref)
                tol = 2e-6 + slack_g[name]
                report.append((float(err.max()), k + " [abs]"))
                if (err > tol).any():
                    i = int(np.argmax(err - tol))
                    failures.append(f"{k} (after Adam): err {err[i]:.3e} > tol {tol[i]:.3e}")
            for k in g.keys(pre + "buf."):
                # from the second step on, running means inherit 0.1 x the Adam noise of the conv biases (see above)
                report.append((g.check(k, sd[k.split("buf.", 1)[1]], rtol=1e-5, atol=0.1 * 2 * LR * s, what=" (BatchNorm buffer)"), k))
        # ---- (b) the live oracle under the device's routing decisions (all tensors, every element)
        if rerouted or not big:
            o_loss, o_pred, o_g = avm_ref.train_step(p, b, state, aud if g.audio else None, vis, lab, masks, g.audio,
                                                     pool_taps=taps if rerouted else None)
            assert (pred.cpu().view(-1, 1) - o_pred).abs().max().item() < 2e-5
            assert abs(loss.item() - o_loss.item()) < 2e-5 * max(1.0, abs(o_loss.item()))
            for name, og in o_g.items():
                mine = model.grad_of(name).cpu().reshape(og.shape)
                scale = max(og.abs().max().item(), 1e-30)
                gerr = (mine - og).abs()
                floor = 2e-5 * o_g[_weight_of(name)].abs().max().item() if _is_reduction_grad(name) else 0.0
                report.append((gerr.max().item() / scale, f"{pre}grad.{name} [oracle]"))
                if gerr.max().item() > 1e-4 * scale + floor:
                    failures.append(f"{pre}{name}: gradient vs oracle err {gerr.max().item():.3e} (max|g| {scale:.3e})")
                slack_o[name] = slack_o.get(name, 0.0) + LR * torch.clamp(8.0 * gerr / (og.abs() + 1e-8), max=2.0)
                over = ((sd[name] - p[name]).abs() - (2e-6 + slack_o[name])).max().item()
                if over > 0:
                    failures.append(f"{pre}{name}: after Adam exceeds its sensitivity bound vs oracle by {over:.3e}")
            for k, v in b.items():
                if not torch.allclose(sd[k].double(), v.double(), rtol=1e-5, atol=1e-6):
                    failures.append(f"{pre}{k}: BatchNorm buffer differs from oracle")
            # start the next step from the device's parameters: Adam turns rounding noise in ~zero gradients (conv
            # biases) into +-lr kicks, and routing decisions must be compared on the SAME parameters
            for k in p:
                p[k].copy_(sd[k])
            for k in b:
                b[k].copy_(sd[k])
    report.sort(reverse=True)
    print(f"[parity] {case}: largest errors (relative to max|ref| unless [abs]); rerouted={rerouted}")
    for e, k in report[:8]:
        print(f"[parity]     {e:.3e}  {k}")
    assert not failures, "\n".join(failures)


def test_gradients_within_reference_rounding_of_fp64_truth():
    """Sharp gradient check without cancellation blind spots: run the oracle in fp64 (truth) and in fp32 (what the
    reference computes) under the device's max-pool routing, and require the HIP gradient of EVERY parameter tensor
    to be as close to the truth as the reference's own fp32 arithmetic is (x4), or within 2e-6 of its magnitude."""
    from cvml_goalnet_amd import ops
    n, h = 16, 40
    model, params = load_model(h, True)
    aud, vis, lab = inputs(n, h, True)
    masks = [torch.from_numpy(m) for m in synth.make_drop_masks(n, step=0)]
    out, ctx = model.forward_device(aud.to(DEV), vis.to(DEV), save=True)
    loss = torch.empty(1, device=DEV); dout = torch.empty(n, device=DEV)
    ops.mse_bcast(out, lab.to(DEV), loss, dout)
    model.backward_device(ctx, dout)
    torch.cuda.synchronize()
    taps = hip_taps(ctx)

    def oracle_grads(dtype):
        p = {k: torch.from_numpy(v).to(dtype).requires_grad_(True) for k, v in params.items()}
        inter = {}
        pred = avm_ref.forward(p, avm_ref.init_buffers(dtype), aud.to(dtype), vis.to(dtype), [m.to(dtype) for m in masks], True,
                               inter, pool_taps=taps)
        avm_ref.mse_bcast(pred, lab.to(dtype)).backward()
        return {k: v.grad.double() for k, v in p.items()}, pred.detach().double(), inter

    g64, p64, inter64 = oracle_grads(torch.float64)
    nd, worst = routing_disagreements(inter64, taps)
    print(f"[parity] fp64 truth: {nd} windows routed differently from the fp64 argmax (largest gap {worst:.2e} of max|y|)")
    assert worst <= NEAR_TIE
    g32, p32, _ = oracle_grads(torch.float32)
    e_ref = (p32 - p64).abs().max().item(); e_hip = (out.cpu().double().view(-1, 1) - p64).abs().max().item()
    print(f"[parity] fp64 truth: pred error reference-fp32 {e_ref:.2e}, HIP {e_hip:.2e}")
    assert e_hip <= max(4 * e_ref, 2e-6)
    bad = []
    for k in g64:
        mine = model.grad_of(k).cpu().double().reshape(g64[k].shape)
        scale = max(g64[k].abs().max().item(), 1e-30)
        e_ref = (g32[k] - g64[k]).abs().max().item()
        e_hip = (mine - g64[k]).abs().max().item()
        print(f"[parity] fp64 truth: {k:28s} max|g| {scale:.2e}  err reference-fp32 {e_ref:.2e}  HIP {e_hip:.2e}")
        if e_hip > max(4 * e_ref, 2e-6 * scale):
            bad.append(k)
    assert not bad, f"HIP gradients further from the fp64 truth than the reference's fp32 path: {bad}"


@pytest.mark.parametrize("audio", [True, False])
def test_dropin_surface_cpu_tensors_autograd_and_stock_adam(audio):
    """The reference's own call sequence (main.py:64-70, 187-196) with CPU tensors, vs the oracle."""
    n, h = 10, 40
    model = AVM(audio_included=audio)                                   # main.py:64
    model.dropout_seed = synth.BASE_SEED                                 # the oracle side regenerates the masks from this seed
    optimizer = torch.optim.Adam(params=model.parameters(), lr=0.001)    # main.py:70, BEFORE any forward
    params = synth.make_params(h, h, 30, audio)
    sd = {k: torch.from_numpy(v) for k, v in params.items()}
    sd.update(avm_ref.init_buffers())
    model.load_state_dict(sd)                                            # main.py:66
    criterion = torch.nn.MSELoss()
    aud, vis, lab = inputs(n, h, audio)

    p = {k: torch.from_numpy(v.copy()) for k, v in params.items()}
    b = avm_ref.init_buffers()
    state = {}
    slack = {}
    for step in range(2):
        n_eff = n - 2 if step else n
        masks = [torch.from_numpy(m) for m in synth.make_drop_masks(n_eff, step=step)]
        optimizer.zero_grad()
        with warnings.catch_warnings():
            warnings.simplefilter("ignore")
            out = model(aud[2:], vis[2:]) if step else model(aud, vis)   # sliced views on the second step (main.py:182)
            loss = criterion(out, lab[2:] if step else lab)
        assert out.device.type == "cpu" and out.shape == ((n - 2 if step else n), 1) and out.requires_grad
        loss.backward()
        optimizer.step()
        preds = out.flatten().tolist()                                   # main.py:196
        assert len(preds) == (n - 2 if step else n)
        sl = slice(2, None) if step else slice(None)
        o_loss, o_pred, o_g = avm_ref.train_step(p, b, state, aud[sl] if audio else None, vis[sl], lab[sl], masks, audio)
        assert (out.detach() - o_pred).abs().max().item() < 2e-5
        assert abs(loss.item() - o_loss.item()) < 2e-5 * max(1.0, abs(o_loss.item()))
        new = model.state_dict()
        for k in p:
            gerr = (model.grad_of(k).cpu().reshape(o_g[k].shape) - o_g[k]).abs()
            slack[k] = slack.get(k, 0.0) + LR * torch.clamp(8.0 * gerr / (o_g[k].abs() + 1e-8), max=2.0)
            over = ((new[k] - p[k]).abs() - (2e-6 + slack[k])).max().item()
            assert over <= 0, f"step {step}: {k} after stock Adam exceeds its Adam-sensitivity bound by {over:.3e}"
        for k in b:
            assert torch.allclose(new[k].double(), b[k].double(), rtol=1e-5, atol=1e-6 + 0.1 * 2 * LR * step), k
    # parameters the optimizer holds are the SAME objects that were materialised
    assert all(q.is_cuda for grp in optimizer.param_groups for q in grp["params"])


def test_dropin_surface_with_the_fused_adam_equals_stock_adam():
    """cvml_goalnet_amd.optim.Adam (one pass over the arena) in place of torch.optim.Adam on the drop-in path (main.py:70, 187-193):
    same parameters after three steps, created before the first forward like the stock one."""
    n, h = 10, 40
    aud, vis, lab = inputs(n, h, True)
    criterion = torch.nn.MSELoss()
    out = {}
    for kind in ("stock", "fused"):
        model = AVM(audio_included=True)
        model.dropout_seed = synth.BASE_SEED
        optimizer = torch.optim.Adam(model.parameters(), lr=0.001) if kind == "stock" else model.make_optimizer(lr=0.001)
        sd = {k: torch.from_numpy(v) for k, v in synth.make_params(h, h, 30, True).items()}
        sd.update(avm_ref.init_buffers())
        model.load_state_dict(sd)
        for _ in range(3):
            optimizer.zero_grad()
            with warnings.catch_warnings():
                warnings.simplefilter("ignore")
                loss = criterion(model(aud, vis), lab)
            loss.backward()
            optimizer.step()
        out[kind] = (model._arena.clone(), loss.item())
    diff = (out["stock"][0] - out["fused"][0]).abs()
    # torch steps CUDA parameters with its multi-tensor (foreach) Adam, whose operation order differs from the single-tensor one the fused
    # kernel follows; Adam turns a last-bit difference in a near-zero gradient entry into a kick of up to lr per step. Almost every element
    # agrees to rounding, none may be further apart than 2 lr per step, and the loss of the third step agrees.
    frac = (diff > 1e-6).double().mean().item()
    print(f"[parity] fused vs stock Adam on the drop-in path: max |dp| {diff.max().item():.2e}, {frac:.2e} of the elements beyond 1e-6")
    assert diff.max().item() <= 3 * 2 * LR and frac <= 1e-3, (diff.max().item(), frac)
    assert out["stock"][1] == pytest.approx(out["fused"][1], rel=1e-5)


def test_eval_forward_under_no_grad_updates_bn_buffers():
    """main.py:93-95: whole-video forward under no_grad, model still in train mode."""
    n, h = 23, 40
    model, params = load_model(h, True)
    aud, vis, lab = inputs(n, h, True)
    with torch.no_grad():
        out = model(aud, vis)
    assert not out.requires_grad and out.shape == (n, 1)
    p = {k: torch.from_numpy(v.copy()) for k, v in params.items()}
    b = avm_ref.init_buffers()
    masks = [torch.from_numpy(m) for m in synth.make_drop_masks(n, step=0)]
    with torch.no_grad():
        ref = avm_ref.forward(p, b, aud, vis, masks, True)
    assert (out - ref).abs().max().item() < 2e-5
    sd = model.state_dict()
    assert int(sd["visbl.bnorm2.num_batches_tracked"]) == 1
    assert torch.allclose(sd["visbl.bnorm3.running_var"], b["visbl.bnorm3.running_var"], rtol=1e-5, atol=1e-7)
    rounded = torch.round(out[:, 0]).type(torch.int8).tolist()          # utils.py:610-611 consumes it like this
    assert rounded == torch.round(ref[:, 0]).type(torch.int8).tolist()


def test_state_dict_round_trip_is_torch_native_and_exact(tmp_path):
    model, params = load_model(40, True)
    sd = model.state_dict()
    assert list(sd.keys())[:7] == ["visbl.conv1.weight", "visbl.conv1.bias", "visbl.bnorm1.weight", "visbl.bnorm1.bias",
                                   "visbl.bnorm1.running_mean", "visbl.bnorm1.running_var", "visbl.bnorm1.num_batches_tracked"]
    for k, v in params.items():
        assert sd[k].device.type == "cpu" and tuple(sd[k].shape) == v.shape
        assert np.array_equal(sd[k].numpy(), v), k          # layout permutations are exact
    f = tmp_path / "ckp.pt"
    torch.save(sd, f)                                         # main.py:282
    m2 = AVM(audio_included=True)
    m2.load_state_dict(torch.load(f))                         # main.py:66
    sd2 = m2.state_dict()
    assert all(torch.equal(sd[k], sd2[k]) for k in sd)


def test_default_init_ranges_and_lazy_materialisation():
    torch.manual_seed(1)
    m = AVM(audio_included=True)
    assert all(isinstance(q, torch.nn.parameter.UninitializedParameter) for q in m.parameters())
    aud, vis, _ = inputs(3, 40, True)
    with torch.no_grad():
        out = m(aud, vis)
    assert out.shape == (3, 1) and bool(((out > 1) & (out < 5)).all())
    sd = m.state_dict()
    assert tuple(sd["visbl.linear5.weight"].shape) == (512, 41472)
    for k, v in sd.items():
        if k.endswith("weight") and ".bnorm" not in k:
            bound = 1.0 / np.sqrt(v[0].numel())
            assert v.abs().max().item() <= bound + 1e-7 and v.abs().max().item() > 0.9 * bound, k
    assert torch.equal(sd["visbl.bnorm1.weight"], torch.ones(64))
    with pytest.raises(RuntimeError):
        m(aud, torch.zeros(3, 3, 52, 52))                     # Lazy shapes are fixed after the first forward


def test_ragged_and_edge_batches_properties():
    """Sizes the goldens do not cover: N = 1 and a non-multiple-of-tile N at 64x48 frames; properties only."""
    model, _ = load_model(40, True, dropout="off")
    for n in (1, 37):
        aud, vis, lab = inputs(n, 40, True)
        with torch.no_grad():
            a = model(aud, vis)
            b2 = model(aud, vis)
        assert torch.equal(a, b2), "forward is not deterministic"
        assert bool(((a > 1) & (a < 5)).all())
    # frames are independent given the batch statistics: permuting the batch permutes the output
    aud, vis, lab = inputs(12, 40, True)
    perm = torch.randperm(12, generator=torch.Generator().manual_seed(0))
    with torch.no_grad():
        o1 = model(aud, vis)
        o2 = model(aud[perm], vis[perm])
    assert (o1[perm] - o2).abs().max().item() < 2e-5


def test_bf16_mode_logits_within_1e3_and_gradients_track_the_oracle():
    """precision='bf16' (bf16 MFMA contractions, fp32 accumulate / statistics / master weights): the north star's
    tolerance is 1e-3 on the pre-sigmoid logit vs the fp32 CPU reference. Gradients are compared under the device's
    max-pool routing; with activations perturbed at the 1e-3 level some ReLU / dropout-scaled units flip state, which
    moves individual gradient elements at O(1) with only 16 frames in the batch, so the bound is on the relative L2
    error of every weight gradient (<= 0.15, i.e. cosine similarity > 0.99), not on the max element. The bf16 kernels
    themselves are checked to 5e-6 against fp64 on bf16-rounded operands in tests/test_gpu_ops.py."""
    n, h = 16, 40
    params = synth.make_params(h, h, 30, True)
    model = AVM(audio_included=True, device=DEV, precision="bf16", seed=synth.BASE_SEED)
    sd = {k: torch.from_numpy(v) for k, v in params.items()}
    sd.update(avm_ref.init_buffers())
    model.load_state_dict(sd)
    model.keep_ctx = True
    aud, vis, lab = inputs(n, h, True)
    masks = [torch.from_numpy(m) for m in synth.make_drop_masks(n, step=0)]
    loss, pred = model.train_step(aud.to(DEV), vis.to(DEV), lab.to(DEV))
    torch.cuda.synchronize()
    taps = hip_taps(model.last_ctx)
    p = {k: torch.from_numpy(v.copy()) for k, v in params.items()}
    inter = {}
    with torch.no_grad():
        avm_ref.forward(p, avm_ref.init_buffers(), aud, vis, masks, True, inter)
    e_logit = (model.last_logit.cpu() - inter["logit"].view(-1)).abs()
    print(f"[parity] bf16 mode: logit error vs fp32 CPU reference: mean {e_logit.mean():.2e}, max {e_logit.max():.2e}")
    assert e_logit.max().item() <= 1e-3
    o_loss, o_pred, o_g = avm_ref.train_step(p, avm_ref.init_buffers(), {}, aud, vis, lab, masks, True, pool_taps=taps)
    assert (pred.cpu().view(-1, 1) - o_pred).abs().max().item() <= 2e-3
    worst = 0.0
    bad = []
    for k, og in o_g.items():
        if _is_reduction_grad(k):
            continue
        mine = model.grad_of(k).cpu().reshape(og.shape)
        rel = (mine - og).abs().max().item() / max(og.abs().max().item(), 1e-30)
        l2 = ((mine - og).norm() / og.norm().clamp_min(1e-30)).item()
        print(f"[parity] bf16 mode: {k:26s} max-err/max|g| {rel:.2e}   relative L2 error {l2:.2e}")
        worst = max(worst, rel)
        bad.append(k) if l2 > 0.15 else None
    print(f"[parity] bf16 mode: worst weight-gradient error (of max|g|, device routing): {worst:.2e}")
    assert not bad, f"bf16-mode gradients with relative L2 error > 0.15: {bad}"


def test_bf16_weight_shadow_follows_every_writer_of_the_arena():
    """precision="bf16", > 16 rows: the fused Adam refreshes the bf16 copy of linear5.weight; a stock optimizer step,
    load_state_dict or an in-place edit must invalidate it (the arena's version counter does)."""
    n, h = 20, 40
    aud, vis, lab = inputs(n, h, True)
    a, b = (load_model(h, True, dropout="off")[0] for _ in range(2))
    for m in (a, b):
        m.precision = "bf16"
    ag, vg, lg = aud.to(DEV), vis.to(DEV), lab.to(DEV)
    for _ in range(3):
        a.train_step(ag, vg, lg)                       # a: shadow refreshed by Adam
        b.train_step(ag, vg, lg)
        b._w5b_version = None                          # b: forced to re-cast the fp32 master every step
    torch.cuda.synchronize()
    assert torch.equal(a._w5b, b._w5_bf16(a._w5b.numel() // 512))
    for k, v in a.state_dict().items():
        assert torch.equal(v, b.state_dict()[k]), k
    # an external writer: stock torch Adam on the Parameters
    opt = torch.optim.Adam(a.parameters(), lr=1e-3)
    out = a(aud, vis)
    torch.nn.functional.mse_loss(out[:, 0], lab).backward()
    before = a._w5b.clone()
    opt.step()
    fresh = a._w5_bf16(a._w5b.numel() // 512)
    assert not torch.equal(before, fresh)
    assert torch.equal(fresh, a._pflat("visbl.linear5.weight").to(torch.bfloat16))


def test_bf16_mode_on_frames_wider_than_the_fused_backward_serves():
    """precision="bf16" on 40 x 430 frames: the conv outputs of blocks 2 and 3 are 143 / 141 pixels wide, beyond the 138 the
    fused bf16 BatchNorm/pool backward holds in LDS — forward and backward must take the fp32 kernels for those blocks
    (the reference's Lazy layers accept any size) instead of failing after the forward."""
    n, h, w = 4, 40, 430
    torch.manual_seed(5)
    model = AVM(audio_included=True, device=DEV, precision="bf16", seed=synth.BASE_SEED)
    model.keep_ctx = True
    vis = torch.from_numpy(synth.make_visual(n, h, w))
    aud = torch.from_numpy(synth.make_audio(n))
    lab = torch.from_numpy(synth.make_labels(n))
    (_, _), (_, wp1), (_, wp2), (hp3, wp3) = model._sizes(h, w)
    assert not AVM._bwd16_ok(wp1) and not AVM._bwd16_ok(wp2)
    model._materialize(hp3 * wp3, 8)
    sd = model.state_dict()
    p = {k: v for k, v in sd.items() if v.is_floating_point() and "running" not in k}
    b = {k: v.clone() for k, v in sd.items() if k not in p}
    loss, pred = model.train_step(aud.to(DEV), vis.to(DEV), lab.to(DEV))
    torch.cuda.synchronize()
    taps = hip_taps(model.last_ctx)
    masks = [torch.from_numpy(m) for m in synth.make_drop_masks(n, step=0)]
    inter = {}
    with torch.no_grad():
        avm_ref.forward(p, {k: v.clone() for k, v in b.items()}, aud, vis, masks, True, inter)
    e = (model.last_logit.cpu() - inter["logit"].view(-1)).abs().max().item()
    print(f"[parity] bf16 mode, 40x430 frames: logit max error {e:.2e}")
    assert e <= 1e-3
    o_loss, o_pred, o_g = avm_ref.train_step(p, b, {}, aud, vis, lab, masks, True, pool_taps=taps)
    for k, og in o_g.items():
        if _is_reduction_grad(k):
            continue
        mine = model.grad_of(k).cpu().reshape(og.shape)
        l2 = ((mine - og).norm() / og.norm().clamp_min(1e-30)).item()
        assert l2 <= 0.15, f"{k}: relative L2 error {l2:.3f}"


@pytest.mark.parametrize("precision", ["bf16x6", "fp16x3"])
def test_backward_refuses_split_operands_a_second_forward_overwrote(precision, monkeypatch):
    """precision="bf16x6" / "fp16x3" at 13 frames of 224 x 224, the fewest at which conv2 and conv3 both run on split operands:
    backward reads the split activations the forward left in the cached padded buffers. A second training-mode forward
    overwrites them; the backward of the first must raise, naming the model's precision, instead of using the wrong operands — and
    before its first launch."""
    n, h = 13, 224
    torch.manual_seed(5)
    model = AVM(audio_included=True, device=DEV, precision=precision, seed=synth.BASE_SEED)
    vis = torch.from_numpy(synth.make_visual(n, h, h)).to(DEV)
    aud = torch.from_numpy(synth.make_audio(n)).to(DEV)
    _, ctx = model.forward_device(aud, vis, save=True)
    assert "x2s" in ctx, "conv3 did not run on split operands: the test would be vacuous"
    model.forward_device(aud, vis, save=True)
    dout = torch.ones(n, device=DEV)
    calls = _record_ops_calls(monkeypatch)
    with pytest.raises(RuntimeError, match=f"precision='{precision}'.*overwrote the saved split operands"):
        model.backward_device(ctx, dout)
    assert calls == [], f"refused after {len(calls)} launches: {calls[:4]}"
    torch.cuda.synchronize()


def _record_ops_calls(monkeypatch):
    """every public function of ops behind a recorder: the returned list holds the name of each call made from here on"""
    import types
    calls = []

    def wrap(name, fn):
        def wrapped(*a, **k):
            calls.append(name)
            return fn(*a, **k)
        return wrapped
    for name, fn in list(vars(ops).items()):
        if isinstance(fn, types.FunctionType) and not name.startswith("_"):
            monkeypatch.setattr(ops, name, wrap(name, fn))
    return calls


def test_backward_refusals_precede_the_first_launch(monkeypatch):
    """precision="bf16", 10 frames of 40 x 40 (a forked step: its first launch is the weight flip on the side stream): the backward of a
    ctx whose saved 16-bit operands a second forward overwrote is refused before anything is enqueued or allocated — no ops call, no
    gradient arena, nothing pending on the side stream; the next forward + backward gives the bits of a fresh model's."""
    import _freeze_case as FC
    from _mode_case import fixture
    fx = fixture("regression", True, "train", 10)
    aud, vis = fx["aud"].to(DEV), fx["vis"].to(DEV)
    dout = torch.ones(10, device=DEV)
    m, fresh = FC.load_model(fx, precision="bf16"), FC.load_model(fx, precision="bf16")
    _, ctx = m.forward_device(aud, vis, save=True)
    m.forward_device(aud, vis, save=True)
    calls = _record_ops_calls(monkeypatch)
    with pytest.raises(RuntimeError, match="precision='bf16'.*overwrote the saved bf16 operands"):
        m.backward_device(ctx, dout)
    assert calls == [], calls
    monkeypatch.undo()
    assert m._garena is None
    torch.cuda.synchronize()
    outs = []
    for k in (m, fresh):
        out, ctx = k.forward_device(aud, vis, save=True)
        k.backward_device(ctx, dout)
        outs.append(out)
    torch.cuda.synchronize()
    assert m._side_stream is not None, "the step did not fork: the test would not see a pending side stream"
    assert torch.equal(outs[0], outs[1]) and torch.equal(m._garena, fresh._garena)


def test_an_inputs_only_backward_keeps_gemm_sized_gradients_out_of_scratch(monkeypatch):
    """input_gradients trains nothing, so every parameter gradient a fused kernel cannot omit goes to the pass's scratch. The launches
    that write a GEMM-sized gradient (conv2 / conv3 / linear5 weights) are issued for trained tensors only, so scratch is never asked
    for one: it holds small tensors alone, and the arena is not even allocated."""
    import _freeze_case as FC
    from _mode_case import fixture
    from cvml_goalnet_amd import avm
    fx = fixture("regression", True, "train", 10)
    m = FC.load_model(fx)
    made, init = [], avm._Bwd.__init__

    def spy(self, *a):
        init(self, *a)
        made.append(self)
    monkeypatch.setattr(avm._Bwd, "__init__", spy)
    d_aud, d_vis = m.input_gradients(fx["aud"], fx["vis"])
    torch.cuda.synchronize()
    (bwd,) = made
    assert not bwd.train and "visbl.bnorm3.weight" in bwd.scratch and m._garena is None
    assert d_vis.abs().max().item() > 0, "the data-gradient chain ran through conv3 and conv2"
    for name in bwd.scratch:
        assert m.spec(name).kind not in ("ohwi", "lin5"), f"scratch holds the GEMM-sized gradient of {name}"
