"""GPU: the graph-captured per-video sub-batch loop (reference loop main.py:169-198).

  * the device-counter kernels produce the same bits as their host-scalar twins,
  * VideoTrainer (one HIP-graph launch per sub-batch) == the eager sequence of train_step calls, bit for bit,
    including a ragged last sub-batch and a second video (graphs replayed with new data),
  * three consecutive graph-driven steps reproduce the reference's golden vectors (avm_a1_n10_h40_mask3:
    predictions and losses of every step, parameters after the third Adam update).
"""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import eval_ref  # noqa: E402
from _golden import Golden  # noqa: E402
from cvml_goalnet_amd import AVM, ops, synth  # noqa: E402
from cvml_goalnet_amd.loop import VideoTrainer  # noqa: E402
from oracle import avm_ref  # noqa: E402

DEV = "cuda:0"
LR = 1e-3


def load_model(h, audio, precision="fp32", head="regression", w=None, bins=30):
    w = h if w is None else w
    params = eval_ref.classifier_params(h, audio, w=w, bins=bins) if head == "classifier" else synth.make_params(h, w, bins, audio)
    m = AVM(audio_included=audio, device=DEV, precision=precision, seed=synth.BASE_SEED, head=head)
    sd = {k: torch.from_numpy(v) for k, v in params.items()}
    sd.update(avm_ref.init_buffers())
    m.load_state_dict(sd)
    return m


def test_device_counter_kernels_match_their_host_scalar_twins():
    dev = DEV
    ctr = torch.zeros(4, dtype=torch.int64, device=dev)
    ops.counter_add(ctr[1], 5)
    ops.counter_add(ctr[1], -2)
    assert ctr.tolist() == [0, 3, 0, 0]
    # dropout: five masks in one launch == five goalnet_dropout_mask launches == numpy
    n, widths = 7, (512, 512, 512, 256, 128)
    buf = torch.empty(n * sum(widths), dtype=torch.float32, device=dev)
    got = ops.dropout_masks_dev(buf, n, widths, synth.BASE_SEED, synth.TID_DROP, 8, ctr[1], synth.DROP_P)
    ref_np = synth.make_drop_masks(n, step=3)
    for l, wdt in enumerate(widths):
        one = ops.dropout_mask(torch.empty(n, wdt, dtype=torch.float32, device=dev), synth.BASE_SEED, synth.TID_DROP + 8 * 3 + l, synth.DROP_P)
        assert torch.equal(got[l], one)
        assert np.array_equal(got[l].cpu().numpy(), ref_np[l])
    # a data-parallel shard draws ITS rows of the same masks: rows [4, 7) of the 7-row masks
    got3 = ops.dropout_masks_dev(torch.empty(3 * sum(widths), dtype=torch.float32, device=dev), 3, widths, synth.BASE_SEED,
                                 synth.TID_DROP, 8, ctr[1], synth.DROP_P, row_offset=4)
    for l in range(len(widths)):
        assert torch.equal(got3[l], got[l][4:7])
    # Adam: step read from device == step passed from the host, three steps
    g = torch.Generator().manual_seed(1)
    cnt = 1003
    p0 = torch.randn(cnt, generator=g).to(dev)
    pa, pb = p0.clone(), p0.clone()
    ma, va, mb, vb = (torch.zeros(cnt, device=dev) for _ in range(4))
    t = torch.zeros(1, dtype=torch.int64, device=dev)
    for s in range(1, 4):
        gr = torch.randn(cnt, generator=g).to(dev)
        ops.adam_step(pa, gr, ma, va, LR, 0.9, 0.999, 1e-8, s, 0.5)
        ops.counter_add(t[0], 1)
        ops.adam_step_dev(pb, gr, mb, vb, LR, 0.9, 0.999, 1e-8, t[0], 0.5)
        assert torch.equal(pa, pb) and torch.equal(ma, mb) and torch.equal(va, vb)
    # rows gather / scatter at a device cursor
    table = torch.arange(20 * 6, dtype=torch.float32, device=dev).view(20, 2, 3)
    cur = torch.tensor([4], dtype=torch.int64, device=dev)
    blk = torch.empty(5, 2, 3, dtype=torch.float32, device=dev)
    ops.rows_gather(table, blk, 5, cur[0])
    assert torch.equal(blk, table[4:9])
    out = torch.zeros(20, 2, 3, dtype=torch.float32, device=dev)
    ops.rows_scatter(blk, out, 5, cur[0])
    assert torch.equal(out[4:9], table[4:9]) and out[:4].abs().sum() == 0 and out[9:].abs().sum() == 0
    vec = torch.zeros(20, dtype=torch.float32, device=dev)
    ops.rows_scatter(torch.tensor([7.0], device=dev), vec, 1, cur[0])
    assert vec[4] == 7 and vec.sum() == 7
    # several segments in one launch, with a cursor bias; four counters in one launch
    blk2 = torch.empty(3, 2, 3, dtype=torch.float32, device=dev)
    vec2 = torch.zeros(20, dtype=torch.float32, device=dev)
    ops.rows_copy_batch([(table, blk2, 3, cur[0], 2, True), (vec2, torch.tensor([1.0, 2.0], device=dev), 2, cur[0], -4, False)])
    assert torch.equal(blk2, table[6:9]) and vec2[0] == 1 and vec2[1] == 2 and vec2.sum() == 3
    ops.counters_add4(ctr, 1, 2, 3, -4)
    assert ctr.tolist() == [1, 5, 3, -4]
    # Adam with a step bias: counter holds the completed steps
    t0 = torch.tensor([2], dtype=torch.int64, device=dev)
    pc, mc, vc = p0.clone(), torch.zeros(cnt, device=dev), torch.zeros(cnt, device=dev)
    pd, md, vd = p0.clone(), torch.zeros(cnt, device=dev), torch.zeros(cnt, device=dev)
    ops.adam_step(pc, gr, mc, vc, LR, 0.9, 0.999, 1e-8, 3, 1.0)
    ops.adam_step_dev(pd, gr, md, vd, LR, 0.9, 0.999, 1e-8, t0[0], 1.0, step_bias=1)
    assert torch.equal(pc, pd)


def _video(n, h, audio, salt, w=None, bins=30):
    vis = torch.from_numpy(synth.make_visual(n, h, h if w is None else w, seed=synth.BASE_SEED + salt))
    aud = torch.from_numpy(synth.make_audio(n, bins, seed=synth.BASE_SEED + salt)) if audio else [None] * n
    lab = torch.from_numpy(synth.make_labels(n, seed=synth.BASE_SEED + salt))
    return aud, vis, lab


def _loop_counts(frames, sb):
    """(eager steps, graph replays) of VideoTrainer on videos of `frames` frames with nobody writing the model in between: a sub-batch
    size runs eagerly the first time it occurs (allocations), is captured the second time, and is a replay from then on"""
    seen, eager, replays = set(), 0, 0
    for f in frames:
        for off in range(0, f, sb):
            n = min(sb, f - off)
            eager, replays = (eager, replays + 1) if n in seen else (eager + 1, replays)
            seen.add(n)
    return eager, replays


@pytest.mark.parametrize("audio,precision,head,sb", [
    pytest.param(True, "fp32", "regression", 10, id="True-fp32"), pytest.param(False, "fp32", "regression", 10, id="False-fp32"),
    pytest.param(True, "bf16", "regression", 10, id="True-bf16"), pytest.param(False, "bf16", "regression", 10, id="False-bf16"),
    pytest.param(True, "fp16", "regression", 10, id="True-fp16"), pytest.param(False, "fp16", "regression", 10, id="False-fp16"),
    pytest.param(True, "fp32", "classifier", 10, id="True-fp32-classifier"),
    pytest.param(False, "bf16", "classifier", 10, id="False-bf16-classifier"),
    # sub-batches of 20 (> 16 rows): the captured graph holds the 16-bit linear5 / p3 / y3 kernels and the shadowed Adam
    pytest.param(True, "bf16", "regression", 20, id="True-bf16-sb20"), pytest.param(True, "fp16", "regression", 20, id="True-fp16-sb20")])
def test_graph_loop_equals_eager_train_steps_bit_for_bit(audio, precision, head, sb):
    # sb = 10: 4x10 + 7, then 3x10 + 3: sizes 10, 7, 3 ran eagerly once each, 6 replays; sb = 20: 2x20 + 7, then 20 + 13
    _graph_loop_vs_eager(audio, precision, head, sb, (40, 40), (47, 33), {10: (3, 6), 20: (3, 2)}[sb], [sb])


def test_graph_loop_equals_eager_train_steps_bit_for_bit_on_non_square_frames():
    """two videos of 23 frames, 64 high and 40 wide: the staging tables are (cap, 3, 64, 40), and both the 10-row and the 3-row step are
    captured (each size runs eagerly once, is captured at its second occurrence and replayed from then on) — on a square frame a table
    or a gathered sub-batch laid out (W, H) holds the same bytes"""
    tr = _graph_loop_vs_eager(True, "fp32", "regression", 10, (64, 40), (23, 23), (2, 4), [3, 10])
    assert tr._key == ((64, 40), 30) and tr._vid.shape[1:] == (3, 64, 40)


def _graph_loop_vs_eager(audio, precision, head, sb, hw, frames, counts, captured, bins=None):
    """VideoTrainer against the eager sequence of train_step calls on videos of `frames` frames of hw = (H, W): losses, predictions,
    the state dict, the counters and the Adam moments bit for bit; `counts` = the (eager steps, replays) the caller worked out by
    hand, `captured` = the sub-batch sizes that end up with a graph; `bins` = the audio bin length of each video (None: 30), all with
    the l2 of the first, which sizes audbl.linear3"""
    h, w = hw
    bins = (30,) * len(frames) if bins is None else bins
    videos = [_video(f, h, audio, 1 + i, w=w, bins=b) for i, (f, b) in enumerate(zip(frames, bins))]
    eager, graphed = load_model(h, audio, precision, head, w=w, bins=bins[0]), load_model(h, audio, precision, head, w=w, bins=bins[0])
    tr = VideoTrainer(graphed, subbatch_size=sb, lr=LR)
    for aud, vis, lab in videos:
        # eager: the reference's loop, main.py:177-196, on GPU tensors
        e_loss, e_pred = [], []
        for a in range(0, vis.shape[0], sb):
            b = min(a + sb, vis.shape[0])
            loss, pred = eager.train_step(aud[a:b].to(DEV) if audio else None, vis[a:b].to(DEV), lab[a:b].to(DEV), lr=LR)
            e_loss.append(loss)
            e_pred.append(eager.predict_classes(pred) if head == "classifier" else pred)     # main.py:190: argmax + 1 is collected
        losses, preds = tr.train_video(aud, vis, lab)
        torch.cuda.synchronize()
        assert torch.equal(losses, torch.cat(e_loss))
        assert torch.equal(preds, torch.cat(e_pred))
    want_eager, want_replays = _loop_counts(frames, sb)
    steps = want_eager + want_replays
    assert (want_eager, want_replays) == counts
    assert tr.replays == want_replays and tr.eager_steps == want_eager, (tr.replays, tr.eager_steps)
    assert sorted(k[0] for k in tr._graphs) == captured, "the sub-batch sizes that occurred at least twice are the captured graphs"
    assert any(tr._uses_w5b.values()) == (sb > 16 and precision != "fp32"), "a graph of > 16 rows of a 16-bit mode reads the 16-bit weights"
    sd_e, sd_g = eager.state_dict(), graphed.state_dict()
    for k in sd_e:
        assert torch.equal(sd_e[k], sd_g[k]), k
    assert graphed._state.tolist()[:2] == [steps, steps] and graphed._adam_t == steps and graphed._drop_step == steps
    assert torch.equal(graphed._adam_m, eager._adam_m) and torch.equal(graphed._adam_v, eager._adam_v)
    if precision == "fp16":
        assert graphed._guard.tolist() == [0, 0] and eager._guard.tolist() == [0, 0]
    return tr


@pytest.mark.parametrize("precision", ["bf16", "fp16"])
def test_16bit_graph_of_a_small_sub_batch_keeps_the_16bit_weight_copy_fresh(precision):
    """Two 7-frame videos first: the 7-row step (fp32 weight-streaming linear5) is captured BEFORE the 16-bit copy of linear5.weight
    exists, so that graph's fused Adam updates the fp32 master only. Then 47 frames in sub-batches of 20: the 20-row steps create the
    copy and keep it fresh through their own shadowed Adam, the 7-row tail follows them, and the next 20-row step reads the copy. The
    graph captured without the shadow must not be replayed once the copy is live (its Adam would leave the copy one step behind
    with a valid version stamp: before VideoTrainer captured such a size again, the last video's loss differed from the eager one
    in the fourth digit); compared bit for bit with eager train_step calls, whose Adam looks at the copy on every step."""
    h, sb, frames = 40, 20, (7, 7, 47, 20)
    eager, graphed = load_model(h, True, precision), load_model(h, True, precision)
    tr = VideoTrainer(graphed, subbatch_size=sb, lr=LR)
    for vi, f in enumerate(frames):
        aud, vis, lab = _video(f, h, True, 30 + vi)
        e_loss, e_pred = [], []
        for a in range(0, f, sb):
            b = min(a + sb, f)
            loss, pred = eager.train_step(aud[a:b].to(DEV), vis[a:b].to(DEV), lab[a:b].to(DEV), lr=LR)
            e_loss.append(loss); e_pred.append(pred)
        losses, preds = tr.train_video(aud, vis, lab)
        torch.cuda.synchronize()
        assert torch.equal(losses, torch.cat(e_loss)), f"video {vi}"
        assert torch.equal(preds, torch.cat(e_pred)), f"video {vi}"
    sd_e, sd_g = eager.state_dict(), graphed.state_dict()
    for k in sd_e:
        assert torch.equal(sd_e[k], sd_g[k]), k
    assert torch.equal(graphed._w5b, eager._w5b), "the 16-bit copy of linear5.weight"
    # 7 (eager), 7 (captured without the shadow), 20 (eager), 20 (captured), 7 (the copy is live: captured again, with it), 20 (replay)
    assert tr.eager_steps == 2 and tr.replays == 4, (tr.eager_steps, tr.replays)
    assert all(tr._shadows.values()) and len(tr._graphs) == 2


def test_bf16_graph_loop_survives_writers_outside_the_graph():
    """precision="bf16" with sub-batches of 20 frames (> 16: linear5 reads the bf16 copy of its weights, which a captured
    graph keeps fresh through its own fused Adam but never re-casts). A load_state_dict between two videos, and an in-place
    edit of the Parameter, happen outside the graph: the next sub-batch must not run on the stale copy. Compared bit for
    bit with eager train_step calls subjected to the same writers."""
    h, sb = 40, 20
    eager, graphed = load_model(h, True, "bf16"), load_model(h, True, "bf16")
    tr = VideoTrainer(graphed, subbatch_size=sb, lr=LR)
    other = {k: torch.from_numpy(v) for k, v in synth.make_params(h, h, 30, True, seed=synth.BASE_SEED + 99).items()}
    other.update(avm_ref.init_buffers())
    for vi in range(3):
        aud, vis, lab = _video(60, h, True, 10 + vi)                      # 3 x 20
        if vi == 1:
            for m in (eager, graphed):
                m.load_state_dict(other)                                  # main.py:66 between two videos
        if vi == 2:
            for m in (eager, graphed):
                with torch.no_grad():
                    m.visbl.linear5.weight.mul_(0.5)                      # any in-place writer of the Parameter
        e_loss, e_pred = [], []
        for a in range(0, 60, sb):
            loss, pred = eager.train_step(aud[a:a + sb].to(DEV), vis[a:a + sb].to(DEV), lab[a:a + sb].to(DEV), lr=LR)
            e_loss.append(loss); e_pred.append(pred)
        losses, preds = tr.train_video(aud, vis, lab)
        torch.cuda.synchronize()
        assert torch.equal(losses, torch.cat(e_loss)), f"video {vi}"
        assert torch.equal(preds, torch.cat(e_pred)), f"video {vi}"
    assert graphed.last_used_w5b and tr.replays >= 5 and tr.eager_steps == 3      # first step + one re-validating step per writer
    sd_e, sd_g = eager.state_dict(), graphed.state_dict()
    for k in sd_e:
        assert torch.equal(sd_e[k], sd_g[k]), k


@pytest.mark.parametrize("precision,large", [("fp32", False), ("bf16", False), ("fp16", False), ("fp32", True), ("bf16", True)])
def test_side_stream_overlap_changes_nothing_but_the_schedule(precision, large):
    """Small steps fork their weight-gradient / bias-gradient / AudBl kernels onto a second HIP stream (avm._Fork). Same kernels,
    same order inside every dependency chain: eager and graph-driven results must equal the single-stream run bit for bit."""
    h, sb = 40, 10
    aud, vis, lab = _video(47, h, True, 21)
    ref, forked = load_model(h, True, precision), load_model(h, True, precision)
    ref.overlap_rows, ref.overlap_large, ref.overlap_auto = 0, False, False      # everything on the current stream, Adam after backward
    forked.overlap_large = large                                          # True: also the early Adam on linear5.weight (off by default)
    e_loss, e_pred = [], []
    for a in range(0, 47, sb):
        loss, pred = ref.train_step(aud[a:a + sb].to(DEV), vis[a:a + sb].to(DEV), lab[a:a + sb].to(DEV), lr=LR)
        e_loss.append(loss); e_pred.append(pred)
    tr = VideoTrainer(forked, subbatch_size=sb, lr=LR)
    losses, preds = tr.train_video(aud, vis, lab)
    torch.cuda.synchronize()
    assert forked._side_stream is not None and ref._side_stream is None
    assert torch.equal(losses, torch.cat(e_loss)) and torch.equal(preds, torch.cat(e_pred))
    sd_r, sd_f = ref.state_dict(), forked.state_dict()
    for k in sd_r:
        assert torch.equal(sd_r[k], sd_f[k]), k
    assert torch.equal(ref._garena, forked._garena)


def test_three_graph_driven_steps_reproduce_the_reference_goldens():
    g = Golden("avm_a1_n10_h40_mask3")
    assert g.steps == 3 and g.n == 10
    model = load_model(g.h, True)
    aud = torch.from_numpy(synth.make_audio(g.n)).repeat(3, 1, 1)     # the golden feeds the same ten frames three times
    vis = torch.from_numpy(synth.make_visual(g.n, g.h, g.h)).repeat(3, 1, 1, 1)
    lab = torch.from_numpy(synth.make_labels(g.n)).repeat(3)
    tr = VideoTrainer(model, subbatch_size=10, lr=LR)
    losses, preds = tr.train_video(aud, vis, lab)
    torch.cuda.synchronize()
    assert tr.replays == 2 and tr.eager_steps == 1
    for s in range(3):
        g.check(f"s{s}.pred", preds[10 * s:10 * s + 10], rtol=0.0, atol=2e-5)
        g.check(f"s{s}.loss", losses[s:s + 1], rtol=2e-5)
    sd = model.state_dict()
    for k in g.keys("s2.param."):
        name = k.split("param.", 1)[1]
        idx, ref = g.samples(k)
        err = np.abs(g.flat(sd[name])[idx] - ref)
        # Adam divides by sqrt(v): where a gradient is ~zero (biases in front of a BatchNorm, dead units) its rounding
        # noise becomes a +-lr kick per step (test_gpu_avm.py carries the elementwise bound). Here: the hard bound of
        # three kicks for every sampled element, and fp32-rounding agreement for the bulk of each tensor.
        assert err.max() <= 3 * 2 * LR, f"{k}: {err.max():.3e}"
        assert np.median(err) <= 1e-5, f"{k}: median error {np.median(err):.3e}"
    for k in g.keys("s2.buf."):
        g.check(k, sd[k.split("buf.", 1)[1]], rtol=1e-5, atol=0.1 * 2 * LR * 2, what=" (BatchNorm buffer)")


def test_trainer_input_validation_and_table_growth():
    model = load_model(40, True)
    tr = VideoTrainer(model, subbatch_size=10, graphs=True)
    aud, vis, lab = _video(12, 40, True, 3)
    with pytest.raises(RuntimeError):
        tr.train_video(aud, vis, lab[:5])
    with pytest.raises(RuntimeError):
        tr.train_video(aud[:, :20], vis, lab)
    l1, p1 = tr.train_video(aud, vis, lab)
    assert l1.shape == (2,) and p1.shape == (12,)
    aud, vis, lab = _video(130, 40, True, 4)          # larger than the first table: tables and graphs are rebuilt
    l2, p2 = tr.train_video(aud, vis, lab)
    torch.cuda.synchronize()
    assert l2.shape == (13,) and p2.shape == (130,)
    assert torch.isfinite(l2).all() and ((p2 > 1) & (p2 < 5)).all()


def test_eval_video_matches_the_oracle_forward_and_broadcast_loss():
    """main.py:218-226: whole video, no_grad, train-mode BatchNorm (buffers move), (n,1) x (n,) MSE"""
    n, h = 23, 40
    model = load_model(h, True)
    model.dropout_mode = "off"
    aud, vis, lab = _video(n, h, True, 5)
    tr = VideoTrainer(model)
    loss, pred = tr.eval_video(aud, vis, lab)
    p = {k: torch.from_numpy(v) for k, v in synth.make_params(h, h, 30, True).items()}
    b = avm_ref.init_buffers()
    with torch.no_grad():
        want = avm_ref.forward(p, b, aud, vis, None, True, {})
    assert (pred.cpu() - want.view(-1)).abs().max().item() < 2e-5
    assert abs(loss.item() - avm_ref.mse_bcast(want, lab).item()) < 2e-5
    sd = model.state_dict()
    for k, v in b.items():                                               # running statistics were updated, as in the reference
        assert torch.allclose(sd[k].double(), v.double(), rtol=1e-5, atol=1e-6), k


@pytest.mark.parametrize("n,audio", [(10, True), (16, True), (3, False)])
def test_small_step_one_launch_kernels_match_the_multi_launch_forms(n, audio, monkeypatch):
    """Round 3, the reference's operating point (<= 16 frames of 40 x 40): the fusion MLP forward / backward as one launch each
    (csrc/mlp.hip, grid barriers over sc1 hand-offs), the pool / BatchNorm passes with their finalise step folded in
    (csrc/pool_bn.hip "small shapes"), the one-launch Conv1d backward, the batched weight flips and bias-gradient sums, and the
    scatter + counter tick in the step's last launch. The same two steps with every one of them switched off
    (GOALNET_MLP_FUSED=0, GOALNET_SMALL_BN=0: the multi-launch kernels of rounds 1-2) must give the same predictions, losses,
    gradients and parameters up to fp32 summation order; no grid barrier may have timed out."""
    h = 40
    vis = torch.from_numpy(synth.make_visual(n, h, h)).to(DEV)
    aud = torch.from_numpy(synth.make_audio(n)).to(DEV) if audio else None
    lab = torch.from_numpy(synth.make_labels(n)).to(DEV)

    def two_steps():
        m = load_model(h, audio)
        out = []
        for _ in range(2):
            loss, pred = m.train_step(aud, vis, lab)
            out.append((loss.clone(), pred.clone(), m._garena.clone()))
        torch.cuda.synchronize()
        return m, out

    fused_m, fused = two_steps()
    assert not ops.mlp_sync_error(torch.device(DEV), n, 640 if audio else 512), "a grid barrier of the fused MLP kernels timed out"
    monkeypatch.setenv("GOALNET_MLP_FUSED", "0")
    monkeypatch.setenv("GOALNET_SMALL_BN", "0")
    plain_m, plain = two_steps()
    for s, ((lf, pf, gf), (lp, pp, gp)) in enumerate(zip(fused, plain)):
        assert (pf - pp).abs().max().item() <= 2e-6, f"step {s}: predictions"
        assert abs(lf.item() - lp.item()) <= 2e-6 * max(1.0, abs(lp.item())), f"step {s}: loss"
        for sp in fused_m._specs:
            a, b = gf[sp.offset:sp.offset + sp.numel], gp[sp.offset:sp.offset + sp.numel]
            scale = max(b.abs().max().item(), 1e-30)
            tol = 2e-5 if (sp.name.endswith(".bias") or ".bnorm" in sp.name) else 5e-6      # cancelling sums (test_gpu_avm._is_reduction_grad)
            assert (a - b).abs().max().item() <= tol * scale + 1e-9, f"step {s}: gradient of {sp.name}"
    # after two Adam steps: inside the first-order sensitivity bound of the gradient differences (near-zero gradients turn into +-lr kicks)
    d = (fused_m._arena - plain_m._arena).abs().max().item()
    assert d <= 2 * 2 * LR, f"parameters differ by {d}"
    assert torch.equal(fused_m._state[:2], plain_m._state[:2])


@pytest.mark.parametrize("precision", ["fp32", "fp16"])
def test_a_refused_step_leaves_no_residue(precision):
    """10 frames of 40 x 40: a train_step that forward_device refuses (audio of the wrong shape, before any launch) leaves nothing behind
    on the model — the two good steps that follow equal a fresh model's two steps bit for bit, and the forward right after the refusal
    ticks its dropout draw itself (the tick is not left to a caller that never comes)."""
    import _freeze_case as FC
    from _mode_case import fixture
    fx = fixture("regression", True, "train", 10)
    aud, vis, lab = fx["aud"].to(DEV), fx["vis"].to(DEV), fx["lab"].to(DEV)
    bad_aud = torch.zeros(10, 29, 30, device=DEV)

    def model():
        m = FC.load_model(fx, True, precision)
        m.dropout_mode = "device"                     # counter-based masks: a draw that is not ticked would repeat
        return m

    def two_steps(m):
        out = [tuple(t.clone() for t in m.train_step(aud, vis, lab, lr=LR)) for _ in range(2)]
        torch.cuda.synchronize()
        return out

    a, b, c = model(), model(), model()
    for m in (a, c):
        with pytest.raises(RuntimeError, match="audio_input must be"):
            m.train_step(bad_aud, vis, lab, lr=LR)
    draws = int(c._state[1])
    with torch.no_grad():
        c(aud, vis)
    assert int(c._state[1]) == draws + 1, "the draw of the forward after a refused step was not ticked"
    for s, ((la, pa), (lb, pb)) in enumerate(zip(two_steps(a), two_steps(b))):
        assert torch.equal(la, lb) and torch.equal(pa, pb), f"step {s}"
    for k in ("_arena", "_garena", "_state") + (("_guard",) if precision == "fp16" else ()):
        assert torch.equal(getattr(a, k), getattr(b, k)), k
    assert int(a._state[1]) == 2, "each good step ticked its draw once"
