"""GPU: gradient accumulation on the fused step at model level: AVM.train_step(accumulate=k) and
loop.VideoTrainer(accumulate=k) on 40 x 40 frames with audio. The accumulator is held BIT FOR BIT against the CPU restatement
(tests/_accum_case.restate: t = g * (float)(1 / k); acc + t) built from the device's own gradient-arena snapshots, which isolates the
accumulation from the backward's rounding; an update is held against torch's optimizer on the CPU started from the device's own
pre-step state and accumulator, under the bound of tests/test_gpu_optim_step.py: |p - p_ref| <= 2e-7 + t 2^-23 |p_ref|. The independent
check compares a window with the larger batch where the two agree mathematically, under the project's gradient rule (grad_verdict)."""
import math

import pytest
import torch

pytestmark = pytest.mark.gpu

if not torch.cuda.is_available():
    pytest.skip("no GPU", allow_module_level=True)

import _accum_case as AC                                             # noqa: E402
import ema_ref as R                                                  # noqa: E402
from _abi_guard import bits_equal                                   # noqa: E402
from _freeze_case import flat, load_model                           # noqa: E402
from cvml_goalnet_amd import EmaOptions, GoalnetError              # noqa: E402
from cvml_goalnet_amd.avm import epi_fuse_dw_adam, epi_fuse_pieces  # noqa: E402
from cvml_goalnet_amd.loop import VideoTrainer                      # noqa: E402
from test_gpu_ema_step import _assert_within_bound, _trainable_mask  # noqa: E402
from test_gpu_optim_step import BETAS, EPS, LR, W5, _cpu_slices, _data, _model, _options, _ratio, _torch_step   # noqa: E402

DEV = "cuda:0"


def _names(model):
    return [s.name for s in model._specs]


def _moments(model, names, like):
    if model._adam_m is None:                                        # before the first optimizer step the moments are zero
        return ({k: torch.zeros_like(x) for k, x in like.items()} for _ in range(2))
    return _cpu_slices(model, model._adam_m, names), _cpu_slices(model, model._adam_v, names)


def _adam_ref(names, p0, g, m0, v0, t):
    """p after step t of torch.optim.Adam(foreach=False) started from (p0, m0, v0, t - 1 steps taken) under the gradients g"""
    prm = {k: torch.nn.Parameter(p0[k].clone()) for k in names}
    opt = torch.optim.Adam([prm[k] for k in names], lr=LR, betas=BETAS, eps=EPS, foreach=False)
    for k in names:
        prm[k].grad = g[k].clone()
        opt.state[prm[k]] = {"step": torch.tensor(float(t - 1)), "exp_avg": m0[k].clone(), "exp_avg_sq": v0[k].clone()}
    opt.step()
    return {k: q.detach() for k, q in prm.items()}


def _bn_state(model):
    return ([getattr(model.visbl, f"bnorm{i}").running_mean.clone() for i in (1, 2, 3)],
            [int(getattr(model.visbl, f"bnorm{i}").num_batches_tracked) for i in (1, 2, 3)])


# ---- 1. accumulate=1 is the step without the argument --------------------------------------------------------------------------------------
def test_accumulate_one_is_the_step_without_the_argument():
    a, b = _model(), _model()
    for t in range(3):
        aud, vis, lab = _data(10, 20 + t)
        la, pa = a.train_step(aud, vis, lab, lr=LR)
        lb, pb = b.train_step(aud, vis, lab, lr=LR, accumulate=1)
        torch.cuda.synchronize()
        assert bits_equal(la, lb) and bits_equal(pa, pb), t
        for x, y, what in ((a._arena, b._arena, "arena"), (a._garena, b._garena, "gradients"), (a._adam_m, b._adam_m, "m"), (a._adam_v, b._adam_v, "v")):
            assert bits_equal(x, y), (t, what)
        assert b._gacc is None and b.accum_position == (0, 1)
    assert a._state.tolist() == b._state.tolist() and a._adam_t == b._adam_t == 3 and a._drop_step == b._drop_step


# ---- 2. two windows of k = 3 -----------------------------------------------------------------------------------------------------------------
def test_two_windows_of_three_micro_steps():
    k, n = 3, 4
    model = _model()
    names = _names(model)
    s5 = model.spec(W5)
    acc_ref, g5_prev, worst = None, None, 0.0
    for micro in range(2 * k):
        pos, window = micro % k, micro // k
        last = pos == k - 1
        assert model.accum_position == ((pos, k) if micro else (0, 1))
        arena0 = model._arena.clone()
        p0 = _cpu_slices(model, model._arena, names)
        m0, v0 = _moments(model, names, p0)
        mom0 = None if model._adam_m is None else (model._adam_m.clone(), model._adam_v.clone())
        state0, adam_t0 = model._state.tolist(), model._adam_t
        means0, nbt0 = _bn_state(model)
        model.train_step(*_data(n, 100 + micro), lr=LR, accumulate=k)
        torch.cuda.synchronize()
        g = model._garena.cpu()
        acc_ref = AC.restate(acc_ref, g, k, pos == 0)
        assert bits_equal(model._gacc.cpu(), acc_ref), f"micro-step {micro}: the accumulator is not the restatement's"
        g5 = g[s5.offset:s5.offset + s5.numel].clone()
        assert g5.abs().max().item() > 0 and (g5_prev is None or not bits_equal(g5, g5_prev)), f"micro-step {micro}: linear5.weight's gradient slot"
        g5_prev = g5
        assert bits_equal(model.grad_of("fusion.0.weight").cpu(), flat(model, g, "fusion.0.weight").view(512, -1)), "grad_of: the last micro-step's"
        assert bits_equal(model.accum_of("fusion.0.weight").cpu(), flat(model, acc_ref, "fusion.0.weight").view(512, -1))
        state1 = model._state.tolist()
        means1, nbt1 = _bn_state(model)
        assert state1[1] == state0[1] + 1, "the dropout counter ticks on every micro-step"
        assert nbt1 == [v + 1 for v in nbt0] and all(not bits_equal(x, y) for x, y in zip(means0, means1)), "BatchNorm buffers move on every micro-step"
        if not last:
            assert bits_equal(model._arena, arena0), f"micro-step {micro}: the parameters moved inside the window"
            if mom0 is None:
                assert model._adam_m is None or not (model._adam_m.any().item() or model._adam_v.any().item())
            else:
                assert bits_equal(model._adam_m, mom0[0]) and bits_equal(model._adam_v, mom0[1]), f"micro-step {micro}: the moments moved"
            assert state1[0] == state0[0] and model._adam_t == adam_t0
        else:
            t = window + 1
            assert state1[0] == state0[0] + 1 == t and model._adam_t == adam_t0 + 1 == t
            got = _cpu_slices(model, model._arena, names)
            ref = _adam_ref(names, p0, {q: flat(model, acc_ref, q) for q in names}, m0, v0, t)
            r = max(_ratio(got[q], ref[q], t) for q in names)
            worst = max(worst, r)
            print(f"[accum-step] window {window}: worst |p - p_ref| / bound = {r:.3f}")
            assert r <= 1.0, f"window {window}: {r:.3f} x the bound"
            assert not bits_equal(model._arena, arena0)
    assert model.accum_position == (0, k)


# ---- 3. options compose ----------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def half_norm():
    """half the norm of the first window's accumulated gradient: what max_grad_norm is set to, so that the window is clipped by ~0.5"""
    m = _model()
    for i in range(2):
        m.train_step(*_data(10, 200 + i), lr=LR, accumulate=2)
    return 0.5 * m.grad_norm().item()


def test_options_and_the_average_count_windows(half_norm):
    k = 2
    model, opt, ema = _model(), _options(half_norm), EmaOptions(decay=0.9)
    names = _names(model)
    track = R.Tracker(model._arena.cpu().numpy(), 0.9)
    acc_ref, coefs = None, []
    for window in range(2):
        t = window + 1
        lr_t = opt.lr_at(LR, window)
        p0 = _cpu_slices(model, model._arena, names)
        m0, v0 = _moments(model, names, p0)
        for pos in range(k):
            assert abs(model.current_lr(LR, opt) - lr_t) <= 8 * 2.0 ** -52 * LR, "one schedule tick per window, not per micro-step"
            ema0 = None if model._ema is None else model._ema.clone()
            model.train_step(*_data(10, 200 + k * window + pos), lr=LR, optim=opt, ema=ema, accumulate=k)
            torch.cuda.synchronize()
            acc_ref = AC.restate(acc_ref, model._garena.cpu(), k, pos == 0)
            assert bits_equal(model._gacc.cpu(), acc_ref)
            if pos < k - 1:
                assert bits_equal(model._ema, model._arena if ema0 is None else ema0), "the average moves with the window's update only"
        acc = {q: flat(model, acc_ref, q) for q in names}
        norm = math.sqrt(sum(float((x.double() ** 2).sum()) for x in acc.values()))
        assert abs(model.grad_norm().item() - norm) <= 1e-12 * norm, "grad_norm() is the accumulated gradient's"
        coefs.append(min(1.0, opt.max_grad_norm / (norm + 1e-6)))
        got = _cpu_slices(model, model._arena, names)
        ref, _ = _torch_step(names, p0, acc, m0, v0, t, lr_t, opt.decays, opt.weight_decay, opt.max_grad_norm)
        r = max(_ratio(got[q], ref[q], t) for q in names)
        print(f"[accum-step] options, window {window}: lr_t = {lr_t:.6e}, coef = {coefs[-1]:.4f}, worst |p - p_ref| / bound = {r:.3f}")
        assert r <= 1.0, f"window {window}: {r:.3f} x the bound"
        track.step(model._arena.cpu().numpy(), t)
    assert abs(coefs[0] - 0.5) < 1e-3, coefs
    assert abs(opt.lr_at(LR, 0) - LR / 2) < 1e-15 and opt.lr_at(LR, 1) == LR, "the warm-up was walked by windows"
    assert abs(model.current_lr(LR, opt) - opt.lr_at(LR, 2)) <= 8 * 2.0 ** -52 * LR
    assert model._state.tolist()[0] == 2 and model._adam_t == 2
    _assert_within_bound(model, track, _trainable_mask(model), "two windows of k = 2, decay 0.9")
    assert not bits_equal(model._ema, model._arena)


# ---- 4. the independent check: a window equals the larger batch where that holds mathematically ---------------------------------------
def test_a_window_equals_the_larger_batch_in_eval_mode():
    fx = AC.eval_fixture()
    g64, og = AC.oracle_large(fx, torch.float64), AC.oracle_large(fx, torch.float32)
    pre = AC.verdicts(AC.oracle_window(fx, torch.float32), og, g64)
    assert all(msg is None for _, msg in pre.values()), f"precondition: the oracle's own accumulated fp32 gradient fails the rule: {pre}"
    aud, vis, lab = fx["aud"].to(DEV), fx["vis"].to(DEV), fx["lab"].to(DEV)
    windowed = load_model(fx, mode="eval")
    for i in range(AC.K):
        lo, hi = i * AC.ROWS, (i + 1) * AC.ROWS
        windowed.train_step(aud[lo:hi], vis[lo:hi], lab[lo:hi], lr=LR, loss="mse", accumulate=AC.K)
    large = load_model(fx, mode="eval")
    large.train_step(aud, vis, lab, lr=LR, loss="mse")
    torch.cuda.synchronize()
    assert windowed._state.tolist()[:2] == [1, 0] == large._state.tolist()[:2], "eval(): one update each, no dropout draw"
    failures = []
    for what, mine in (("window of 3 x 6", {q: windowed.accum_of(q).cpu() for q in og}), ("one step of 18", {q: large.grad_of(q).cpu() for q in og})):
        v = AC.verdicts(mine, og, g64)
        print(f"[accum-step] {what}: distance from the fp64 18-frame gradient / allowance, per tensor (oracle's own window: "
              f"worst {max(r for r, _ in pre.values()):.3f})")
        for q, (r, msg) in v.items():
            print(f"[accum-step]     {q:24s} {r:.3f}")
            if msg:
                failures.append(f"{what}: {msg}")
    assert not failures, "\n".join(failures)


# ---- 5. VideoTrainer ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("plan", [{}, {"shuffle": True, "augment": {"flip_p": 0.5}}], ids=["in-order", "shuffled-flipped"])
def test_video_trainer_graphs_equal_eager(plan):
    """30 frames in sub-batches of 4 x 7 + 2, windows of 3, 3 and 2: three updates per pass, the last from a window of two"""
    aud, vis, lab = (x.cpu() for x in _data(30, 300))
    eager, graphed = _model(), _model()
    tr_e = VideoTrainer(eager, subbatch_size=4, lr=LR, graphs=False, accumulate=3, **plan)
    tr_g = VideoTrainer(graphed, subbatch_size=4, lr=LR, graphs=True, accumulate=3, **plan)
    for p in range(2):
        le, pe = tr_e.train_video(aud, vis, lab)
        lg, pg = tr_g.train_video(aud, vis, lab)
        torch.cuda.synchronize()
        assert le.shape == lg.shape == (8,) and pe.shape == pg.shape == (30,)
        assert bits_equal(le, lg) and bits_equal(pe, pg), p
        for a, b, what in ((eager._arena, graphed._arena, "arena"), (eager._adam_m, graphed._adam_m, "m"), (eager._adam_v, graphed._adam_v, "v"),
                           (eager._gacc, graphed._gacc, "accumulator")):
            assert bits_equal(a, b), (p, what)
        assert eager._state.tolist() == graphed._state.tolist() and eager._state.tolist()[0] == 3 * (p + 1)
        assert eager._adam_t == graphed._adam_t == 3 * (p + 1) and eager._drop_step == graphed._drop_step == 8 * (p + 1)
        assert eager.accum_position == graphed.accum_position == (0, 2), "the video ended with its window"
    assert tr_e.replays == 0 and tr_g.replays > 0
    phases = sorted(k[7] for k in tr_g._graphs)
    assert all(k[-1] is True for k in tr_g._graphs) and set(phases) <= {(True, False, 3), (False, False, 3), (False, True, 3), (True, False, 2), (False, True, 2)}
    assert {(True, False, 3), (False, False, 3), (False, True, 3)} <= set(phases), phases
    graphed.training_state()                                          # between videos: not refused


# ---- 6. the 16-bit copy of linear5.weight --------------------------------------------------------------------------------------------------------
def test_the_16bit_copy_follows_the_windows_update():
    k = 2
    model = _model("bf16")
    s5 = model.spec(W5)
    acc_ref = None
    for pos in range(k):
        w5_0 = model._arena[s5.offset:s5.offset + s5.numel].clone()
        model.train_step(*_data(32, 400 + pos), lr=LR, accumulate=k)
        torch.cuda.synchronize()
        acc_ref = AC.restate(acc_ref, model._garena.cpu(), k, pos == 0)
        assert bits_equal(model._gacc.cpu(), acc_ref), pos
        assert model._w5b is not None and model._w5b_version == model._w5_version(), "the copy is live"
        w5 = model._arena[s5.offset:s5.offset + s5.numel]
        assert bits_equal(w5, w5_0) == (pos < k - 1)
        assert bits_equal(model._w5b.reshape(-1), w5.to(torch.bfloat16)), f"micro-step {pos}: the copy is not the cast of the master"


# ---- 7. the shortcuts are off ------------------------------------------------------------------------------------------------------------------------
def test_accumulation_switches_the_fused_epilogue_off():
    model = _model()
    assert epi_fuse_dw_adam(256, plain=True, synced=False, precision="fp32", train_w5=True, shadowed=False, inspected=False, forced=None,
                            pieces=epi_fuse_pieces(None)), "without accumulation this step updates linear5.weight in its GEMM epilogue"
    model._ensure_garena()
    for pos in range(2):
        flat(model, model._garena, W5).fill_(float("nan"))
        model.train_step(*_data(256, 500 + pos), lr=LR, accumulate=2)
        torch.cuda.synchronize()
        g5 = flat(model, model._garena, W5)
        assert torch.isfinite(g5).all().item() and g5.abs().max().item() > 0, f"micro-step {pos}: the gradient slot was not written"
        assert model.epi_fused_dw == 0
    assert model._state.tolist()[0] == 1 and torch.isfinite(model._arena).all().item()


# ---- 8. refusals: raised before anything is launched ----------------------------------------------------------------------------------------------
def _arenas(model):
    return [None if x is None else x.clone() for x in (model._arena, model._garena, model._gacc, model._adam_m, model._adam_v, model._state)]


def _untouched(model, before):
    torch.cuda.synchronize()
    now = (model._arena, model._garena, model._gacc, model._adam_m, model._adam_v, model._state)
    return all((a is None and b is None) or (a is not None and b is not None and bits_equal(a, b)) for a, b in zip(before, now))


def test_fp16_refuses_accumulation():
    model = _model("fp16")
    before = _arenas(model)
    with pytest.raises(GoalnetError, match="fp16"):
        model.train_step(*_data(10), lr=LR, accumulate=2)
    assert _untouched(model, before) and model.accum_position == (0, 1)


def test_refusals_inside_a_window():
    model = _model()
    model.train_step(*_data(4, 600), lr=LR, accumulate=3)
    torch.cuda.synchronize()
    assert model.accum_position == (1, 3)
    before = _arenas(model)
    with pytest.raises(GoalnetError, match="may not change inside a window"):
        model.train_step(*_data(4, 601), lr=LR, accumulate=2)
    with pytest.raises(GoalnetError, match="may not change inside a window"):
        model.train_step(*_data(4, 601), lr=LR)
    model.fusion["0"].weight.requires_grad = False
    with pytest.raises(GoalnetError, match="frozen"):
        model.train_step(*_data(4, 601), lr=LR, accumulate=3)
    model.fusion["0"].weight.requires_grad = True
    with pytest.raises(GoalnetError, match="finish the window first"):
        model.training_state()
    with pytest.raises(GoalnetError, match="finish the window first"):
        model.load_training_state({"format": 1})
    with pytest.raises(ValueError):
        model.train_step(*_data(4, 601), lr=LR, accumulate=0)
    assert _untouched(model, before) and model.accum_position == (1, 3)
    for i in range(2):                                                # the window can still be finished
        model.train_step(*_data(4, 601 + i), lr=LR, accumulate=3)
    torch.cuda.synchronize()
    assert model.accum_position == (0, 3) and model._state.tolist()[0] == 1
    assert model.training_state()["adam_t"] == 1
