"""CPU: the selectable losses of the regression head (include/goalnet_loss.h) — what holds without a GPU: the
second header against its ctypes table and the built library, the untouched first ABI, the argument refusals of the new entry points
(every one returns before any launch; pointers are small fake integers, as in tests/test_abi.py) and the Python-level errors."""
import ctypes
import os
import re

import pytest
import torch

from cvml_goalnet_amd import AVM, GoalnetError, _lib, ops
from cvml_goalnet_amd.loop import VideoTrainer

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
E_NULL, E_SHAPE, E_ALIGN, E_WORKSPACE, E_VALUE = -1, -2, -3, -4, -5
A, A2, A3, A4, A5, A6 = 4096, 8192, 12288, 16384, 20480, 24576        # fake, 16-byte aligned "device addresses": never dereferenced
MSE_BCAST, MSE, L1, SMOOTH_L1, RANK = 0, 1, 2, 3, 4


def _header():
    return open(os.path.join(ROOT, "include", "goalnet_loss.h")).read()


def _declared():
    text = re.sub(r"/\*.*?\*/", "", _header(), flags=re.S)
    return sorted(set(re.findall(r"\b(goalnet_[a-z0-9_]+)\s*\(", text)))


def test_loss_header_and_binding_agree():
    assert _declared() == sorted(_lib.LOSS_PROTOTYPES)
    if not os.path.exists(_lib.LIB_PATH):
        import __graft_entry__ as g
        g.build()
    lib = ctypes.CDLL(_lib.LIB_PATH)
    for name in _declared():
        assert hasattr(lib, name), f"{name} missing from libgoalnet_hip.so"
    loaded = _lib.load()
    for name, (res, args) in _lib.LOSS_PROTOTYPES.items():
        fn = getattr(loaded, name)
        assert fn.restype is res and list(fn.argtypes) == args, f"{name} was not bound by _lib.load()"


def test_loss_kind_codes_match_the_header():
    codes = {m.group(1).lower(): int(m.group(2)) for m in re.finditer(r"#define GOALNET_LOSS_([A-Z0-9_]+) (\d+)", _header())}
    assert codes == _lib.LOSS_KINDS
    assert int(re.search(r"#define GOALNET_FRAME_LOSS_MAX_N (\d+)", _header()).group(1)) == _lib.FRAME_LOSS_MAX_N == 65536
    assert int(re.search(r"#define GOALNET_E_VALUE \((-\d+)\)", _header()).group(1)) == E_VALUE


def test_first_abi_is_untouched():
    assert set(_lib.PROTOTYPES).isdisjoint(_lib.LOSS_PROTOTYPES)
    assert _lib.ABI_VERSION == 7 and _lib.load().goalnet_abi_version() == 7
    first = open(os.path.join(ROOT, "include", "goalnet_hip.h")).read()
    assert "#define GOALNET_ABI_VERSION 7" in first
    for name in _lib.LOSS_PROTOTYPES:
        assert name + "(" not in first, f"{name} belongs to include/goalnet_loss.h"


def _refused(name, args, code, what):
    lib = _lib.load()
    rc = getattr(lib, name)(*args)
    msg = lib.goalnet_last_error()
    assert rc == code, f"{name}, {what}: rc = {rc}, expected {code} ({msg!r})"
    assert rc < 0 and msg, f"{name}, {what}: no error message"


# goalnet_frame_loss(kind, param, pred, labels, weights, n, loss, dpred, ws, ws_bytes, stream)
def _fl(kind=MSE, param=1.0, pred=A, labels=A2, weights=None, n=10, loss=A3, dpred=A4, ws=A5, ws_bytes=1 << 20):
    return [kind, param, pred, labels, weights, n, loss, dpred, ws, ws_bytes, None]


FRAME_LOSS_REFUSALS = [
    ("pred = NULL", _fl(pred=None), E_NULL),
    ("labels = NULL", _fl(labels=None), E_NULL),
    ("loss = dpred = NULL", _fl(loss=None, dpred=None), E_NULL),
    ("loss = dpred = NULL (rank)", _fl(kind=RANK, loss=None, dpred=None), E_NULL),
    ("n = 0", _fl(n=0), E_SHAPE),
    ("n = 65537", _fl(n=65537), E_SHAPE),
    ("n = 65537 (rank)", _fl(kind=RANK, n=65537), E_SHAPE),
    ("kind = 5", _fl(kind=5), E_VALUE),
    ("kind = -1", _fl(kind=-1), E_VALUE),
    ("beta = 0", _fl(kind=SMOOTH_L1, param=0.0), E_VALUE),
    ("beta < 0", _fl(kind=SMOOTH_L1, param=-1.0), E_VALUE),
    ("beta = NaN", _fl(kind=SMOOTH_L1, param=float("nan")), E_VALUE),
    ("weights with rank", _fl(kind=RANK, weights=A6), E_VALUE),
    ("weights with mse_bcast", _fl(kind=MSE_BCAST, weights=A6), E_VALUE),
    ("rank without a workspace", _fl(kind=RANK, ws=None), E_NULL),
    ("rank workspace one byte short", _fl(kind=RANK, n=10, ws_bytes=239), E_WORKSPACE),
    ("rank workspace one byte short at 65536", _fl(kind=RANK, n=65536, ws_bytes=24 * 65536 - 1), E_WORKSPACE),
    ("misaligned workspace", _fl(kind=RANK, ws=A5 + 8), E_ALIGN),
]


@pytest.mark.parametrize("what,args,code", FRAME_LOSS_REFUSALS, ids=[r[0] for r in FRAME_LOSS_REFUSALS])
def test_frame_loss_refuses_before_any_launch(what, args, code):
    _refused("goalnet_frame_loss", args, code, what)


def test_frame_loss_ws_bytes_matches_its_header_comment():
    """the header: 24 n bytes for the rank loss with 1 <= n <= 65536, 0 for every other kind and for refused arguments"""
    assert "24 n bytes" in _header()
    lib = _lib.load()
    for n in (1, 2, 10, 16, 17, 1000, 65536):
        assert lib.goalnet_frame_loss_ws_bytes(RANK, n) == 24 * n
        for kind in (MSE_BCAST, MSE, L1, SMOOTH_L1, 5, -1):
            assert lib.goalnet_frame_loss_ws_bytes(kind, n) == 0
    for n in (0, -3, 65537):
        assert lib.goalnet_frame_loss_ws_bytes(RANK, n) == 0


# goalnet_mlp_fwd_loss: goalnet_mlp_fwd's arguments with (loss_kind, loss_param, weights) in front of n
W5 = (ctypes.c_void_p * 5)(A, A2, A3, A4, A5)
H4 = (ctypes.c_void_p * 4)(A, A2, A3, A4)
LD4 = (ctypes.c_int64 * 4)(512, 512, 256, 128)
adr = ctypes.addressof


def _mlp(kind=MSE, param=1.0, weights=None, n=9, labels=A3, loss=A4, dout=A5, cat=A):
    return [cat, 640, 640, adr(W5), adr(W5), adr(H4), adr(LD4), adr(H4), adr(H4), A, A2, labels, loss, dout, kind, param, weights, n, A6, None]


MLP_REFUSALS = [
    ("kind = 7", _mlp(kind=7), E_VALUE),
    ("beta = 0", _mlp(kind=SMOOTH_L1, param=0.0), E_VALUE),
    ("weights with rank", _mlp(kind=RANK, weights=A6), E_VALUE),
    ("weights with mse_bcast", _mlp(kind=MSE_BCAST, weights=A6), E_VALUE),
    ("n = 17", _mlp(n=17), E_SHAPE),
    ("n = 0", _mlp(n=0), E_SHAPE),
    ("cat = NULL", _mlp(cat=None), E_NULL),
    ("labels without a destination", _mlp(loss=None, dout=None), E_NULL),
]


@pytest.mark.parametrize("what,args,code", MLP_REFUSALS, ids=[r[0] for r in MLP_REFUSALS])
def test_mlp_fwd_loss_refuses_before_any_launch(what, args, code):
    _refused("goalnet_mlp_fwd_loss", args, code, what)


# ---- Python-level errors: raised before any launch, on a machine without a GPU ---------------------------------------------------
def _cpu_model(**kw):
    return AVM(audio_included=True, **kw)


def _inputs(n=4):
    return torch.zeros(n, 30, 30), torch.zeros(n, 3, 40, 40), torch.ones(n)


def test_loss_spec():
    assert ops.loss_spec() == (0, 0.0)
    assert ops.loss_spec("mse", None, True) == (1, 0.0) and ops.loss_spec("l1") == (2, 0.0)
    assert ops.loss_spec("smooth_l1") == (3, 1.0) and ops.loss_spec("smooth_l1", 0.25, True) == (3, 0.25)
    assert ops.loss_spec("rank") == (4, 0.0)
    assert ops.loss_spec("mse_bcast", head="classifier") == (0, 0.0)
    for bad in (("huber",), ("smooth_l1", 0.0), ("smooth_l1", -2.0), ("smooth_l1", float("nan")), ("rank", None, True),
                ("mse_bcast", None, True)):
        with pytest.raises(ValueError):
            ops.loss_spec(*bad)
    with pytest.raises(ValueError):
        ops.loss_spec("mse", head="classifier")


@pytest.mark.parametrize("kw", [dict(loss="huber"), dict(loss="smooth_l1", loss_param=0.0), dict(loss="smooth_l1", loss_param=-1.0),
                                dict(loss="rank", weights=torch.ones(4)), dict(loss="mse_bcast", weights=torch.ones(4)),
                                dict(weights=torch.ones(4))], ids=str)
def test_train_step_value_errors(kw):
    with pytest.raises(ValueError):
        _cpu_model().train_step(*_inputs(), **kw)


def test_train_step_refuses_other_losses_on_the_classifier_head():
    m = _cpu_model(head="classifier", num_classes=5)
    for name in ("mse", "l1", "smooth_l1", "rank"):
        with pytest.raises(ValueError):
            m.train_step(*_inputs(), loss=name)
        with pytest.raises(ValueError):
            VideoTrainer(m, loss=name)


@pytest.mark.parametrize("weights", [torch.ones(5), torch.ones(4, dtype=torch.float64), torch.ones(4, 2), [1.0, 1.0, 1.0, 1.0]], ids=str)
def test_train_step_weight_shape_and_dtype(weights):
    with pytest.raises(RuntimeError) as e:
        _cpu_model().train_step(*_inputs(), loss="mse", weights=weights)
    assert not isinstance(e.value, GoalnetError) and "weights" in str(e.value)


def test_global_batch_keeps_its_one_loss(tmp_path):
    import torch.distributed as dist
    from cvml_goalnet_amd import ddp
    dist.init_process_group("gloo", init_method=f"file://{tmp_path}/pg", rank=0, world_size=1)
    try:
        m = ddp.enable_global_batch(_cpu_model())
        for name in ("mse", "l1", "smooth_l1", "rank"):
            with pytest.raises(GoalnetError, match="global-batch"):
                m.train_step(*_inputs(), loss=name)
    finally:
        dist.destroy_process_group()


def test_video_trainer_errors():
    m = _cpu_model()
    for kw in (dict(loss="huber"), dict(loss="smooth_l1", loss_param=0.0)):
        with pytest.raises(ValueError):
            VideoTrainer(m, **kw)
    aud, vis, lab = _inputs()
    for name in ("mse_bcast", "rank"):
        tr = VideoTrainer(m, loss=name)
        with pytest.raises(ValueError):
            tr.train_video(aud, vis, lab, weights=torch.ones(4))
        with pytest.raises(ValueError):
            tr.eval_video(aud, vis, lab, weights=torch.ones(4))
    tr = VideoTrainer(m, loss="smooth_l1", loss_param=0.5)
    for bad in (torch.ones(3), torch.ones(4, dtype=torch.float64)):
        with pytest.raises(RuntimeError, match="weights"):
            tr.train_video(aud, vis, lab, weights=bad)
        with pytest.raises(RuntimeError, match="weights"):
            tr.eval_video(aud, vis, lab, weights=bad)


def test_frame_loss_python_errors():
    p, y = torch.zeros(4), torch.zeros(4)
    with pytest.raises(ValueError):
        ops.frame_loss(p, y, torch.zeros(1), None, "huber")
    with pytest.raises(ValueError):
        ops.frame_loss(p, y, torch.zeros(1), None, "smooth_l1", 0.0)
    with pytest.raises(ValueError):
        ops.frame_loss(p, y, torch.zeros(1), None, "rank", None, torch.ones(4))
    with pytest.raises(RuntimeError, match="weights"):
        ops.frame_loss(p, y, torch.zeros(1), None, "mse", None, torch.ones(5))
    with pytest.raises(RuntimeError, match="neither"):
        ops.frame_loss(p, y, None, None, "mse")
