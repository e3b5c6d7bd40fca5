"""CPU: the dispatch rule of the fp32 GEMM epilogue fusion (cvml_goalnet_amd.avm.epi_fuse_dw_adam, epi_fuse_pieces) and the argument
contract of goalnet_linear_bwd_dw_adam, which returns before any launch (no GPU is needed and none is touched)."""
import pytest

import test_abi_contract_host as C
from cvml_goalnet_amd import _lib
from cvml_goalnet_amd.avm import EPI_FUSE_MIN_ROWS, EPI_FUSE_SKINNY_ROWS, epi_fuse_dw_adam, epi_fuse_pieces

# goalnet_linear_bwd_dw_adam joins the table of tests/test_abi_contract_host.py (the pattern of tests/test_rankcorr_host.py).
# arguments: 0 dy, 1 lddy, 2 x, 3 ldx, 4 scale, 5 shift, 6 bnC, 7 p, 8 m, 9 v, 10 db, 11 M, 12 K, 13 J, 14 lr, 15 beta1, 16 beta2,
# 17 eps, 18 step, 19 step_bias, 20 grad_scale, 21 stream
NAME = "goalnet_linear_bwd_dw_adam"
C.ROWS.setdefault(NAME, C.auto(
    NAME, {1: 36, 3: 1028, 4: None, 5: None, 6: 0, 10: None, 11: 40, 12: 1028, 13: 36, 14: 1e-3, 15: 0.9, 16: 0.999, 17: 1e-8, 19: 1, 20: 1.0},
    nullable=(4, 5, 10), shape=[(13, 34), (12, 1030), (11, 0), (11, 16)],
    align=[(0, 4), (2, 8), (1, 38), (3, 1030), (7, 8), (8, 4), (9, 8)], extra=[({4: 4096 * 5}, C.E_NULL), ({4: 4096 * 5, 5: 4096 * 6, 6: 6}, C.E_SHAPE)]))
ROW = C.ROWS[NAME]


def _mutations():
    for i in ROW["null"]:
        yield "null", i, None, C.E_NULL
    for i, v in ROW["shape"]:
        yield "shape", i, v, C.E_SHAPE
    for i, v in ROW["align"]:
        yield "align", i, v, C.E_ALIGN
    for changes, code in ROW["extra"]:
        yield "extra", tuple(changes), changes, code


@pytest.mark.parametrize("kind,index,value,code", list(_mutations()), ids=lambda v: str(v) if not isinstance(v, dict) else None)
def test_dw_adam_bad_argument_is_refused_before_any_launch(kind, index, value, code):
    args = list(ROW["args"])
    if kind == "extra":
        for i, v in value.items():
            args[i] = v
    else:
        args[index] = value
    C._refused(_lib.load(), NAME, args, code, f"{kind}: argument {index} = {value}")


def test_dw_adam_row_covers_every_pointer_and_the_abi_version_stays():
    types = _lib.PROTOTYPES[NAME][1]
    assert len(ROW["args"]) == len(types) == 22
    assert set(ROW["null"]) == {0, 2, 7, 8, 9, 18}, "dy, x, p, m, v and the step counter are required"
    assert {7, 8, 9} <= {i for i, _ in ROW["align"]}, "p, m and v are 16-byte aligned"
    assert (11, EPI_FUSE_SKINNY_ROWS) in ROW["shape"], "the weight-streaming rows are refused, not served by two launches"
    assert _lib.load().goalnet_abi_version() == _lib.ABI_VERSION == 7


def test_env_switch_parsing():
    assert epi_fuse_pieces(None) == epi_fuse_pieces("") == epi_fuse_pieces("1") == frozenset("a")
    assert epi_fuse_pieces("0") == frozenset()
    assert epi_fuse_pieces("a") == epi_fuse_pieces("A") == frozenset("a")
    assert epi_fuse_pieces("x") == frozenset(), "an unknown letter names no piece"


OK = dict(plain=True, synced=False, precision="fp32", train_w5=True, shadowed=False, inspected=False, forced=None, pieces=frozenset("a"))


def test_size_rule():
    assert EPI_FUSE_MIN_ROWS == 256 and EPI_FUSE_SKINNY_ROWS == 16
    for n, want in ((1, False), (16, False), (17, False), (255, False), (256, True), (1024, True)):
        assert epi_fuse_dw_adam(n, **OK) is want, n
    # model.epi_fuse = True: down to the first step the 128 x 128 tile serves, never the weight-streaming rows
    for n, want in ((10, False), (16, False), (17, True), (32, True), (1024, True)):
        assert epi_fuse_dw_adam(n, **{**OK, "forced": True}) is want, n
    assert not epi_fuse_dw_adam(1024, **{**OK, "forced": False})
    assert not epi_fuse_dw_adam(1024, **{**OK, "pieces": epi_fuse_pieces("0")})


def test_an_inspected_step_keeps_its_gradient():
    """model.keep_ctx = True (tests that read the arena's gradients after a step): the size rule yields, an explicit epi_fuse = True
    does not"""
    assert not epi_fuse_dw_adam(1024, **{**OK, "inspected": True})
    assert epi_fuse_dw_adam(1024, **{**OK, "inspected": True, "forced": True})


@pytest.mark.parametrize("change", [dict(plain=False), dict(synced=True), dict(train_w5=False), dict(shadowed=True), dict(precision="bf16"),
                                    dict(precision="fp16"), dict(precision="bf16x6"), dict(precision="fp16x3")],
                         ids=lambda c: "-".join(f"{k}={v}" for k, v in c.items()))
def test_everything_else_keeps_the_two_launches(change):
    """frozen or re-thawed tensors, DDP, a frozen linear5.weight, a live 16-bit copy of the weight, every other precision: at
    every size, forced or not"""
    for forced in (None, True):
        for n in (32, 256, 1024):
            assert not epi_fuse_dw_adam(n, **{**OK, **change, "forced": forced})
