"""CPU: the argument contract of include/goalnet_hip.h — every check below returns before any launch, so no GPU is needed (and
none is touched where one is present). Pointers are small fake integers, as in tests/test_abi.py.

ROWS holds, per entry point, one valid argument list and the mutations that must be refused: each required pointer set to NULL
(GOALNET_E_NULL), one out-of-set dim (GOALNET_E_SHAPE), a misaligned pointer or leading dimension where the header names an
alignment (GOALNET_E_ALIGN) and, for workspace-taking entry points, ws_bytes - 1 at a shape whose *_ws_bytes is above zero
(GOALNET_E_WORKSPACE). In every case the code is negative and goalnet_last_error() is non-empty.

test_every_entry_point_is_accounted_for fails when include/goalnet_hip.h (through _lib.PROTOTYPES) gains an entry point that is
in none of ROWS, NO_ERROR_PATH (functions that cannot fail: sizes, predicates, names) and PENDING. PENDING is the list of entry
points whose rows are still to be written; it may only shrink."""
import ctypes

import pytest

import _abi_shapes as B
from cvml_goalnet_amd import _lib

E_NULL, E_SHAPE, E_ALIGN, E_WORKSPACE = -1, -2, -3, -4
A, A2, A3, A4 = 4096, 8192, 12288, 16384        # fake, 16-byte aligned "device addresses": never dereferenced
ADAM = [A, A2, A3, A4, 1024, 1e-3, 0.9, 0.999, 1e-8]


def row(args, null=(), shape=(), align=(), ws=None):
    """args: a valid call; null: indices of required pointers; shape / align: (index, bad value) pairs, one mutation each;
    ws: (ws_bytes function, its dims, index of the ws_bytes argument)"""
    return dict(args=list(args), null=tuple(null), shape=tuple(shape), align=tuple(align), ws=ws)


CONV = (10, 11, 11, 256, 512)                     # split-K: goalnet_conv3x3_fwd_ws_bytes > 0
LIN = (7, 41472, 512)
ROWS = {
    "goalnet_conv3x3_fwd": row([A, None, None, A2, None, 1, A3, *CONV, A4, 1 << 30, None, 0, None], null=(0, 3, 6), shape=[(10, 65), (11, 30), (7, 0)],
                               align=[(0, A + 4), (6, A3 + 8)], ws=("goalnet_conv3x3_fwd_ws_bytes", CONV, 13)),
    "goalnet_conv3x3_wgrad": row([A, None, None, A2, A3, A4, 1 << 30, None, None, 0, *CONV, None], null=(0, 3, 4, 5), shape=[(13, 66), (10, 0)],
                                 align=[(4, A3 + 4)], ws=("goalnet_conv3x3_wgrad_ws_bytes", CONV, 6)),
    "goalnet_conv3x3_wgrad_codes": row([A, 2, 5, 5, None], null=(0,)),
    "goalnet_linear_fwd": row([A, LIN[1], None, None, 0, A2, None, 0, None, 0, A3, 512, None, 0, *LIN, A4, 1 << 30, None], null=(0, 5, 10),
                              shape=[(15, 33), (16, 510)], align=[(1, LIN[1] + 2), (11, 514), (0, A + 4)], ws=("goalnet_linear_fwd_ws_bytes", LIN, 18)),
    "goalnet_linear_bwd_dx": row([A, 96, A2, None, 0, A3, 1000, 16, 1000, 96, None], null=(0, 2, 5), shape=[(9, 40), (8, 1002)], align=[(1, 98), (6, 1002)]),
    "goalnet_linear_bwd_dw": row([A, 36, A2, 1028, None, None, 0, A3, None, 16, 1028, 36, None], null=(0, 2, 7), shape=[(11, 34), (9, 0)],
                                 align=[(1, 38), (3, 1030)]),
    "goalnet_colsum": row([A, 36, 16, 36, A2, None], null=(0, 4), shape=[(2, 0)]),
    "goalnet_mul": row([A, 40, A2, 40, A3, 40, 7, 37, None], null=(0, 2, 4), shape=[(7, 0)]),
    "goalnet_relu_bwd": row([A, A2, A3, 100, None], null=(0, 1, 2), shape=[(3, 0)]),
    "goalnet_scale": row([A, 100, 0.5, None], null=(0,), shape=[(1, 0)]),
    "goalnet_partials_sum": row([A, 4, 64, 64, A2, None], null=(0, 4), shape=[(2, 63), (1, 0)]),
    "goalnet_partials_sum_f64": row([A, 4, 64, 64, A2, None], null=(0, 4), shape=[(2, 63)]),
    "goalnet_partials_sum2": row([A, 4, 64, A2, A3, 4, 64, A4, None], null=(0, 3, 4, 7), shape=[(5, 0)]),
    "goalnet_conv1d_fwd": row([A, A2, A3, 1, A4, 4, 30, 30, 64, 2, 1, None], null=(0, 1, 2, 4), shape=[(9, 0)]),
    "goalnet_conv1d_bwd": row([A, A2, A3, None, A4, A, 4, 30, 30, 64, 2, 1, None, 0, None], null=(0, 1, 2, 4, 5), shape=[(6, 0)]),
    "goalnet_conv1d_bwd_small": row([A, A2, None, A3, None, A4, A, 4, 30, 30, 64, 2, 1, None], null=(0, 1, 3, 5, 6), shape=[(7, 64), (8, 257)]),
    "goalnet_head_fwd": row([A, 128, A2, A3, None, A4, 4, 128, None], null=(0, 2, 3, 5), shape=[(6, 0)]),
    "goalnet_head_bwd": row([A, A2, A3, 128, A4, None, 0, A, 128, A2, A3, 4, 128, None], null=(0, 1, 2, 4, 7, 9, 10), shape=[(12, 1024)]),
    "goalnet_mse_bcast": row([A, A2, 4, None, None, None], null=(0, 1), shape=[(2, 0)]),
    "goalnet_adam_step": row([*ADAM, 1, 1.0, None], null=(0, 1, 2, 3), shape=[(9, 0), (4, 0)], align=[(0, A + 8), (1, A2 + 4), (2, A3 + 8), (3, A4 + 4)]),
    "goalnet_adam_step_dev": row([*ADAM, A, 1, 1.0, None], null=(0, 1, 2, 3, 9), shape=[(4, 0)], align=[(0, A + 8), (3, A4 + 4)]),
    "goalnet_adam_step_dev_blocks": row([*ADAM, A, 1, 1.0, 128, None], null=(0, 1, 2, 3, 9), shape=[(12, 0), (12, 65536), (4, 0)], align=[(1, A2 + 8)]),
    "goalnet_adam_step_dev_shadow": row([*ADAM, A, 1, 1.0, A2, 0, 1024, 0, None], null=(0, 1, 2, 3, 9, 12),
                                        shape=[(13, 2), (14, 1022), (14, 1028), (14, 0)], align=[(12, A2 + 2), (12, A2 + 4), (2, A3 + 8)]),
    "goalnet_adam_step_dev_guarded": row([*ADAM, A, 1, 1.0, A2, 0, 1024, 0, A3, None], null=(0, 1, 2, 3, 9, 16), shape=[(13, 2), (14, 1028)],
                                         align=[(12, A2 + 4), (0, A + 8)]),
    "goalnet_grad_finite_check": row([A, 100, A2, 1, A3, None, None], null=(0, 2, 4), shape=[(1, 0)]),
    "goalnet_counter_add": row([A, 1, None], null=(0,)),
    "goalnet_counters_add4": row([A, 1, 1, 1, 1, None], null=(0,)),
    "goalnet_counters_add4_guarded": row([A, 1, 1, 1, 1, A2, None], null=(0, 5)),
    "goalnet_rows_gather": row([A, A2, 16, 2, A3, None], null=(0, 1, 4), shape=[(2, 6), (3, 0)]),
    "goalnet_rows_scatter": row([A, A2, 16, 2, A3, None], null=(0, 1, 4), shape=[(2, 6), (3, 0)]),
}

def auto(name, vals=None, nullable=(), shape=(), align=(), ws=None, extra=()):
    """A row whose valid call is built from the prototype: pointer i is the fake 16-byte aligned address 4096 (i + 1), the stream
    NULL, an integer 1 and a float 0.5 unless `vals` gives the argument. Every pointer argument that is not listed in `nullable`
    (the ones the header calls nullable or optional) must be refused with GOALNET_E_NULL. align: (index, byte offset added to the
    pointer, or a new leading dimension). extra: ({index: value, ...}, code) mutations of more than one argument."""
    vals = dict(vals or {})
    types = _lib.PROTOTYPES[name][1]
    args, null = [], []
    for i, t in enumerate(types):
        if i in vals:
            args.append(vals[i])
        elif t is _lib.P:
            args.append(None if i == len(types) - 1 else 4096 * (i + 1))
        else:
            args.append(0.5 if t in (ctypes.c_float, ctypes.c_double) else 1)
        if t is _lib.P and i != len(types) - 1 and i not in nullable:
            null.append(i)
    r = row(args, null=null, shape=shape, align=[(i, args[i] + v if types[i] is _lib.P else v) for i, v in align], ws=ws)
    r["extra"] = tuple(extra)
    return r


BIG = 1 << 30                                     # a ws_bytes that is never the reason for a refusal
W5 = (ctypes.c_void_p * 5)(A, A2, A3, A4, A + A4)        # HOST arrays of fake device pointers (goalnet_mlp_fwd / _bwd read them)
H4 = (ctypes.c_void_p * 4)(A, A2, A3, A4)
W5_HOLE = (ctypes.c_void_p * 5)(A, A2, None, A4, A + A4)
LD4 = (ctypes.c_int64 * 4)(512, 512, 256, 128)
WIDTHS = (ctypes.c_int * 4)(512, 512, 256, 128)
WIDTHS_BAD = (ctypes.c_int * 4)(512, 0, 256, 128)
adr = ctypes.addressof
POOL = {0: 2, 1: 9, 2: 9, 3: 64}                 # N, Hc, Wc, C
SMALL = (3, 3, 5, 256)
WG = (16, 13, 13, 64, 256)
O16 = (64, 32, 32, 64, 256)                       # served by the 256 x 256 tile: N H W >= 65536, Cout >= 256
LSPLIT = (256, 65536, 256)                        # goalnet_linear_split_ok
LO16 = (512, 1 << 18, 256)                        # goalnet_linear_bwd_dx_bf16_o16_ok


def at(first, dims):
    return {first + i: d for i, d in enumerate(dims)}


ROWS.update({
    "goalnet_fill_uniform": auto("goalnet_fill_uniform", {1: 8}, shape=[(1, -1)]),
    "goalnet_dropout_mask": auto("goalnet_dropout_mask", {1: 8}, shape=[(1, -1), (4, 1.0), (4, -0.5)]),
    "goalnet_transpose_inner": auto("goalnet_transpose_inner", {2: 4, 3: 5, 4: 6}, shape=[(2, 0), (2, 65536), (4, 0)]),
    "goalnet_conv3x3_weight_flip": auto("goalnet_conv3x3_weight_flip", {2: 64, 3: 64}, shape=[(2, 0), (3, 0)]),
    "goalnet_conv3x3_weight_flip2": auto("goalnet_conv3x3_weight_flip2", {2: 64, 3: 64, 6: 64, 7: 64}, shape=[(2, 0), (7, 0)]),
    "goalnet_conv1_fwd": auto("goalnet_conv1_fwd", at(4, (3, 41, 38)), shape=[(4, 0), (6, 0)], align=[(3, 4)]),
    "goalnet_conv1_wgrad": auto("goalnet_conv1_wgrad", {5: BIG, **at(6, (3, 41, 38))}, nullable=(3,), shape=[(6, 0), (7, 0)],
                                ws=("goalnet_conv1_wgrad_ws_bytes", (3, 41, 38), 5)),
    "goalnet_pool_bnstats_fwd": auto("goalnet_pool_bnstats_fwd", {4: 2, **at(5, (2, 9, 9, 64))}, nullable=(2,),
                                     shape=[(8, 48), (6, 2), (7, 2), (4, 0), (4, 1025)], align=[(0, 4), (1, 8), (2, 2)]),
    "goalnet_pool_bnstats_fwd_p16": auto("goalnet_pool_bnstats_fwd_p16", {1: 0, 5: 2, **at(6, (2, 9, 9, 64)), 10: 0}, nullable=(3,),
                                         shape=[(9, 16), (7, 2), (5, 0)], align=[(0, 4), (2, 8)]),
    "goalnet_bn_finalize": auto("goalnet_bn_finalize", {1: 2, 8: 100, 9: 64}, shape=[(9, 0), (8, 0)]),
    "goalnet_pool_bn_eval_fwd": auto("goalnet_pool_bn_eval_fwd", {1: 0, 3: 0, 11: 2, **at(12, (2, 9, 9, 64)), 16: 0}, nullable=(4,),
                                     shape=[(15, 48), (13, 2), (1, 1), (11, 0)], align=[(0, 4), (2, 8), (10, 4)],
                                     extra=[({3: 1, 15: 16}, E_SHAPE), ({3: 1, 14: 171}, E_SHAPE)]),     # a 16-bit p needs C % 32 == 0, Wc <= 170
    "goalnet_bn_bwd_finalize_eval": auto("goalnet_bn_bwd_finalize_eval", {1: 2, 4: 64}, shape=[(4, 0)]),
    "goalnet_bn_bwd_reduce": auto("goalnet_bn_bwd_reduce", {5: 2, 6: 100, 7: 64}, shape=[(7, 48), (6, 0), (5, 0), (5, 1025)],
                                  align=[(0, 4), (1, 4), (2, 4), (3, 8)]),
    "goalnet_bn_bwd_reduce_t": auto("goalnet_bn_bwd_reduce_t", {1: 0, 3: 0, 7: 2, 8: 100, 9: 64, 10: 0}, shape=[(9, 48), (8, 0), (7, 0)],
                                    align=[(0, 4), (2, 8)]),
    "goalnet_bn_bwd_finalize": auto("goalnet_bn_bwd_finalize", {1: 2, 5: 100, 6: 64}, shape=[(6, 0), (5, 0)]),
    "goalnet_bnpool_bwd": auto("goalnet_bnpool_bwd", {6: 2, **at(7, (2, 9, 9, 64))}, shape=[(10, 48), (8, 2), (6, 0)], align=[(0, 4), (3, 4), (4, 4)]),
    "goalnet_bnpool_bwd_bf16p": auto("goalnet_bnpool_bwd_bf16p", {7: 2, **at(8, (2, 9, 9, 64)), 12: 0}, nullable=(4,), shape=[(11, 16), (9, 2)],
                                     align=[(5, 8), (0, 4)]),
    "goalnet_bnpool_bwd_bf16p_t": auto("goalnet_bnpool_bwd_bf16p_t", {1: 0, 3: 0, 9: 2, **at(10, (2, 9, 9, 64)), 14: 0}, nullable=(6, 7),
                                       shape=[(13, 16), (12, 2)], align=[(0, 4), (7, 8)], extra=[({6: None, 7: None}, E_NULL)]),
    "goalnet_pool_bn_fwd_small": auto("goalnet_pool_bn_fwd_small", {14: BIG, **at(16, SMALL)}, nullable=(2,), shape=[(19, 1024), (19, 48), (17, 2), (16, 1 << 20)],
                                      align=[(0, 4), (1, 8), (13, 4)], ws=("goalnet_bn_small_ws_bytes", SMALL[3:], 14)),
    "goalnet_bn_bwd_reduce_small": auto("goalnet_bn_bwd_reduce_small", {9: BIG, **at(11, SMALL)}, shape=[(14, 1024), (12, 2)], align=[(0, 4), (7, 4), (8, 4)],
                                        ws=("goalnet_bn_small_ws_bytes", SMALL[3:], 9)),
    "goalnet_bn_bwd_reduce_small_eval": auto("goalnet_bn_bwd_reduce_small_eval", {9: BIG, **at(11, SMALL)}, shape=[(14, 1024), (12, 2)],
                                             align=[(0, 4), (7, 4), (8, 4)], ws=("goalnet_bn_small_ws_bytes", SMALL[3:], 9)),
    "goalnet_bnpool_bwd_small": auto("goalnet_bnpool_bwd_small", {7: BIG, **at(9, SMALL)}, shape=[(12, 1024), (10, 2)], align=[(0, 4), (4, 4)],
                                     ws=("goalnet_bn_small_ws_bytes", SMALL[3:], 7)),
    "goalnet_cast_bf16": auto("goalnet_cast_bf16", {2: 8, 3: 0}, shape=[(2, 12), (2, 0)], align=[(0, 4), (1, 8)]),
    "goalnet_cast_f32": auto("goalnet_cast_f32", {2: 8, 3: 0}, shape=[(2, 12), (2, 0)], align=[(0, 8), (1, 4)]),
    "goalnet_bn_apply_bf16": auto("goalnet_bn_apply_bf16", {4: 128, 5: 64, 6: 0}, shape=[(5, 12), (4, 100)], align=[(0, 4), (1, 4), (2, 4), (3, 8)]),
    "goalnet_bn_apply_bf16_p16": auto("goalnet_bn_apply_bf16_p16", {4: 128, 5: 64, 6: 0}, shape=[(5, 12), (4, 100)], align=[(0, 8), (3, 8)]),
    "goalnet_conv3x3_fwd_bf16": auto("goalnet_conv3x3_fwd_bf16", {3: 1, **at(5, (2, 9, 9, 64, 64)), 10: 0}, nullable=(2,), shape=[(8, 32), (9, 30), (5, 0)],
                                     align=[(0, 8), (1, 8), (4, 4)]),
    "goalnet_linear_fwd_bf16": auto("goalnet_linear_fwd_bf16", {1: LIN[1], 4: 1, 6: 512, 8: 512, 10: 512, **at(11, LIN), 15: BIG, 16: 0}, nullable=(3, 5, 9, 14),
                                    shape=[(12, LIN[1] + 8), (13, 510), (11, 0)], align=[(0, 8), (7, 4), (1, LIN[1] + 4), (8, 514)],
                                    ws=("goalnet_linear_fwd_bf16_ws_bytes", LIN, 15), extra=[({14: None}, E_WORKSPACE), ({14: 4096 * 15 + 8}, E_WORKSPACE)]),
    "goalnet_to_bf16_padded": auto("goalnet_to_bf16_padded", {**at(4, (2, 9, 9, 64)), 8: 0}, shape=[(7, 12), (4, 0)], align=[(0, 4), (1, 4), (3, 8)]),
    "goalnet_to_bf16_padded_p16": auto("goalnet_to_bf16_padded_p16", {**at(4, (2, 9, 9, 64)), 8: 0}, shape=[(7, 12), (4, 0)], align=[(0, 8), (2, 4), (3, 8)]),
    "goalnet_conv3x3_fwd_bf16p": auto("goalnet_conv3x3_fwd_bf16p", {3: 1, **at(5, CONV), 11: BIG, 12: 0}, nullable=(2, 10), shape=[(8, 32), (9, 30), (6, 0)],
                                      align=[(0, 8), (4, 4)], ws=("goalnet_conv3x3_fwd_bf16p_ws_bytes", CONV, 11), extra=[({10: 4096 * 11 + 8}, E_WORKSPACE)]),
    "goalnet_conv3x3_fwd_bf16p_o16": auto("goalnet_conv3x3_fwd_bf16p_o16", {3: 1, **at(5, O16), 10: 0}, nullable=(2,), shape=[(5, 1), (8, 32), (9, 260)],
                                          align=[(4, 8), (2, 4)]),
    "goalnet_conv3x3_wgrad_bf16": auto("goalnet_conv3x3_wgrad_bf16", {4: BIG, **at(5, WG), 10: 0}, shape=[(8, 36), (9, 100), (5, 0)], align=[(2, 4), (3, 8)],
                                       ws=("goalnet_conv3x3_wgrad_bf16_ws_bytes", WG, 4)),
    "goalnet_absmax": auto("goalnet_absmax", {1: 64, 4: 64, 5: 4, 6: 64}, shape=[(6, 12), (5, 0), (4, 48)], align=[(0, 4)]),
    "goalnet_split_scales": auto("goalnet_split_scales"),
    "goalnet_split_padded": auto("goalnet_split_padded", {0: 3, **at(6, (2, 9, 11, 64))}, nullable=(4,), shape=[(0, 4), (0, 1), (9, 12)], align=[(1, 4), (5, 8)],
                                 extra=[({0: 2, 4: None}, E_NULL)]),
    "goalnet_split_rows": auto("goalnet_split_rows", {0: 3, 2: 64, 5: 64, 8: 4, 9: 64}, nullable=(6,), shape=[(0, 1), (9, 12), (8, 0)], align=[(1, 4), (7, 8)],
                               extra=[({0: 2, 6: None}, E_NULL)]),
    "goalnet_conv3x3_fwd_split": auto("goalnet_conv3x3_fwd_split", {0: 3, 4: 1, **at(6, (2, 9, 11, 64, 256))}, nullable=(3, 11), shape=[(0, 5), (9, 32), (10, 30)],
                                      align=[(1, 8), (5, 4)], extra=[({0: 2, 11: None}, E_NULL)]),
    "goalnet_conv3x3_wgrad_split": auto("goalnet_conv3x3_wgrad_split", {0: 3, 5: BIG, **at(6, (2, 9, 11, 64, 256))}, nullable=(11,), shape=[(0, 1), (9, 36)],
                                        align=[(3, 4), (4, 8)], ws=("goalnet_conv3x3_wgrad_split_ws_bytes", (3, 2, 9, 11, 64, 256), 5),
                                        extra=[({0: 2, 11: None}, E_NULL)]),
    "goalnet_linear_fwd_split": auto("goalnet_linear_fwd_split", {0: 3, 4: 1, 6: 256, 8: 256, 10: 256, **at(11, LSPLIT), 15: BIG}, nullable=(3, 5, 9, 16),
                                     shape=[(11, 16), (0, 4), (12, 65536 + 8)], align=[(1, 8), (7, 4), (14, 8), (8, 258)],
                                     ws=("goalnet_linear_fwd_split_ws_bytes", (3,) + LSPLIT, 15), extra=[({0: 2, 16: None}, E_NULL)]),
    "goalnet_linear_bwd_dx_split": auto("goalnet_linear_bwd_dx_split", {0: 3, 4: LSPLIT[1], **at(5, LSPLIT)}, nullable=(8,), shape=[(5, 16), (0, 1)],
                                        align=[(3, 4), (4, LSPLIT[1] + 2)], extra=[({0: 2, 8: None}, E_NULL)]),
    "goalnet_linear_bwd_dw_split": auto("goalnet_linear_bwd_dw_split", {0: 3, **at(4, LSPLIT)}, nullable=(7,), shape=[(4, 16), (0, 1)], align=[(3, 4), (1, 8)],
                                        extra=[({0: 2, 7: None}, E_NULL)]),
    "goalnet_linear_bwd_dx_bf16": auto("goalnet_linear_bwd_dx_bf16", {1: 64, 4: 1000, 6: 1000, 7: 16, 8: 1000, 9: 64, 10: 0}, nullable=(3,),
                                       shape=[(9, 40), (8, 1004), (7, 0)], align=[(0, 8), (5, 4), (1, 68), (6, 1002)]),
    "goalnet_linear_bwd_dx_bf16_o16": auto("goalnet_linear_bwd_dx_bf16_o16", {1: 256, 4: LO16[1], **at(5, LO16), 8: 0}, shape=[(5, 16), (7, 40), (6, LO16[1] + 4)],
                                           align=[(3, 8), (1, 260), (4, LO16[1] + 4)]),
    "goalnet_linear_bwd_dw_bf16": auto("goalnet_linear_bwd_dw_bf16", {1: 64, 3: 1000, 5: 16, 6: 1000, 7: 64, 8: 0}, shape=[(7, 36), (6, 1004), (5, 0)],
                                       align=[(4, 4), (1, 68), (3, 1004)]),
    "goalnet_mlp_fwd": auto("goalnet_mlp_fwd", {1: 640, 2: 640, 3: adr(W5), 4: adr(W5), 5: adr(H4), 6: adr(LD4), 7: adr(H4), 8: adr(H4), 14: 9},
                            nullable=(11, 12, 13), shape=[(14, 0), (14, 17), (2, 644), (2, 6), (2, 0)], align=[(0, 4), (1, 642)],
                            extra=[({12: None, 13: None}, E_NULL), ({3: adr(W5_HOLE)}, E_NULL), ({4: adr(W5_HOLE)}, E_NULL)]),
    "goalnet_mlp_bwd": auto("goalnet_mlp_bwd", {2: adr(W5), 3: 640, 4: adr(W5), 5: 640, 6: adr(W5), 7: adr(W5), 8: adr(W5), 10: 640, 12: 128, 13: 9, 14: 640, 16: BIG},
                            nullable=(11,), shape=[(13, 0), (13, 17), (14, 644), (14, 6), (12, 126), (12, 640)], align=[(9, 4), (15, 8), (3, 642), (10, 642)],
                            ws=("goalnet_mlp_bwd_ws_bytes", (9,), 16), extra=[({2: adr(W5_HOLE)}, E_NULL), ({7: adr(W5_HOLE)}, E_NULL)]),
    "goalnet_cubic_resample": auto("goalnet_cubic_resample", {3: 2, 4: 8, 5: 4}, shape=[(4, 3), (3, 0), (5, 0)]),
    "goalnet_logmel_slots": auto("goalnet_logmel_slots", {3: 2, 4: 4}, shape=[(3, 0), (3, 65536), (4, 0)]),
    "goalnet_mfcc_from_logmel": auto("goalnet_mfcc_from_logmel", {2: 2, 3: 8, 8: 30, 9: 16, 10: 80.0}, shape=[(3, 3), (8, 129), (8, 0), (2, 0), (9, 0)]),
    "goalnet_cls_head_fwd": auto("goalnet_cls_head_fwd", {1: 128, 6: 4, 7: 128, 8: 5}, nullable=(4,), shape=[(8, 9), (8, 1), (7, 1024), (6, 0)]),
    "goalnet_cross_entropy": auto("goalnet_cross_entropy", {4: 4, 5: 5}, nullable=(2, 3), shape=[(5, 9), (5, 1), (4, 0)], extra=[({2: None, 3: None}, E_NULL)]),
    "goalnet_cls_head_bwd": auto("goalnet_cls_head_bwd", {3: 128, 6: 128, 8: 128, 11: 4, 12: 128, 13: 5}, nullable=(5,), shape=[(13, 9), (12, 1024), (11, 0)]),
    "goalnet_argmax_plus1": auto("goalnet_argmax_plus1", {2: 4, 3: 5}, shape=[(3, 0), (2, 0)]),
    "goalnet_dropout_masks_dev": auto("goalnet_dropout_masks_dev", {1: 4, 2: WIDTHS, 3: 4, 9: 0}, shape=[(3, 0), (3, 9), (8, 1.0), (9, -1), (1, 0)],
                                      extra=[({2: None}, E_NULL), ({2: WIDTHS_BAD}, E_SHAPE)]),
    "goalnet_frames_preprocess": auto("goalnet_frames_preprocess", {1: 2, 2: 8, 3: 8, 5: 4, 6: 4}, shape=[(1, 0), (3, 0), (5, 0)]),
    "goalnet_frames_preprocess_strided": auto("goalnet_frames_preprocess_strided", {1: 5, 2: 2, 3: 8, 4: 8, 6: 4, 7: 4}, shape=[(1, 0), (2, 0), (6, 0), (4, 0)]),
    "goalnet_gather_clips": auto("goalnet_gather_clips", {1: 100, 2: 64, 5: 4, 7: 15, 12: BIG}, shape=[(1, 0), (2, 0), (5, 0), (7, -1)],
                                 ws=("goalnet_gather_clips_ws_bytes", (4,), 12)),
    "goalnet_knapsack": auto("goalnet_knapsack", {2: 4, 3: 100, 6: BIG}, shape=[(2, 0), (3, -1)], ws=("goalnet_knapsack_ws_bytes", (4, 100), 6)),
    "goalnet_fscore": auto("goalnet_fscore", {2: 3, 3: 100}, shape=[(2, 0), (3, 0)]),
    "goalnet_postprocess": auto("goalnet_postprocess", {1: 20, 2: 5, 3: 100, 5: 4, 6: 5, 7: 75, 9: 3, 17: BIG}, shape=[(1, 0), (5, 0), (2, 0), (9, 0)],
                                ws=("goalnet_postprocess_ws_bytes", (4, 75, 3), 17)),
    "goalnet_postprocess_batch": auto("goalnet_postprocess_batch", {1: 3, 2: 20, 3: 5, 4: 100, 6: 4, 7: 5, 8: 75, 10: 3, 18: BIG},
                                      shape=[(1, 0), (1, 65536), (6, 0)], ws=("goalnet_postprocess_batch_ws_bytes", (4, 75, 3, 3), 18)),
    "goalnet_mean_annotations": auto("goalnet_mean_annotations", {1: 20, 2: 100, 3: 5}, shape=[(1, 0), (1, 129), (3, 0), (2, 0)]),
})

# the workspace of the fp32 conv1d backward is optional (frame slices from 512 frames on), a lent one must be whole and 8-byte aligned
ROWS["goalnet_conv1d_bwd"] = row([A, A2, A3, None, A4, A, 515, 30, 30, 64, 2, 1, A2, BIG, None], null=(0, 1, 2, 4, 5), shape=[(6, 0), (11, -1)],
                                 align=[(12, A2 + 4)], ws=("goalnet_conv1d_bwd_ws_bytes", (515, 30, 64), 13))

# no error path: sizes, names, predicates and constants; each is checked against its header comment further down
NO_ERROR_PATH = {n for n, (res, _) in _lib.PROTOTYPES.items() if res is not ctypes.c_int} | {
    "goalnet_abi_version", "goalnet_stat_parts", "goalnet_mlp_blocks", "goalnet_linear_split_ok", "goalnet_linear_bwd_dx_bf16_o16_ok",
    "goalnet_conv3x3_fwd_bf16p_o16_ok", "goalnet_conv1d_bwd_small_ok"}
# argument lists that the table cannot express: segment structs (test_row_copy_segments_are_checked) and host out-pointers
# (test_bf16_padded_layout_refuses_bad_arguments)
STRUCT_ROWS = {"goalnet_rows_copy_batch", "goalnet_rows_scatter_tick", "goalnet_bf16_padded_layout"}
PENDING = set()          # nothing may be parked here: test_every_entry_point_is_accounted_for asserts it stays empty


def test_every_entry_point_is_accounted_for():
    names = set(_lib.PROTOTYPES)
    assert not PENDING, "every entry point has its row: nothing is parked"
    groups = [set(ROWS), NO_ERROR_PATH, STRUCT_ROWS]
    covered = set().union(*groups)
    assert names - covered == set(), f"entry points of include/goalnet_hip.h without a row here: {sorted(names - covered)}"
    assert covered - names == set(), f"rows for entry points the header no longer declares: {sorted(covered - names)}"
    assert sum(len(g) for g in groups) == len(covered), "an entry point is listed twice (a row was written: take it out of PENDING)"
    for name, r in ROWS.items():
        assert len(r["args"]) == len(_lib.PROTOTYPES[name][1]), f"{name}: the row has {len(r['args'])} arguments"


def _refused(lib, name, args, code, what):
    rc = getattr(lib, name)(*args)
    msg = lib.goalnet_last_error()
    assert rc == code, f"{name}, {what}: rc = {rc}, expected {code} ({msg!r})"
    assert rc < 0 and msg, f"{name}, {what}: no error message"


def _mutations():
    for name, r in ROWS.items():
        for i in r["null"]:
            yield name, "null", i, None, E_NULL
        for i, v in r["shape"]:
            yield name, "shape", i, v, E_SHAPE
        for i, v in r["align"]:
            yield name, "align", i, v, E_ALIGN
        for k, (changes, code) in enumerate(r.get("extra", ())):
            yield name, "extra", k, None, code


@pytest.mark.parametrize("name,kind,index,value,code", list(_mutations()), ids=lambda v: str(v) if not isinstance(v, float) else None)
def test_bad_argument_is_refused_before_any_launch(name, kind, index, value, code):
    lib = _lib.load()
    args = list(ROWS[name]["args"])
    if kind == "extra":
        value = ROWS[name]["extra"][index][0]
        for i, v in value.items():
            args[i] = v
    else:
        args[index] = value
    _refused(lib, name, args, code, f"{kind}: argument {index} = {value}")


@pytest.mark.parametrize("name", [n for n, r in ROWS.items() if r["ws"]])
def test_short_workspace_is_refused_before_any_launch(name):
    lib = _lib.load()
    fn, dims, index = ROWS[name]["ws"]
    need = getattr(lib, fn)(*dims)
    assert need > 0, f"{fn}{dims} = 0: the row needs a shape with a workspace"
    args = list(ROWS[name]["args"])
    args[index] = need - 1
    _refused(lib, name, args, E_WORKSPACE, f"ws_bytes = {need} - 1")


def test_row_copy_segments_are_checked():
    lib = _lib.load()
    seg = lambda **kw: (_lib.RowCopy * 1)(_lib.RowCopy(**{**dict(src=A, dst=A2, row_bytes=16, nrows=2, gather=0, cursor=A3, cursor_bias=0), **kw}))
    for name, tail in (("goalnet_rows_copy_batch", (None,)), ("goalnet_rows_scatter_tick", (A4, 1, 1, 1, 1, None, None))):
        _refused(lib, name, (None, 1) + tail, E_NULL, "segs = NULL")
        _refused(lib, name, (seg(), 0) + tail, E_SHAPE, "count = 0")
        _refused(lib, name, (seg(), 5) + tail, E_SHAPE, "count = 5")
        for field in ("src", "dst", "cursor"):
            _refused(lib, name, (seg(**{field: None}), 1) + tail, E_NULL, f"segment {field} = NULL")
        _refused(lib, name, (seg(row_bytes=6), 1) + tail, E_SHAPE, "row_bytes = 6")
        _refused(lib, name, (seg(nrows=0), 1) + tail, E_SHAPE, "nrows = 0")
    _refused(lib, "goalnet_rows_scatter_tick", (seg(), 1, None, 1, 1, 1, 1, None, None), E_NULL, "counters = NULL")
    _refused(lib, "goalnet_rows_scatter_tick", (seg(row_bytes=1 << 20, nrows=8), 1, A4, 1, 1, 1, 1, None, None), E_SHAPE, "more than 4 MB")


# ---- the condition that keeps tests/test_gpu_abi_contract.py honest -------------------------------------------------------
@pytest.mark.parametrize("name", sorted(B.WS_ROWS))
def test_guarded_rows_include_a_real_workspace(name):
    """'the workspace is exactly *_ws_bytes long' means nothing at a shape that needs none: every workspace-taking row of the GPU
    table has a shape with ws_bytes > 0, and where the header makes the workspace optional, one with 0 as well"""
    lib = _lib.load()
    fn, shapes, optional = B.WS_ROWS[name]
    sizes = [getattr(lib, fn)(*dims) for dims in shapes]
    assert any(s > 0 for s in sizes), f"{fn}: no row of the GPU table needs a workspace ({list(zip(shapes, sizes))})"
    if optional:
        assert any(s == 0 for s in sizes), f"{fn}: no row of the GPU table runs without a workspace"


# ---- pure-host functions against the rule their header comment states ------------------------------------------------------
def test_stat_parts_is_clamped_and_monotone():
    lib = _lib.load()
    prev = 0
    for units in list(range(-2, 40)) + [1000, 1023, 1024, 1025, 5000, 1 << 20, 1 << 40]:
        parts = lib.goalnet_stat_parts(units)
        assert 1 <= parts <= _lib.STAT_PARTS and parts >= prev, f"stat_parts({units}) = {parts} after {prev}"
        prev = parts
    assert lib.goalnet_stat_parts(1) == 1 and lib.goalnet_stat_parts(10) == 10 and lib.goalnet_stat_parts(1 << 40) == _lib.STAT_PARTS


@pytest.mark.parametrize("n,h,w,c", [(1, 1, 1, 64), (2, 9, 11, 64), (10, 11, 11, 256), (16, 13, 13, 64), (3, 224, 5, 32)])
def test_bf16_padded_layout_holds_the_guard_pixels(n, h, w, c):
    """W + 3 zero guard pixels in front of padded pixel 0 and W + 3 + 64 behind the N (H + 2)(W + 2) padded pixels"""
    lib = _lib.load()
    total, offset = ctypes.c_int64(-1), ctypes.c_int64(-1)
    assert lib.goalnet_bf16_padded_layout(n, h, w, c, ctypes.byref(total), ctypes.byref(offset)) == 0
    assert offset.value >= (w + 3) * c
    assert total.value >= offset.value + n * (h + 2) * (w + 2) * c + (w + 3 + 64) * c
    assert offset.value * 2 % 16 == 0, "padded pixel 0 must keep 16-byte alignment"


def test_kernel_names_exist_for_the_guarded_shapes():
    """the header: a compiler-spelled string "... [AL = ..., BL = ...]" for the fp32 and the 16-bit forward; the knapsack keeps its
    row in LDS up to 20 000 columns and rolls two rows in the workspace above"""
    lib = _lib.load()
    shapes = B.WS_ROWS["goalnet_conv3x3_fwd"][1]
    for dims in shapes:
        for flag in (0, 1):
            name = lib.goalnet_conv3x3_fwd_kernel_name(*dims, flag)
            assert name and b"AL" in name and b"BL" in name, f"conv3x3_fwd_kernel_name{dims}: {name!r}"
    for dims in [d for d in shapes if d[3] % 64 == 0 and d[4] % 4 == 0] + [O16, WG]:
        for forward in (0, 1):
            name = lib.goalnet_conv3x3_fwd_bf16p_kernel_name(*dims, forward)
            assert name and b"AL" in name and b"BL" in name, f"conv3x3_fwd_bf16p_kernel_name{dims}: {name!r}"
    for cap, word in ((0, b"lds"), (100, b"lds"), (19000, b"lds"), (30000, b"rolling"), (1 << 24, b"rolling")):
        name = lib.goalnet_postprocess_batch_kernel_name(4, cap)
        assert name and word in name, f"postprocess_batch_kernel_name(4, {cap}) = {name!r}"


def test_bf16_padded_layout_refuses_bad_arguments():
    lib = _lib.load()
    total, offset = ctypes.c_int64(-1), ctypes.c_int64(-1)
    none = ctypes.POINTER(ctypes.c_int64)()
    for args, code in (((2, 9, 11, 64, none, ctypes.byref(offset)), E_NULL), ((2, 9, 11, 64, ctypes.byref(total), none), E_NULL),
                       ((0, 9, 11, 64, ctypes.byref(total), ctypes.byref(offset)), E_SHAPE), ((2, 9, 11, 0, ctypes.byref(total), ctypes.byref(offset)), E_SHAPE)):
        _refused(lib, "goalnet_bf16_padded_layout", args, code, str(args[:4]))


def test_mlp_blocks_is_the_resident_grid():
    """the header: 64 resident blocks walk the layers"""
    assert _lib.load().goalnet_mlp_blocks() == 64


def test_served_predicates_agree_with_their_entry_points(monkeypatch):
    """goalnet_conv3x3_fwd_bf16p_o16_ok / goalnet_linear_bwd_dx_bf16_o16_ok / goalnet_linear_split_ok say whether the dims are served:
    0 or 1; 0 for dims outside the entry point's own divisibility rules; where 0, the entry point refuses the dims with
    GOALNET_E_SHAPE before any launch; where 1, the 256 x 256 tile is the kernel (the conv names it; the linear split has a
    workspace, which only served dims have). Served dims are never CALLED here: the pointers are fake."""
    monkeypatch.delenv("GOALNET_BF16_TILE", raising=False)
    lib = _lib.load()
    conv_row, dx_row, split_row = (ROWS[n]["args"] for n in ("goalnet_conv3x3_fwd_bf16p_o16", "goalnet_linear_bwd_dx_bf16_o16", "goalnet_linear_fwd_split"))
    assert lib.goalnet_conv3x3_fwd_bf16p_o16_ok(*O16) == 1 and lib.goalnet_linear_bwd_dx_bf16_o16_ok(*LO16) == 1
    assert b"256" in lib.goalnet_conv3x3_fwd_bf16p_kernel_name(*O16, 1)
    for dims in [(2, 9, 11, 64, 256), (10, 11, 11, 256, 512), (64, 32, 32, 64, 64), (64, 32, 32, 32, 256), (64, 32, 32, 64, 252), (0, 32, 32, 64, 256),
                 (64, 32, 32, 64, -256)]:
        assert lib.goalnet_conv3x3_fwd_bf16p_o16_ok(*dims) == 0, dims
        args = list(conv_row)
        args[5:10] = dims
        _refused(lib, "goalnet_conv3x3_fwd_bf16p_o16", args, E_SHAPE, f"dims {dims}")
    for dims in [(16, 1000, 64), (512, 1 << 18, 40), (512, (1 << 18) + 4, 256), (0, 1 << 18, 256), (37, 640, 512)]:
        assert lib.goalnet_linear_bwd_dx_bf16_o16_ok(*dims) == 0, dims
        args = list(dx_row)
        args[5:8] = dims
        _refused(lib, "goalnet_linear_bwd_dx_bf16_o16", args, E_SHAPE, f"dims {dims}")
    for parts in (2, 3):
        assert lib.goalnet_linear_split_ok(parts, *LSPLIT) == 1 and lib.goalnet_linear_fwd_split_ws_bytes(parts, *LSPLIT) > 0
        for dims in [(16, 65536, 256), (256, 65536, 40), (256, 65536 + 8, 256), (256, 1024, 256), (0, 65536, 256)]:
            assert lib.goalnet_linear_split_ok(parts, *dims) == 0 and lib.goalnet_linear_fwd_split_ws_bytes(parts, *dims) == 0, dims
            args = list(split_row)
            args[0], args[11:14] = parts, dims
            if parts == 2:
                args[16] = A
            _refused(lib, "goalnet_linear_fwd_split", args, E_SHAPE, f"parts {parts}, dims {dims}")
    for parts in (0, 1, 4):
        assert lib.goalnet_linear_split_ok(parts, *LSPLIT) == 0
    # goalnet_conv1d_bwd_small_ok: N < 64, Cin <= 256 and N * (256 / Cin) * Lo floats of dz within 48 KB (the header's comment); the row's
    # own dims are served, and tests/test_bin_classes_host.py walks every (N, B) of the two AudBl layers against the rule
    small_row = ROWS["goalnet_conv1d_bwd_small"]["args"]
    assert lib.goalnet_conv1d_bwd_small_ok(*small_row[7:13]) == 1
    for dims in [(52, 30, 60, 64, 2, 1), (62, 64, 100, 128, 2, 1), (64, 30, 30, 64, 2, 1), (4, 257, 30, 64, 2, 1), (0, 30, 30, 64, 2, 1)]:
        assert lib.goalnet_conv1d_bwd_small_ok(*dims) == 0, dims
        args = list(small_row)
        args[7:13] = dims
        _refused(lib, "goalnet_conv1d_bwd_small", args, E_SHAPE, f"dims {dims}")
    assert lib.goalnet_conv1d_bwd_small_ok(51, 30, 60, 64, 2, 1) == 1 and lib.goalnet_conv1d_bwd_small_ok(61, 64, 100, 128, 2, 1) == 1
