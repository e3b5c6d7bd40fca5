"""CPU: the audio bin-length classes (tests/_bin_classes.py) against the rules they restate, the rules against the library's own
query, and the tables of the GPU tests against both sides of every class boundary. B = 1 .. 256, N = 1 .. 63."""
import ctypes

import _bin_classes as BC
from cvml_goalnet_amd import _lib

BS = range(1, 257)
NS = range(1, 64)
E_SHAPE = -2


def test_l1_and_l2_are_ceilings_and_the_conv1d_output_length():
    for b in BS:
        assert BC.l1(b) == -(-b // 2) == BC.conv1d_out(b) and BC.l2(b) == -(-BC.l1(b) // 2) == BC.conv1d_out(BC.l1(b))
        assert BC.k3(b) == 128 * BC.l2(b)
    assert [(BC.l1(b), BC.l2(b)) for b in (1, 2, 3, 4, 5)] == [(1, 1), (1, 1), (2, 1), (2, 1), (3, 2)]


def test_fit_rule_equals_the_library_query_for_every_n_and_b():
    """goalnet_conv1d_bwd_small_ok is host arithmetic: no device is needed to ask it"""
    lib = _lib.load()
    for b in BS:
        for n in range(1, 70):
            assert bool(lib.goalnet_conv1d_bwd_small_ok(n, 30, b, 64, 2, 1)) == BC.conv1_fits(n, b), (n, b)
            assert bool(lib.goalnet_conv1d_bwd_small_ok(n, 64, BC.l1(b), 128, 2, 1)) == BC.conv2_fits(n, b), (n, b)
    for dims in [(0, 30, 30, 64, 2, 1), (64, 30, 30, 64, 2, 1), (4, 257, 30, 64, 2, 1), (4, 0, 30, 64, 2, 1), (4, 30, 0, 64, 2, 1),
                 (4, 30, 30, 0, 2, 1), (4, 30, 30, 64, 0, 1), (4, 30, 30, 64, 2, -1), (4, 30, 2, 64, 2, 0)]:
        assert lib.goalnet_conv1d_bwd_small_ok(*dims) == 0, dims


def test_the_entry_point_refuses_exactly_what_the_query_refuses():
    """where the query says 0 the entry point returns GOALNET_E_SHAPE before any launch and names the query; served dims are never
    CALLED here: the pointers are fake"""
    lib = _lib.load()
    buf = (ctypes.c_float * 64)()
    a = ctypes.addressof(buf)
    for n, cin, length, cout in [(52, 30, 60, 64), (63, 30, 60, 64), (16, 30, 200, 64), (62, 64, 100, 128), (49, 64, 128, 128)]:
        assert lib.goalnet_conv1d_bwd_small_ok(n, cin, length, cout, 2, 1) == 0
        rc = lib.goalnet_conv1d_bwd_small(a, a, a, a, a, a, a, n, cin, length, cout, 2, 1, None)
        assert rc == E_SHAPE and b"goalnet_conv1d_bwd_small_ok" in lib.goalnet_last_error(), (n, cin, length, rc)
    for n, cin, length, cout in [(51, 30, 60, 64), (63, 30, 30, 64), (61, 64, 100, 128)]:
        assert lib.goalnet_conv1d_bwd_small_ok(n, cin, length, cout, 2, 1) == 1


def test_refusal_table_of_the_design_notes():
    for b, n in BC.CONV1_REFUSED_FROM.items():
        assert BC.refused_from(BC.conv1_fits, b) == n, b
    for b, n in BC.CONV2_REFUSED_FROM.items():
        assert BC.refused_from(BC.conv2_fits, b) == n, b
    # 30 bins never reach the limit below the many-frame kernels: it would take 103 frames
    assert BC.refused_from(BC.conv1_fits, 30) is None and 102 * 8 * 15 * 4 <= BC.SMALL_LDS < 103 * 8 * 15 * 4
    # the first bin length at which a batch below 64 is refused, per layer
    assert min(b for b in BS if BC.refused_from(BC.conv1_fits, b)) == 49 and min(b for b in BS if BC.refused_from(BC.conv2_fits, b)) == 193


def test_skinny_classes_switch_at_the_documented_bin_lengths():
    ks = {b: BC.skinny_fwd_splits(BC.k3(b)) for b in BS}
    assert all(ks[b] == 1 for b in range(1, 17)) and ks[17] == 2
    assert all(2 <= ks[b] <= 7 for b in range(17, 113)) and ks[112] == 7 and ks[113] == 8
    assert all(BC.skinny_fwd_class(BC.k3(b)) == ("direct" if b <= 16 else "<MR,1,1>" if b <= 112 else "<MR,4,1>") for b in BS)
    assert all(BC.skinny_bwd_class(BC.k3(b)) == ("<MR,16>" if b >= 129 else "<MR,4>") for b in BS)
    assert BC.k3(128) == 4096 and BC.k3(129) == 4224
    assert BC.linear3_engine(16) == "skinny" and BC.linear3_engine(17) == "gemm"


def test_conv1d_rows_stand_on_both_sides_of_every_boundary():
    rows = BC.CONV1D_ROWS
    assert len(set(rows)) == len(rows) == 23
    bs = {b for _, b in rows}
    # B mod 4 is the class of the window cut: all four among the new rows (B = 2 is the only B = 2 mod 4 of them: l1 = 1), and all four
    # again at l1 >= 3 once the rows test_audbl_conv1d had before (B = 30) are counted, which run the same code
    assert {1, 2, 3} <= bs and {b % 4 for b in bs} == {0, 1, 2, 3}
    assert {b % 4 for _, b in rows + BC.CONV1D_EXISTING if BC.l1(b) >= 3} == {0, 1, 2, 3}
    # the parity of B and of l1 decides how the last window of each layer is cut
    assert {(b % 2, BC.l1(b) % 2) for b in bs} == {(0, 0), (0, 1), (1, 0), (1, 1)}
    # skinny KS 1 | 2 in the chained shapes
    assert {BC.skinny_fwd_splits(BC.k3(b)) for b in (16, 17)} == {1, 2}
    for fits, layer in ((BC.conv1_fits, "conv1"), (BC.conv2_fits, "conv2")):
        small = [(n, b) for n, b in rows if n <= BC.SMALL_MAX_N]
        assert any(fits(n, b) for n, b in small) and any(not fits(n, b) for n, b in small), layer
        # a boundary pair: the same B, n and n + 1, fit and no fit
        assert any(fits(n, b) and (n + 1, b) in rows and not fits(n + 1, b) for n, b in small), layer
    assert BC.conv1_fits(51, 60) and not BC.conv1_fits(52, 60) and not BC.conv1_fits(63, 60) and BC.conv2_fits(63, 60)
    assert BC.conv2_fits(61, 200) and not BC.conv2_fits(62, 200) and not BC.conv1_fits(61, 200)
    # both layers in one launch, conv1 multi / conv2 one launch, both multi: every mixture the per-layer dispatch can produce below 64
    mixes = {(BC.conv1_fits(n, b), BC.conv2_fits(n, b)) for n, b in rows if n <= BC.SMALL_MAX_N}
    assert mixes == {(True, True), (False, True), (False, False)}
    assert {n for n, _ in BC.CONV1D_MANY} == {64, 70, 515} and all(n > BC.SMALL_MAX_N for n, _ in BC.CONV1D_MANY)


def test_linear3_rows_stand_on_both_sides_of_every_boundary():
    assert len(BC.LINEAR3_ROWS) == 32 and set(BC.LINEAR3_M) == {10, 16, 17, 60}
    ks = [BC.skinny_fwd_splits(128 * k) for k in BC.LINEAR3_L2]
    assert ks == [1, 1, 2, 4, 7, 8, 8, 9]
    assert [BC.skinny_fwd_class(128 * k) for k in (4, 5, 28, 29)] == ["direct", "<MR,1,1>", "<MR,1,1>", "<MR,4,1>"]
    assert [128 * k for k in (32, 33)] == [4096, 4224] and [BC.skinny_bwd_class(128 * k) for k in (32, 33)] == ["<MR,4>", "<MR,16>"]
    assert 15 == BC.l2(60) and 128 * 15 % BC.KT != 0, "B = 60: a ragged last slab"
    # every l2 is one some bin length gives
    assert set(BC.LINEAR3_L2) <= {BC.l2(b) for b in BS}


def test_step_cells_land_in_the_class_their_comment_states():
    assert len(BC.STEP_CELLS) == 6
    for (precision, head, mode, n, b), classes in BC.STEP_CELLS:
        assert BC.step_classes(n, b) == classes, (n, b)
    by = {(n, b): c for (_, _, _, n, b), c in BC.STEP_CELLS}
    assert by[(10, 60)]["ks"] == 4 and BC.k3(60) % BC.KT == 384
    assert not by[(60, 60)]["conv1_fits"] and by[(60, 60)]["conv2_fits"] and by[(60, 60)]["engine"] == "gemm"
    assert by[(10, 15)]["ks"] == 1 and BC.k3(15) == 512
    assert (by[(10, 2)]["l1"], by[(10, 2)]["l2"], BC.k3(2)) == (1, 1, 128)
    assert by[(32, 17)]["l1"] % 2 == 1 and 17 % 2 == 1
    frames, sub, (b0, b1) = BC.LOOP_ROW
    assert BC.l2(b0) == BC.l2(b1) and BC.l1(b0) == BC.l1(b1) and b0 != b1 and frames % sub != 0
