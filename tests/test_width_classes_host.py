"""CPU: the tables of tests/_width_classes.py against the dispatch rules restated there. Every kernel class of conv1 and of the pool /
BatchNorm rounds that a frame can select must be selected by a table row, on both sides of every boundary between two classes; a row
that is the only cover of a class cannot be removed without one of these assertions failing. No GPU, no kernel: the rules are the
dispatchers' arithmetic, each next to the lines it mirrors."""
import _width_classes as WC


def _boundaries(rule, widths):
    """[(last width of a class, first width of the next)] of `rule` over consecutive widths"""
    return [(a, b) for a, b in zip(widths, widths[1:]) if rule(a) != rule(b)]


def test_conv1_forward_rows_sit_on_both_sides_of_every_class_boundary():
    edges = _boundaries(WC.conv1_fwd_class, range(1, 4000))
    assert edges == [(80, 81), (164, 165), (251, 252), (335, 336), (1622, 1623)]
    assert [WC.conv1_fwd_class(a) for a, _ in edges] + [WC.conv1_fwd_class(1623)] == list(WC.CONV1_FWD_CLASSES)
    have = {w for _, _, w in WC.CONV1_ROWS}
    for a, b in edges[:-1]:
        assert a in have and b in have, (a, b)
    # v2 -> v1: the first v1 width runs with no switch set; v2 is run from its first width (a frame of 1 622 pixels serves no model)
    assert 1623 in have and WC.conv1_fwd_class(1623) == "v1"
    for cls in WC.CONV1_FWD_CLASSES:
        assert any(WC.conv1_fwd_class(w) == cls for w in have), cls
    # one table row per edge side: each is the only cover of its side
    assert sorted(w for _, _, w in WC.CONV1_FWD_EDGES) == sorted(x for e in edges[:-1] for x in e)


def test_conv1_weight_gradient_rows_reach_every_kernel_and_the_lds_limit():
    cls = {row: WC.conv1_wgrad_class(row[2]) for row in WC.CONV1_WGRAD_ROWS}
    assert cls == {(2, 7, 8): "v3", (2, 8, 44): "v3", (2, 7, 536): "v3", (1, 7, 537): "v1", (2, 7, 81): "v2"}
    assert set(cls.values()) == set(WC.CONV1_WGRAD_CLASSES)
    assert [WC.conv1_out(w) for _, _, w in WC.CONV1_WGRAD_ROWS] == [4, 16, 180, 181, 29]
    # 536 is the widest frame of v3 / v2 and 537 the first of v1
    assert all(WC.conv1_wgrad_class(w) != "v1" for w in range(1, 537)) and all(WC.conv1_wgrad_class(w) == "v1" for w in range(537, 4000))
    assert (9 * 3 * 180 + 180 * 64) * 4 == 65520 <= WC.LDS < (9 * 3 * 181 + 181 * 64) * 4
    # v3 needs Wo % 4 == 0: of the forward's edge widths only 80 and 164 have it, every other one is a v2 row as well
    assert [WC.conv1_wgrad_class(w) for _, _, w in WC.CONV1_FWD_EDGES] == ["v3", "v2", "v3", "v2", "v2", "v2", "v2", "v2"]
    assert set(WC.CONV1_WGRAD_ROWS) <= set(WC.CONV1_ROWS)


def test_conv1_row_loop_rows_make_a_block_walk_several_rows():
    (a, b) = WC.CONV1_ROW_LOOPS
    assert a == (1030, 7, 8) and b == (513, 7, 252) and {a, b} <= set(WC.CONV1_ROWS)
    assert a[0] * WC.conv1_out(a[1]) == 4120 and b[0] * WC.conv1_out(b[1]) == 2052
    assert WC.rows_per_block(a[0], a[1], WC.CONV1_FWD_GRID) == (2, 3) and WC.rows_per_block(a[0], a[1], WC.CONV1_WGRAD_GRID) == (5, 6)
    assert WC.rows_per_block(b[0], b[1], WC.CONV1_FWD_GRID) == (1, 2) and 2052 - WC.CONV1_FWD_GRID == 4      # blocks 0 .. 3 only
    assert WC.rows_per_block(b[0], b[1], WC.CONV1_WGRAD_GRID) == (2, 3)
    assert (WC.conv1_fwd_class(a[2]), WC.conv1_wgrad_class(a[2])) == ("v3<3>", "v3")
    assert (WC.conv1_fwd_class(b[2]), WC.conv1_wgrad_class(b[2])) == ("v3<12>", "v2")
    # every other conv1 row is one row per block at most: the loops are these two rows' alone
    for n, h, w in WC.CONV1_ROWS:
        if (n, h, w) not in (a, b):
            assert n * WC.conv1_out(h) <= WC.CONV1_WGRAD_GRID


def test_pool_rows_sit_on_both_sides_of_every_forward_and_backward_boundary():
    widths = range(3, 400)
    fwd = _boundaries(WC.pool_fwd_class, widths)
    bwd = _boundaries(WC.pool_bwd_class, widths)
    assert fwd == [(32, 33), (64, 65), (96, 97), (128, 129), (160, 161), (170, 171)]
    assert bwd == [(32, 33), (34, 35), (64, 65), (66, 67), (96, 97), (98, 99), (128, 129), (130, 131), (134, 135)]
    have = {wc for _, _, wc, c, _ in WC.POOL_ROWS if c == 32}
    assert have == set(WC.POOL_WIDTHS)
    for a, b in fwd + bwd:
        assert a in have and b in have, (a, b)
    assert [WC.pool_fwd_class(a) for a, _ in fwd] + [WC.pool_fwd_class(171)] == list(WC.POOL_FWD_CLASSES)
    assert [WC.pool_bwd_class(a) for a, _ in bwd] + [WC.pool_bwd_class(135)] == list(WC.POOL_BWD_CLASSES)
    # the widest v2 widths and the first v1 ones
    assert WC.pool_fwd_class(170) == ("v2", 6) and WC.pool_fwd_class(171) == ("v1",)
    assert WC.pool_bwd_class(134) == (5, 5) and WC.pool_bwd_class(135) == ("v1",)
    # every (k, k + 1) class has exactly two widths, and both are rows
    for k in (1, 2, 3, 4):
        two = [wc for wc in widths if WC.pool_bwd_class(wc) == (k, k + 1)]
        assert two == [32 * k + 1, 32 * k + 2] and set(two) <= set(WC.POOL_WIDTHS)
    # each width runs with one partial row per frame and with 12
    for wc in WC.POOL_WIDTHS:
        assert {p for n, hc, w, c, p in WC.POOL_ROWS if (w, c) == (wc, 32)} == {0, 12}
    for wc in WC.POOL_WIDTHS_C64:
        assert {p for n, hc, w, c, p in WC.POOL_ROWS if (w, c) == (wc, 64)} == {0, 12}
    assert {WC.pool_bwd_class(wc) for wc in WC.POOL_WIDTHS_C64} == {(1, 2), (3, 4), (4, 5), ("v1",)}
    assert all((n, hc) == (2, 5) for n, hc, _, _, _ in WC.POOL_ROWS)


def test_the_default_case_of_the_backward_switch_is_unreachable_under_the_lds_limit():
    assert WC.POOL_BWD_UNREACHABLE == (5, 6) and WC.POOL_BWD_UNREACHABLE not in WC.POOL_BWD_CLASSES
    # (5, 6): a pooled row of at most 160 pixels whose conv row has more, i.e. Wc in {161, 162}; the ring rows stop at Wc = 134
    need = [wc for wc in range(3, 2000) if ((wc - 2 + 31) // 32, (wc + 31) // 32) == (5, 6)]
    assert need == [161, 162]
    assert all(3 * (wc + 2) * WC.CS * 5 > WC.LDS for wc in need) and 3 * (134 + 2) * WC.CS * 5 <= WC.LDS < 3 * (135 + 2) * WC.CS * 5
    assert all(WC.pool_bwd_class(wc) != (5, 6) for wc in range(3, 2000))


def test_band_rows_split_a_frame_into_several_row_bands():
    # hc = 5: one band whatever `parts` is
    assert WC.row_bands(12, 2, 5 - 2) == 1 == WC.row_bands(12, 2, 5) == WC.row_bands(2, 2, 5)
    for n, hc, wc, c, parts in WC.POOL_BAND_ROWS:
        assert WC.row_bands(parts, n, hc - 2) == 2 and WC.row_bands(parts, n, hc) == 3
    assert [WC.pool_bwd_class(wc) for _, _, wc, _, _ in WC.POOL_BAND_ROWS] == [(1, 2), (2, 3), (3, 4), (4, 5), (5, 5), ("v1",)]
    assert [WC.pool_fwd_class(wc)[1] for _, _, wc, _, _ in WC.POOL_BAND_ROWS] == [2, 3, 4, 5, 5, 6]


def test_rows_added_to_the_bit_identity_tests_reach_the_classes_they_did_not():
    # eval form (STATS = false): fp32 at 2 .. 5 passes; the 16-bit kinds at 4 and 5 passes, the _y16 ones through the integer-key kernel
    f32 = [wc for c, wc, kind in WC.EVAL_FWD_ROWS if kind == "f32"]
    assert [WC.pool_fwd_class(wc) for wc in f32] == [("v2", 2), ("v2", 3), ("v2", 4), ("v2", 5)]
    assert [WC.pool_bwd_class(wc) for wc in f32] == [(1, 2), (2, 3), (3, 4), (4, 5)]
    for kind in ("bf16", "fp16", "bf16_y16", "fp16_y16"):
        rows = [(c, wc) for c, wc, k in WC.EVAL_FWD_ROWS if k == kind]
        assert [wc for _, wc in rows] == [98, 130]
        if kind.endswith("_y16"):
            assert [WC.pool_fwd_k16_class(wc, c) for c, wc in rows] == [(4, 4), (4, 5)]
    # integer-key kernel: old and new rows together reach all twelve (WPL, NPW); the old ones four of them
    old = {WC.pool_fwd_k16_class(wc, c) for wc, c in WC.K16_EXISTING}
    new = [WC.pool_fwd_k16_class(wc, c) for _, _, wc, c, _ in WC.K16_ROWS]
    assert old == {(4, 1), (4, 2), (4, 3), (2, 1)}
    assert new == [(4, 4), (4, 5), (4, 6), (4, 6), (2, 2), (2, 4), (2, 6), (2, 3), (2, 5)]
    assert old | set(new) == set(WC.POOL_K16_CLASSES) and not old & set(new)
    assert {wc for _, _, wc, c, _ in WC.K16_ROWS if c == 64} == {98, 130, 162, 170}
    assert {wc for _, _, wc, c, _ in WC.K16_ROWS if c == 32} >= {40, 98, 170}
    assert {kind for *_, kind in WC.K16_ROWS} == {"relu", "signed", "special"}
    # 16-bit pooled activations and gradients: every (k, k + 1) backward class and the widest (5, 5)
    assert [WC.pool_bwd_class(wc) for _, _, wc, _ in WC.H16_ROWS] == [(1, 2), (2, 3), (3, 4), (4, 5), (5, 5)]
    assert [wc for _, _, wc, _ in WC.H16_ROWS] == [34, 66, 98, 130, 134] and all(hc == 5 for _, hc, _, _ in WC.H16_ROWS)


def test_the_whole_step_frame_lands_in_the_classes_it_is_there_for():
    from cvml_goalnet_amd import AVM
    assert AVM._sizes(*WC.STEP_HW) == WC.STEP_GEOMETRY
    (h1, w1), (h2, w2), (h3, w3), (hp3, wp3) = WC.STEP_GEOMETRY
    assert (w1, w2, w3, wp3) == (102, 100, 98, 96)
    assert WC.conv1_fwd_class(WC.STEP_HW[1]) == WC.STEP_CLASSES["conv1_fwd"] == "v3<12>"
    assert (WC.pool_fwd_class(w2), WC.pool_fwd_class(w3)) == WC.STEP_CLASSES["pool_fwd"] == (("v2", 4), ("v2", 4))
    assert (WC.pool_bwd_class(w2), WC.pool_bwd_class(w3)) == WC.STEP_CLASSES["pool_bwd"] == ((4, 4), (3, 4))
    assert WC.STEP_CELLS == (("fp32", "regression", True, "train", 10, (40, 300)), ("bf16", "regression", False, "train", 10, (40, 300)))
    # the launch counts, by the rule tests/_mode_case.py states: the one-launch kernel takes a train-mode block whose conv output and
    # pooled activation are fp32, c <= 512 and n * hc * wc * c <= 2^20. Block 1 is fp32 in every precision; blocks 2 and 3 are over.
    n = 10
    elems = [n * h1 * w1 * 64, n * h2 * w2 * 256, n * h3 * w3 * 512]
    assert elems == [979200, 3328000, 5519360]
    small = sum(e <= WC.SMALL_BN_ELEMS for e in elems)
    assert (small, 3 - small, 0) == WC.STEP_LAUNCHES == (1, 2, 0)
