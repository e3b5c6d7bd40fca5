"""CPU: the host side of fine-tuning — the range merging of avm.trainable_ranges, the argument contract of
goalnet_adam_step_dev_ranges (every refusal returns before any launch, so no GPU is needed), the comparison of tests/_freeze_case.py
with the oracle standing in for the device (and two wrong "devices" that it must reject), and the oracle-plus-torch-Adam helper against
a fixture recorded from the reference itself."""
import ctypes
import os
import zlib

import numpy as np
import pytest
import torch

import _freeze_case as FC
import test_abi_contract_host as C
from cvml_goalnet_amd import _lib, synth
from cvml_goalnet_amd.avm import AVM, trainable_ranges

HW3, L2 = 81, 8                                   # 40 x 40 frames, 30 bins
E_NULL, E_SHAPE, E_ALIGN = -1, -2, -3
A, A2, A3, A4 = 4096, 8192, 12288, 16384          # fake, 16-byte aligned "device addresses": never dereferenced


def _specs():
    m = AVM(audio_included=True)
    return m, m._param_specs(HW3, L2)


# ---- trainable_ranges ------------------------------------------------------------------------------------------------------------------
def test_trainable_ranges_merge_neighbours():
    m, specs = _specs()
    names = [s.name for s in specs]
    by = {s.name: s for s in specs}
    last = max(specs, key=lambda s: s.offset)
    assert trainable_ranges(specs, frozenset(), {}) == [(0, last.offset + last.numel, 0)]
    f1 = trainable_ranges(specs, FC.frozen_set("F1", names), {})
    b5 = by["visbl.linear5.bias"]
    assert len(f1) == 1 and f1[0][0] == 0 and f1[0][0] + f1[0][1] <= b5.offset, f1      # fusion.* and audbl.*: one range in front of visbl.*
    f3 = trainable_ranges(specs, FC.frozen_set("F3", names), {})
    w5 = by["visbl.linear5.weight"]
    assert f3 == [(0, b5.offset + b5.numel, 0), (by["visbl.bnorm3.weight"].offset, last.offset + last.numel - by["visbl.bnorm3.weight"].offset, 0)]
    assert f3[0][0] + f3[0][1] <= w5.offset and f3[1][0] >= w5.offset + w5.numel
    f5 = trainable_ranges(specs, FC.frozen_set("F5", names), {})
    assert 1 < len(f5) <= _lib.ADAM_RANGES_MAX
    for f in ("F1", "F2", "F3", "F4", "F5", "F6"):
        frozen = FC.frozen_set(f, names)
        rs = trainable_ranges(specs, frozen, {})
        assert all(b % 64 == 0 and c > 0 for b, c, _ in rs) and all(x[0] + x[1] <= y[0] for x, y in zip(rs, rs[1:]))
        covered = lambda s: any(b <= s.offset and s.offset + s.numel <= b + c for b, c, _ in rs)      # noqa: E731
        touched = lambda s: any(b < s.offset + s.numel and s.offset < b + c for b, c, _ in rs)       # noqa: E731
        assert all(covered(s) != (s.name in frozen) and touched(s) != (s.name in frozen) for s in specs), f
    # tensors that sat out different numbers of steps do not share a range
    rs = trainable_ranges(specs, frozenset(), {"fusion.9.weight": 2, "fusion.9.bias": 2})
    assert [r[2] for r in rs] == [0, 2, 0] and rs[1][0] == by["fusion.9.weight"].offset


def test_sat_out_bookkeeping_over_the_freeze_schedule():
    m, specs = _specs()
    m._specs = specs
    names = [s.name for s in specs]
    seen = []
    for set_id in FC.SCHEDULE:
        frozen = FC.frozen_set(set_id, names)
        for _ in range(3):                           # three optimizer steps per phase, as in tests/test_gpu_freeze.py
            seen.append(tuple(trainable_ranges(specs, frozen, m._sat_out)))
            m._count_sat_out(frozen)                 # what AVM.adam_step / VideoTrainer's replay bookkeeping do after the update
    assert len(set(seen[0:3])) == 1 and len(set(seen[3:6])) == 1 and len(set(seen[6:9])) == 1, "stable inside a phase: graphs stay valid"
    assert len({seen[0], seen[3], seen[6]}) == 3, "every phase has its own signature"
    b5 = m.spec("visbl.linear5.bias")
    assert [r[2] for r in seen[6]] == [0, 3] and seen[6][1][0] == b5.offset, "the re-thawed trunk runs 3 steps behind"
    assert all(m._sat_out[k] == 3 for k in FC.frozen_set("F1", names)) and len(m._sat_out) == 14


def test_flags_set_on_lazy_parameters_are_kept():
    m = AVM(audio_included=True)
    m.visbl.requires_grad_(False)
    m.fusion["12"].requires_grad_(False)
    assert m._frozen_names() == FC.frozen_set("F1", dict(m.named_parameters())) | {"fusion.12.weight", "fusion.12.bias"}
    assert m.trainable_signature() == tuple(sorted(m._frozen_names()))
    m.requires_grad_(True)
    assert m._frozen_names() == frozenset() and m.trainable_signature() == ()


# ---- the argument contract of goalnet_adam_step_dev_ranges -----------------------------------------------------------------------------
def _arr(*ranges):
    return (_lib.AdamRange * len(ranges))(*[_lib.AdamRange(*r) for r in ranges])


GOOD = _arr((0, 128, 0), (192, 1001, 2), (2048, 64, 5))


def _valid():
    return [A, A2, A3, A4, GOOD, 3, 1e-3, 0.9, 0.999, 1e-8, A, 1.0, None, 0, 0, 0, None, None]


REFUSALS = [(f"null pointer {i}", {i: None}, E_NULL) for i in (0, 1, 2, 3, 4, 10)] + [
    ("no range", {5: 0}, E_SHAPE),
    ("33 ranges", {4: _arr(*[(64 * i, 4, 0) for i in range(33)]), 5: 33}, E_SHAPE),
    ("unsorted", {4: _arr((192, 64, 0), (0, 128, 0)), 5: 2}, E_SHAPE),
    ("overlapping", {4: _arr((0, 128, 0), (124, 64, 0)), 5: 2}, E_SHAPE),
    ("empty range", {4: _arr((0, 0, 0)), 5: 1}, E_SHAPE),
    ("negative begin", {4: _arr((-4, 8, 0)), 5: 1}, E_SHAPE),
    ("negative skipped", {4: _arr((0, 128, -1)), 5: 1}, E_SHAPE),
    ("misaligned range", {4: _arr((0, 128, 0), (130, 64, 0)), 5: 2}, E_ALIGN),
    ("misaligned p", {0: A + 4}, E_ALIGN),
    ("misaligned v", {3: A4 + 8}, E_ALIGN),
    ("shadow offset", {12: A2, 13: 2, 14: 64}, E_SHAPE),
    ("shadow length", {12: A2, 13: 0, 14: 62}, E_SHAPE),
    ("misaligned shadow", {12: A2 + 4, 13: 0, 14: 64}, E_ALIGN),
]


# goalnet_adam_step_dev_ranges joins the table of tests/test_abi_contract_host.py, whose accounting test wants a row for every entry
# point of the header (as tests/test_kts_host.py does for goalnet_kts): the valid call, its required pointers (shadow_16 and bad_step
# are nullable) and the single-argument mutations. That file's rows became test cases when it was collected, so every refusal, the
# ones inside the range array included, runs below.
C.ROWS.setdefault("goalnet_adam_step_dev_ranges", C.row(_valid(), null=(0, 1, 2, 3, 4, 10), shape=[(5, 0), (5, 33)],
                                                        align=[(0, A + 4), (3, A4 + 8)]))


def test_the_contract_table_row_lists_every_required_pointer():
    r = C.ROWS["goalnet_adam_step_dev_ranges"]
    types = _lib.PROTOTYPES["goalnet_adam_step_dev_ranges"][1]
    pointers = {i for i, t in enumerate(types[:-1]) if t is _lib.P or t is ctypes.POINTER(_lib.AdamRange)}
    assert set(r["null"]) == pointers - {12, 16} and len(r["args"]) == len(types)
    assert {(f"null pointer {i}", E_NULL) for i in r["null"]} <= {(w, c) for w, _, c in REFUSALS}


@pytest.mark.parametrize("what,mutation,code", REFUSALS, ids=[r[0] for r in REFUSALS])
def test_adam_ranges_refuses_before_any_launch(what, mutation, code):
    lib = _lib.load()
    args = _valid()
    for i, v in mutation.items():
        args[i] = v
    rc = lib.goalnet_adam_step_dev_ranges(*args)
    assert rc == code, (what, rc, lib.goalnet_last_error())
    assert lib.goalnet_last_error(), what


# ---- the comparison, with the oracle standing in for the device ----------------------------------------------------------------------------
@pytest.fixture(scope="module")
def schedule():
    p0 = FC.start_params()
    aud, vis, lab = FC.schedule_inputs(FC.SUB)
    return p0, (aud, vis, lab), FC.oracle_schedule(p0, aud, vis, lab)


def _as_device(steps):
    return [dict(s, grads=dict(s["grads"]), params={k: v.clone() for k, v in s["params"].items()}) for s in steps]


def test_compare_accepts_the_oracle_and_rejects_wrong_devices(schedule):
    p0, inputs, ref = schedule
    FC.compare_schedule(_as_device(ref), ref, p0)
    # a "device" that updated a frozen tensor, by one part in 2^20 of one element
    dev = _as_device(ref)
    dev[1]["params"]["visbl.conv3.weight"].view(-1)[7] *= 1 + 2.0 ** -20
    with pytest.raises(AssertionError, match="frozen and moved"):
        FC.compare_schedule(dev, ref, p0)
    # a "device" whose optimizer has ONE step count: after the thaw visbl.* is bias-corrected with t = 3 instead of 2
    wrong = FC.oracle_schedule(p0, *inputs, per_tensor_count=False)
    for k in FC.frozen_set("F1", p0):
        assert torch.equal(wrong[1]["params"][k], ref[1]["params"][k])
    with pytest.raises(AssertionError, match=r"step 2: visbl\..* exceeds its Adam-sensitivity bound"):
        FC.compare_schedule(wrong, ref, p0)
    d = (wrong[2]["params"]["visbl.conv3.weight"] - ref[2]["params"]["visbl.conv3.weight"]).abs()
    assert d.median().item() > 0.05 * FC.LR, "the global count is off by a visible fraction of lr on a typical element"


# ---- the helper against the reference's own run ----------------------------------------------------------------------------------------
def test_oracle_schedule_matches_the_reference_fixture():
    """tests/golden/avm_freeze_a1_n10_h40_p0.npz: utils.AVM with dropout p = 0 and stock torch.optim.Adam through the schedule (one
    10-frame step per phase), recorded by tests/golden/make_golden_freeze.py"""
    g = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "avm_freeze_a1_n10_h40_p0.npz"))
    p0 = FC.start_params()
    steps = FC.oracle_schedule(p0, *FC.schedule_inputs(FC.SUB), dropout=False)
    assert int(g["meta|steps"][0]) == len(steps) == 3
    for i, s in enumerate(steps):
        assert abs(s["loss"] - float(g[f"s{i}.loss"][0])) < 1e-6 * max(1.0, abs(s["loss"]))
        assert np.allclose(s["pred"].numpy(), g[f"s{i}.pred"], rtol=1e-5, atol=1e-6)
        for k, v in s["params"].items():
            a = v.double().reshape(-1).numpy()
            idx = synth.sample_indices(a.size, 16, zlib.crc32(k.encode()) & 0xFFFF)
            assert np.allclose(a[idx], g[f"s{i}.param.{k}|samples"], rtol=1e-5, atol=1e-7), (i, k)
            want = g[f"s{i}.param.{k}|stats"]
            assert np.allclose([a.sum(), (a * a).sum()], want, rtol=1e-5, atol=1e-6), (i, k)
    frozen = FC.frozen_set("F1", p0)
    for k in frozen:      # the reference leaves the frozen trunk bit-unchanged in the second step: equal checksums
        assert np.array_equal(g[f"s0.param.{k}|stats"], g[f"s1.param.{k}|stats"]), k
