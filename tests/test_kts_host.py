"""CPU: temporal segmentation (csrc/kts.hip, cvml_goalnet_amd/segment.py) — extension, parity unpinned (no reference code).
The numpy restatement tests/kts_ref.py against brute force and against its planted inputs, and the argument contract of
goalnet_kts / goalnet_kts_ws_bytes, which returns before any launch (no GPU is needed and none is touched)."""
import numpy as np
import pytest
import torch

import kts_ref as R
import test_abi_contract_host as C
from cvml_goalnet_amd import _lib

# goalnet_kts joins the table of tests/test_abi_contract_host.py, whose accounting test wants a row for every entry point of the
# header: one valid call with fake addresses, and the mutations that must be refused. The rows of that file were turned into test
# cases when it was collected, so this row's mutations run below, through that file's own helpers.
KTS_DIMS = (10, 8, 3)                                 # n, d, max_cp
C.ROWS.setdefault("goalnet_kts", C.auto(
    "goalnet_kts", {1: 10, 2: 8, 3: 1, 4: 3, 5: 1, 6: 10, 7: 1.0, 8: 2, 9: 20, 17: C.BIG},
    shape=[(1, 0), (1, 8193), (2, 0), (2, 4097), (4, -1), (4, 10), (5, 0), (6, 0), (5, 11), (8, 0), (9, 18), (9, 21), (7, float("nan"))],
    align=[(16, 8)], ws=("goalnet_kts_ws_bytes", KTS_DIMS, 17)))
KTS_ROW = C.ROWS["goalnet_kts"]


def _kts_mutations():
    for i in KTS_ROW["null"]:
        yield "null", i, None, C.E_NULL
    for i, v in KTS_ROW["shape"]:
        yield "shape", i, v, C.E_SHAPE
    for i, v in KTS_ROW["align"]:
        yield "align", i, v, C.E_ALIGN


@pytest.mark.parametrize("kind,index,value,code", list(_kts_mutations()), ids=lambda v: str(v))
def test_kts_bad_argument_is_refused_before_any_launch(kind, index, value, code):
    args = list(KTS_ROW["args"])
    args[index] = value
    C._refused(_lib.load(), "goalnet_kts", args, code, f"{kind}: argument {index} = {value}")


def test_kts_row_covers_every_pointer_and_the_short_workspace():
    lib = _lib.load()
    types = _lib.PROTOTYPES["goalnet_kts"][1]
    assert set(KTS_ROW["null"]) == {i for i, t in enumerate(types[:-1]) if t is _lib.P}, "no pointer of goalnet_kts is nullable"
    need = lib.goalnet_kts_ws_bytes(*KTS_DIMS)
    assert need > 0
    args = list(KTS_ROW["args"])
    args[17] = need - 1
    C._refused(lib, "goalnet_kts", args, C.E_WORKSPACE, f"ws_bytes = {need} - 1")


def test_kts_argument_errors_do_not_need_a_gpu():
    """the style of tests/test_abi.py::test_argument_errors_do_not_need_a_gpu: codes and words of the messages"""
    lib = _lib.load()
    A = 4096
    good = dict(x=A, n=10, d=8, normalize=1, max_cp=3, lmin=1, lmax=10, vmax=1.0, skip=2, full_n=19, cps=A, n_clips=A, samples=A, cost=A,
                objective=A, status=A, ws=A, ws_bytes=1 << 30)

    def call(**kw):
        return lib.goalnet_kts(*{**good, **kw}.values(), None)

    assert call(x=None) == -1 and b"null" in lib.goalnet_last_error()
    assert call(n=0) == -2 and call(n=8193) == -2 and b"8192" in lib.goalnet_last_error()
    assert call(d=4097) == -2 and b"4096" in lib.goalnet_last_error()
    assert call(max_cp=10) == -2 and b"max_cp" in lib.goalnet_last_error()
    assert call(lmin=0) == -2 and call(lmin=5, lmax=4) == -2 and b"lmin" in lib.goalnet_last_error()
    assert call(skip=0) == -2 and b"skip_frames" in lib.goalnet_last_error()
    assert call(full_n=18) == -2 and call(full_n=21) == -2 and b"full_n_frames" in lib.goalnet_last_error()   # (n-1) skip < full_n <= n skip
    assert call(ws_bytes=lib.goalnet_kts_ws_bytes(10, 8, 3) - 1) == -4 and b"workspace" in lib.goalnet_last_error()
    assert call(max_cp=9, ws_bytes=lib.goalnet_kts_ws_bytes(10, 8, 9) - 1) == -4          # max_cp = n - 1 is inside the limits


def test_kts_ws_bytes_is_monotone_and_covers_the_tables():
    lib = _lib.load()
    ws = lib.goalnet_kts_ws_bytes
    for n, d, m in [(10, 8, 3), (97, 37, 48), (2000, 640, 500)]:
        # S, D, the n x n scatter table, I and P
        assert ws(n, d, m) >= 8 * ((n + 1) * d + (n + 1) + n * n + (m + 1) * (n + 1)) + 4 * (m + 1) * (n + 1)
    prev = 0
    for n in (4, 5, 64, 65, 1000, 8192):
        cur = ws(n, 16, 3)
        assert cur >= prev and cur > 0                           # every table is rounded up to 256 bytes: equal for n = 4 and 5
        prev = cur
    assert ws(8192, 16, 3) > ws(1000, 16, 3) > ws(64, 16, 3)
    prev = 0
    for d in (1, 2, 63, 64, 640, 4096):
        cur = ws(100, d, 3)
        assert cur >= prev and cur > 0
        prev = cur
    assert ws(100, 4096, 3) > ws(100, 1, 3)
    prev = 0
    for m in (0, 1, 2, 50, 99):
        cur = ws(100, 16, m)
        assert cur >= prev and cur > 0
        prev = cur
    assert ws(100, 16, 99) > ws(100, 16, 0)
    assert ws(8192, 4096, 8191) > 512 << 20                     # the n x n float64 table alone is 512 MiB at the limits
    for bad in [(0, 8, 0), (8193, 8, 0), (10, 0, 0), (10, 4097, 0), (10, 8, -1), (10, 8, 10)]:
        assert ws(*bad) == 0, bad


@pytest.mark.parametrize("n,d,lmin,lmax,seed", [(9, 3, 1, None, 0), (8, 5, 2, 4, 1), (7, 1, 1, 3, 2), (9, 4, 3, None, 3), (1, 2, 1, None, 4),
                                                (6, 2, 2, 2, 5)])
def test_restatement_against_brute_force(n, d, lmin, lmax, seed):
    """every segmentation enumerated: the DP's I[m][n] is the optimum for every m (+inf where none exists), and the change points it
    back-tracks to attain it"""
    X = np.random.default_rng(seed).standard_normal((n, d)).astype(np.float32)
    for normalize in (True, False):
        max_cp = n - 1
        r = R.kts(X, max_cp, lmin, lmax, normalize=normalize)
        want = R.brute_force(X, max_cp, lmin, lmax, normalize=normalize)
        assert np.array_equal(np.isfinite(r["cost"]), np.isfinite(want))
        fin = np.isfinite(want)
        scale = r["D"][n] + 1e-300
        assert np.all(np.abs(r["cost"][fin] - want[fin]) <= 1e-12 * scale)
        assert r["feasible"] == bool(fin.any())
        if r["feasible"]:
            m = r["m"]
            assert len(r["samples"]) == m and list(r["samples"]) == sorted(set(r["samples"])) and all(0 < c < n for c in r["samples"])
            assert abs(R.total_scatter(r["S"], r["D"], r["samples"], lmin, lmax) - want[m]) <= 1e-12 * scale
            obj = r["objective"]
            assert obj[m] == np.min(obj[fin]) and not np.any(obj[:m] <= obj[m])         # the smallest minimiser


@pytest.mark.parametrize("name", sorted(R.CASES))
def test_restatement_on_the_planted_cases(name):
    """the cases of tests/test_gpu_kts.py: the planted boundaries are recovered where the plant is identifiable; a planted one-sample
    segment inside 1100 samples is not worth its penalty and is dropped"""
    n, d, bounds, lmin, lmax, max_cp, returns = R.CASES[name]
    X, r = R.case(name)
    assert X.shape == (n, d) and X.dtype == np.float32
    assert r["feasible"] and r["samples"] == returns and r["m"] == len(returns)
    if name in R.PLANT_RECOVERED:
        assert r["samples"] == bounds
    obj = np.sort(r["objective"][np.isfinite(r["objective"])])
    if len(obj) > 1:
        assert obj[1] - obj[0] >= 4.9e-4, "the model-selection margin that makes the chosen m a property of the data, not of rounding"
    cps = R.to_frames(r["samples"], 7, 7 * n - 3)
    assert cps[0, 0] == 0 and cps[-1, 1] == 7 * n - 4 and np.array_equal(cps[1:, 0], cps[:-1, 1] + 1)


def test_restatement_reports_no_feasible_segmentation():
    X = R.planted(10, 4, [5], R.SIGMA)
    r = R.kts(X, 9, 4, 4)
    assert not r["feasible"] and r["m"] is None and not np.isfinite(r["cost"]).any()


def test_video_summarizer_without_change_points_needs_a_segmenter():
    from cvml_goalnet_amd import AVM, TemporalSegmenter, VideoSummarizer
    with pytest.raises(ValueError):
        VideoSummarizer(AVM(audio_included=False), None)
    with pytest.raises(ValueError):
        VideoSummarizer(AVM(audio_included=False), None, skip_frames=10, segmenter=None)
    vs = VideoSummarizer(AVM(audio_included=False), None, skip_frames=10, segmenter=TemporalSegmenter())
    assert vs.change_points is None and vs.segmenter is not None
    cps = np.array([[0, 2], [3, 5]])
    assert VideoSummarizer(AVM(audio_included=False), cps, segmenter=TemporalSegmenter()).segmenter is None     # explicit change points win


def test_segmenter_checks_its_arguments_and_fails_loudly_without_a_gpu(monkeypatch):
    from cvml_goalnet_amd import GoalnetError, TemporalSegmenter
    for kw in (dict(max_change_points=-1), dict(lmin=0), dict(lmin=3, lmax=2)):
        with pytest.raises(ValueError):
            TemporalSegmenter(**kw)
    seg = TemporalSegmenter()
    assert (seg.lmin, seg.lmax, seg.vmax, seg.normalize, seg.max_change_points) == (1, None, 1.0, True, None)
    # the default: at most one change point per 60 frames, and never more than n - 1
    assert seg.default_max_change_points(60, 600) == 10 and seg.default_max_change_points(5, 601) == 4 and seg.default_max_change_points(1, 7) == 0
    x = np.zeros((6, 4), dtype=np.float32)
    for bad in (dict(full_n_frames=61, skip_frames=10), dict(full_n_frames=50, skip_frames=10), dict(full_n_frames=60, skip_frames=0)):
        with pytest.raises(ValueError):
            seg.segment(x, **bad)
    with pytest.raises(ValueError):
        seg.segment(np.zeros(6, dtype=np.float32), 60, 10)
    with pytest.raises(ValueError):
        TemporalSegmenter(max_change_points=6).segment(x, 60, 10)
    monkeypatch.setattr(torch.cuda, "is_available", lambda: False)
    with pytest.raises(GoalnetError):
        seg.segment(x, 60, 10)
