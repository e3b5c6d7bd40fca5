"""Rank correlation on the GPU: how well per-frame importances order the frames the way each annotator does.

EXTENSION, PARITY UNPINNED (no reference code). The reference's only quality figure is the knapsack F-score (`utils.py:552-643`),
which on TVSum is dominated by the clip lengths the knapsack sees (hence `baseline.py`: ten untrained models for a chance level).
The figure the field reports beside it is the rank correlation of the predicted importances with every annotator's per-frame
scores — Kendall's tau-b and Spearman's rho, ties handled, averaged over the annotators — next to the leave-one-out figure of the
annotators themselves. `RankEvaluator` keeps a video's (A, full_n) score matrix resident on the device, as `SummaryEvaluator` keeps
the change points, and computes every (prediction, annotator) pair in one call of csrc/rankcorr.hip. The oracle is
scipy.stats.kendalltau (variant b) / spearmanr through the fixtures tests/golden/rankcorr_*.npz and, for the integer counts, the
numpy restatement tests/rankcorr_ref.py; the definitions are written out in DESIGN.md §4.9.

No CPU fallback: without the library / a GPU the calls raise.
"""
from __future__ import annotations

from dataclasses import dataclass
from typing import Tuple, Union

import numpy as np
import torch

from . import _lib
from ._lib import GoalnetError, check
from .ops import _s

MAX_N, MAX_ANNOTATORS, MAX_BATCH = 65536, 128, 65535
COUNT_NAMES = ("S", "tx", "ty", "txy", "cxy", "cxx", "cyy", "bad")


@dataclass
class RankCorrelation:
    """One prediction vector (`ev(pred)`), or B of them with a leading B on every field (`ev.batch(preds)`)."""
    kendall: Union[float, np.ndarray]          # mean of the defined tau-b over the annotators (NaN when none is defined)
    spearman: Union[float, np.ndarray]         # mean of the defined rho
    kendall_per_annotator: np.ndarray          # (A,) float64; NaN for a constant annotator, a constant or non-finite prediction
    spearman_per_annotator: np.ndarray         # (A,) float64
    n_valid: np.ndarray                        # (2,) int32: how many tau / rho entered the means
    counts: np.ndarray                         # (A, 8) int64: S, tx, ty, txy, cxy, cxx, cyy, bad (COUNT_NAMES)
    nonfinite: Union[bool, np.ndarray]         # a NaN or inf among the values compared: everything of that row is NaN


@dataclass
class HumanConsistency:
    """`ev.human()`: every annotator against every OTHER annotator."""
    kendall: float                             # mean of kendall_per_annotator over the annotators where it is defined
    spearman: float
    kendall_per_annotator: np.ndarray          # (A,) float64: mean of the defined tau-b against the A - 1 others
    spearman_per_annotator: np.ndarray         # (A,) float64
    kendall_matrix: np.ndarray                 # (A, A) float64, symmetric; the diagonal is NaN (left out, not 1)
    spearman_matrix: np.ndarray                # (A, A) float64
    n_valid: np.ndarray                        # (A, 2) int32: how many others entered each annotator's means


def _device(device, *tensors):
    if not torch.cuda.is_available():
        raise GoalnetError("rank correlation runs on the GPU (torch.cuda.is_available() is False); there is no CPU fallback")
    if device is not None:
        return torch.device(device)
    for t in tensors:
        if torch.is_tensor(t) and t.is_cuda:
            return t.device
    return torch.device("cuda:0")


def _tensor(v):
    return v.detach() if torch.is_tensor(v) else torch.from_numpy(np.ascontiguousarray(np.asarray(v)))


def _rows(v, what: str) -> torch.Tensor:
    t = _tensor(v)
    if t.dim() == 1:
        t = t[None, :]
    if t.dim() != 2 or t.shape[0] < 1 or t.shape[1] < 1:
        raise ValueError(f"{what} must be (rows, n) or (n,) with at least one element, got {tuple(t.shape)}")
    return t


def _prediction_rows(t: torch.Tensor, N: int, batched: bool, why: str) -> torch.Tensor:
    """(N,) or (N, 1) -> (1, N); batched: (B, N) or (B, N, 1) -> (B, N). Anything else is a ValueError."""
    if batched:
        if t.dim() == 3 and t.shape[-1] == 1:
            t = t[:, :, 0]
        if t.dim() != 2 or t.shape[0] < 1 or t.shape[1] != N or t.shape[0] > MAX_BATCH:
            raise ValueError(f"predictions must be (B, {N}) with 1 <= B <= {MAX_BATCH} ({why}), got {tuple(t.shape)}")
        return t
    if t.dim() == 2 and t.shape[-1] == 1:
        t = t[:, 0]
    if t.dim() != 1 or t.shape[0] != N:
        raise ValueError(f"predictions must be ({N}, 1) or ({N},) ({why}), got {tuple(t.shape)}")
    return t[None, :]


def _packed_bytes(B: int, A: int) -> int:
    """bytes of the one result buffer: [counts int64 [B][A][8] | tau float64 [B][A] | rho [B][A] | mean [B][2] | n_valid int32 [B][2]
    | status int32 [B]]. No padding: every byte is written by the call, so two calls on the same inputs give the same buffer."""
    return 8 * (8 * B * A + 2 * B * A + 2 * B) + 4 * (2 * B + B)


def _launch(lib, x: torch.Tensor, ldx: int, x_repeat: int, y: torch.Tensor, ldy: int, y_stride: int, B: int, A: int, n: int) -> torch.Tensor:
    """x, y: float32 on one device. Returns the packed uint8 buffer; nothing has been synchronised."""
    packed = torch.empty(_packed_bytes(B, A), dtype=torch.uint8, device=x.device)
    o_tau = 8 * B * A                                               # offsets in 8-byte words
    o_rho, o_mean, o_valid = o_tau + B * A, o_tau + 2 * B * A, o_tau + 2 * B * A + 2 * B
    base = packed.data_ptr()
    with torch.cuda.device(x.device):
        check(lib.goalnet_rank_corr(x.data_ptr(), ldx, x_repeat, y.data_ptr(), ldy, y_stride, B, A, n, base, base + 8 * o_tau,
                                    base + 8 * o_rho, base + 8 * o_mean, base + 8 * o_valid, base + 8 * o_valid + 8 * B, _s()), "rank_corr")
    return packed


def _unpack(host: torch.Tensor, B: int, A: int):
    """the packed buffer on the host -> counts (B, A, 8), tau (B, A), rho (B, A), mean (B, 2), n_valid (B, 2), status (B,)"""
    h = host.numpy()
    o, nf = 64 * B * A, 8 * (2 * B * A + 2 * B)
    counts = h[:o].view(np.int64).reshape(B, A, 8).copy()
    f = h[o:o + nf].view(np.float64)
    tau, rho, mean = f[:B * A].reshape(B, A).copy(), f[B * A:2 * B * A].reshape(B, A).copy(), f[2 * B * A:].reshape(B, 2).copy()
    i32 = h[o + nf:].view(np.int32)
    return counts, tau, rho, mean, i32[:2 * B].reshape(B, 2).copy(), i32[2 * B:3 * B].copy()


def rank_correlation(x, y, device=None) -> Tuple[np.ndarray, np.ndarray]:
    """Kendall's tau-b and Spearman's rho of every row of x with every row of y. x: (B, n) or (n,); y: (A, n) or (n,); on the GPU
    or the host; compared as float32. Returns (tau, rho), float64 arrays (B, A) (a 1-D argument is one row); NaN where a row is
    constant or holds a non-finite value. One launch sequence, one read-back. Extension, parity unpinned (no reference code)."""
    tx, ty = _rows(x, "x"), _rows(y, "y")
    B, n = int(tx.shape[0]), int(tx.shape[1])
    A = int(ty.shape[0])
    if int(ty.shape[1]) != n:
        raise ValueError(f"x has {n} elements per row, y has {int(ty.shape[1])}")
    if n > MAX_N or A > MAX_ANNOTATORS or B > MAX_BATCH:
        raise ValueError(f"need n <= {MAX_N}, at most {MAX_ANNOTATORS} rows of y and at most {MAX_BATCH} rows of x, got n = {n}, "
                         f"{A} and {B}")
    dev = _device(device, tx, ty)
    lib = _lib.load()
    xd = tx.to(device=dev, dtype=torch.float32).contiguous()
    yd = ty.to(device=dev, dtype=torch.float32).contiguous()
    host = _launch(lib, xd, n, 1, yd, n, 1, B, A, n).cpu()
    _, tau, rho, _, _, _ = _unpack(host, B, A)
    return tau, rho


class RankEvaluator:
    """`RankEvaluator(user_scores, skip_frames, frames="sampled" | "full")`: one video's annotator scores `user_scores`
    (A, full_n_frames) — `load_mat_file`'s `user_anno`, or the matrix of the tsv's rows that `groundtruth.get_annotations` takes —
    kept on the device as float32. `ev(predictions)` takes the model's N = ceil(full_n_frames / skip_frames) importances
    (`VideoTrainer.eval_video`'s second result) and returns a `RankCorrelation`.

    frames="sampled": prediction i against every annotator's score of frame i skip_frames, the frames `get_annotations` labels.
    frames="full": prediction j // skip_frames against the score of every frame j — `expand_array` (utils.py:396-410) applied
    to the predictions; full_n_frames <= 65536.
    Extension, parity unpinned (no reference code)."""

    def __init__(self, user_scores, skip_frames: int, frames: str = "sampled", device=None):
        if frames not in ("sampled", "full"):
            raise ValueError(f'frames must be "sampled" or "full", got {frames!r}')
        t = _tensor(user_scores)
        if t.dim() != 2 or t.shape[0] < 1 or t.shape[1] < 1:
            raise ValueError(f"user_scores must be (n_annotators, full_n_frames), got {tuple(t.shape)}")
        self.skip = int(skip_frames)
        if self.skip < 1:
            raise ValueError("skip_frames must be positive")
        self.frames = frames
        self.n_annotators, self.full_n = int(t.shape[0]), int(t.shape[1])
        self.n_sampled = -(-self.full_n // self.skip)
        self.n = self.n_sampled if frames == "sampled" else self.full_n
        if self.n_annotators > MAX_ANNOTATORS or self.n > MAX_N:
            raise ValueError(f"need at most {MAX_ANNOTATORS} annotators and {MAX_N} compared frames, got {self.n_annotators} and {self.n}")
        self.device = _device(device, t)
        self.lib = _lib.load()
        self.scores = t.to(device=self.device, dtype=torch.float32).contiguous()
        self._x_repeat, self._y_stride = (1, self.skip) if frames == "sampled" else (self.skip, 1)

    @classmethod
    def from_annotations(cls, user_anno, skip_frames: int, frames: str = "sampled", device=None):
        """from the array `SummaryEvaluator.from_annotations` takes: `load_mat_file`'s (A, full_n_frames) `user_anno`, utils.py:102"""
        return cls(user_anno, skip_frames, frames, device)

    def _predictions(self, predictions, batched: bool) -> torch.Tensor:
        t = _prediction_rows(_tensor(predictions), self.n_sampled, batched, f"{self.full_n} frames sampled every {self.skip}")
        return t.to(device=self.device, dtype=torch.float32).contiguous()

    def launch(self, predictions) -> torch.Tensor:
        """The kernels on the current stream for (N,), (N, 1) or (B, N) predictions; returns the packed device buffer (uint8;
        `unpack` reads a host copy of it) WITHOUT synchronising."""
        t = _tensor(predictions)
        single = t.dim() == 1 or (t.dim() == 2 and tuple(t.shape) == (self.n_sampled, 1))
        return self._run(self._predictions(t, batched=not single))

    def _run(self, pred: torch.Tensor) -> torch.Tensor:
        return _launch(self.lib, pred, self.n_sampled, self._x_repeat, self.scores, self.full_n, self._y_stride, int(pred.shape[0]),
                       self.n_annotators, self.n)

    def unpack(self, host: torch.Tensor, B: int) -> RankCorrelation:
        """a host copy of `launch`'s buffer for B prediction rows -> `RankCorrelation` with a leading B"""
        counts, tau, rho, mean, n_valid, status = _unpack(host, B, self.n_annotators)
        return RankCorrelation(mean[:, 0].copy(), mean[:, 1].copy(), tau, rho, n_valid, counts, status != 0)

    def batch(self, predictions) -> RankCorrelation:
        """B prediction vectors of this video, (B, N): every field with a leading B. One read-back."""
        pred = self._predictions(predictions, batched=True)
        return self.unpack(self._run(pred).cpu(), int(pred.shape[0]))   # the one synchronising read-back

    def __call__(self, predictions) -> RankCorrelation:
        """One prediction vector, (N, 1) or (N,). One read-back. Non-finite predictions give NaN and nonfinite=True, not an error."""
        pred = self._predictions(predictions, batched=False)
        r = self.unpack(self._run(pred).cpu(), 1)                       # the one synchronising read-back
        return RankCorrelation(float(r.kendall[0]), float(r.spearman[0]), r.kendall_per_annotator[0], r.spearman_per_annotator[0],
                               r.n_valid[0], r.counts[0], bool(r.nonfinite[0]))

    def human(self) -> HumanConsistency:
        """Leave-one-out consistency of the annotators: the score rows themselves go in as x (every skip_frames-th frame of them
        for frames="sampled"), the diagonal is dropped, and every annotator's defined correlations with the others are averaged in
        float64 on the host, in annotator order; the overall figure is the mean of those per-annotator means. The same kernel as
        `ev(...)`, one read-back."""
        A = self.n_annotators
        if self.frames == "sampled":
            x = self.scores[:, ::self.skip].contiguous()
            ldx = self.n_sampled
        else:
            x, ldx = self.scores, self.full_n
        host = _launch(self.lib, x, ldx, 1, self.scores, self.full_n, self._y_stride, A, A, self.n).cpu()
        _, tau, rho, _, _, _ = _unpack(host, A, A)
        out = []
        n_valid = np.zeros((A, 2), dtype=np.int32)
        for k, m in enumerate((tau, rho)):
            np.fill_diagonal(m, np.nan)
            per = np.full(A, np.nan)
            for a in range(A):
                s, c = 0.0, 0
                for o in range(A):
                    if m[a, o] == m[a, o]:
                        s += float(m[a, o])
                        c += 1
                n_valid[a, k] = c
                if c:
                    per[a] = s / c
            defined = [float(v) for v in per if v == v]
            total = 0.0
            for v in defined:
                total += v
            out.append((total / len(defined) if defined else float("nan"), per, m))
        return HumanConsistency(out[0][0], out[1][0], out[0][1], out[1][1], out[0][2], out[1][2], n_valid)
