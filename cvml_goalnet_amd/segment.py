"""Temporal segmentation on the GPU: the change points of a video from the per-frame descriptors the model already computes.

EXTENSION, PARITY UNPINNED (no reference code). The reference never segments a video: it reads the change points of the 50 TVSum
videos from `eccv16_dataset_tvsum_google_pool5.h5` (`utils.py:424-431`, `624-625`), where they were made with Kernel Temporal
Segmentation (KTS: Potapov, Douze, Harchaoui, Schmid, "Category-specific video summarization", ECCV 2014). `TemporalSegmenter` is
that published algorithm with the linear kernel, run on the device (csrc/kts.hip) on the `(N, 512 | 640)` input of the fusion MLP
(`AVM.last_features`), so that `VideoSummarizer` can summarise a video that is not in the dataset. The oracle is the project's
own float64 restatement (tests/kts_ref.py); the algorithm is written out in DESIGN.md §4.8.

No CPU fallback: without the library / a GPU the call raises.
"""
from __future__ import annotations

from dataclasses import dataclass
from typing import Optional

import numpy as np
import torch

from . import _lib
from ._lib import GoalnetError, check
from .ops import _s

MAX_N, MAX_D = 8192, 4096


@dataclass
class Segmentation:
    change_points: np.ndarray      # (n_clips, 2) int32, frame units, end inclusive: what SummaryEvaluator takes
    samples: np.ndarray            # (n_change_points,) int32: the change points in sample units, ascending
    cost: np.ndarray               # (max_change_points + 1,) float64: I[m][n], the within-segment scatter of the best m-change-point
                                   # segmentation (+inf where lmin / lmax allow none)
    objective: np.ndarray          # (max_change_points + 1,) float64: cost[m] / n + penalty(m)
    n_change_points: int           # the chosen m = argmin objective (the smallest on a tie)


class TemporalSegmenter:
    """`TemporalSegmenter(max_change_points=None, lmin=1, lmax=None, vmax=1.0, normalize=True).segment(descriptors, full_n_frames,
    skip_frames)` -> `Segmentation`. Extension, parity unpinned (no reference code).

    max_change_points: the largest number of change points considered. The default is min(n - 1, ceil(full_n_frames / 60)): at most
    one change point per two seconds of 30 fps video. That default is THIS PROJECT'S CHOICE; nothing in the reference fixes it.
    lmin / lmax: the shortest / longest segment in samples (lmax=None: n). vmax: the scale of the penalty
    (vmax m / (2n)) (ln(n / m) + 1) that selects the number of change points. normalize: divide every descriptor by its L2 norm."""

    def __init__(self, max_change_points: Optional[int] = None, lmin: int = 1, lmax: Optional[int] = None, vmax: float = 1.0,
                 normalize: bool = True):
        if max_change_points is not None and int(max_change_points) < 0:
            raise ValueError("max_change_points must be >= 0")
        if int(lmin) < 1 or (lmax is not None and int(lmax) < int(lmin)):
            raise ValueError("need 1 <= lmin <= lmax")
        self.max_change_points = None if max_change_points is None else int(max_change_points)
        self.lmin = int(lmin)
        self.lmax = None if lmax is None else int(lmax)
        self.vmax = float(vmax)
        self.normalize = bool(normalize)

    def default_max_change_points(self, n: int, full_n_frames: int) -> int:
        return min(n - 1, -(-int(full_n_frames) // 60))

    def segment(self, descriptors, full_n_frames: int, skip_frames: int, device=None) -> Segmentation:
        """descriptors: (n, d) float32, one row per sampled frame (n = ceil(full_n_frames / skip_frames)), on the GPU or the host.
        The kernels go on the current stream; ONE read-back fetches every result and is the only synchronisation. Raises GoalnetError
        when lmin / lmax leave no feasible segmentation."""
        t = descriptors if torch.is_tensor(descriptors) else torch.from_numpy(np.ascontiguousarray(descriptors))
        if t.dim() != 2 or not 1 <= t.shape[0] <= MAX_N or not 1 <= t.shape[1] <= MAX_D:
            raise ValueError(f"descriptors must be (n, d) with 1 <= n <= {MAX_N} and 1 <= d <= {MAX_D}, got {tuple(t.shape)}")
        n, d = int(t.shape[0]), int(t.shape[1])
        full_n, skip = int(full_n_frames), int(skip_frames)
        if skip < 1 or not (n - 1) * skip < full_n <= n * skip:
            raise ValueError(f"{n} descriptors do not belong to {full_n} frames sampled every {skip}: need n = ceil(full_n_frames / skip_frames)")
        max_cp = self.default_max_change_points(n, full_n) if self.max_change_points is None else self.max_change_points
        if max_cp > n - 1:
            raise ValueError(f"max_change_points = {max_cp} needs more than {n} samples")
        lmax = n if self.lmax is None else self.lmax
        if not torch.cuda.is_available():
            raise GoalnetError("temporal segmentation runs on the GPU (torch.cuda.is_available() is False); there is no CPU fallback")
        lib = _lib.load()
        dev = torch.device(device) if device is not None else (t.device if t.is_cuda else torch.device("cuda:0"))
        x = t.detach().to(device=dev, dtype=torch.float32).contiguous()
        rows = max_cp + 1
        # one buffer, one read-back: [n_clips | status | change_points [rows][2] | samples [max(max_cp, 1)] | pad to 8 B] int32, then
        # [cost [rows] | objective [rows]] float64
        n_i32 = 2 + 2 * rows + max(max_cp, 1)
        n_i32 += n_i32 & 1
        packed = torch.empty(n_i32 * 4 + 2 * rows * 8, dtype=torch.uint8, device=dev)
        ints = packed[:n_i32 * 4].view(torch.int32)
        f64 = packed[n_i32 * 4:].view(torch.float64)
        ws_bytes = lib.goalnet_kts_ws_bytes(n, d, max_cp)
        ws = torch.empty(ws_bytes // 8, dtype=torch.float64, device=dev)
        with torch.cuda.device(dev):
            check(lib.goalnet_kts(x.data_ptr(), n, d, int(self.normalize), max_cp, self.lmin, lmax, self.vmax, skip, full_n,
                                  ints[2:].data_ptr(), ints[0:].data_ptr(), ints[2 + 2 * rows:].data_ptr(), f64.data_ptr(),
                                  f64[rows:].data_ptr(), ints[1:].data_ptr(), ws.data_ptr(), ws_bytes, _s()), "kts")
        host = packed.cpu()                                             # the one synchronising read-back
        hi = host[:n_i32 * 4].view(torch.int32).numpy()
        hf = host[n_i32 * 4:].view(torch.float64).numpy()
        n_clips, status = int(hi[0]), int(hi[1])
        if status != 0:
            raise GoalnetError(f"no feasible segmentation: lmin = {self.lmin}, lmax = {lmax} allow no split of {n} samples into at most "
                               f"{max_cp + 1} segments")
        m = n_clips - 1
        return Segmentation(hi[2:2 + 2 * n_clips].reshape(n_clips, 2).copy(), hi[2 + 2 * rows:2 + 2 * rows + m].copy(),
                            hf[:rows].copy(), hf[rows:2 * rows].copy(), m)
