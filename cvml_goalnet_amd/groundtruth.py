"""A video's ground truth on the GPU: what the reference's `get_dataloaders` computes before the first training step.

    annotator_summaries   utils.py:102-118   one `postprocess` per annotator (20 pure-Python knapsacks per video) ->
                                             `gd_summarized_video_frame_indices`, one batched call here
    get_annotations       utils.py:370-394   per-frame mean of the annotators, every skip_frames-th, np.round -> labels

Reading the files stays the caller's I/O: `user_anno` is `load_mat_file`'s (A, full_n) array, `scores` the (A, full_n) matrix
of the tsv's rows, `change_points` the KTS intervals of the HDF5 file. `SummaryEvaluator.from_annotations` (postprocess.py)
is `annotator_summaries` whose masks stay on the device as the evaluator's `gd`.

No CPU fallback: without the library / a GPU these functions raise.
"""
from __future__ import annotations

from typing import Tuple

import numpy as np
import torch

from . import _lib
from ._lib import check
from .ops import _s
from .postprocess import SummaryEvaluator, _dev

F32 = torch.float32


def annotator_summaries(user_anno, change_points, skip_frames: int, full_n_frames: int, device=None) -> np.ndarray:
    """utils.py:103-118: row a = the summary mask `postprocess` returns for annotator a's per-frame scores. (A, full_n_frames) uint8."""
    ev = SummaryEvaluator(change_points, full_n_frames, skip_frames, None, device)
    return ev.postprocess_batch(user_anno)[1]


def get_annotations(scores, skip_frames: int, device=None) -> Tuple[torch.Tensor, torch.Tensor]:
    """utils.py:370-394 on the (A, full_n) score matrix: (labels of frames 0, skip, 2 skip, ..., labels of every frame), float32
    on the device — np.round (half to even) of np.mean over the annotators in float32, in numpy's summation order for a 1-D
    array (the reference reduces one column at a time)."""
    dev = _dev(device)
    lib = _lib.load()
    t = scores if torch.is_tensor(scores) else torch.from_numpy(np.ascontiguousarray(np.asarray(scores, dtype=np.float32)))
    if t.dim() != 2 or t.shape[0] < 1 or t.shape[1] < 1:
        raise ValueError("scores must be (n_annotators, full_n_frames)")
    skip = int(skip_frames)
    if skip < 1:
        raise ValueError("skip_frames must be positive")
    t = t.detach().to(device=dev, dtype=F32).contiguous()
    n_annot, full_n = int(t.shape[0]), int(t.shape[1])
    full = torch.empty(full_n, dtype=F32, device=dev)
    trimmed = torch.empty((full_n + skip - 1) // skip, dtype=F32, device=dev)
    with torch.cuda.device(dev):
        check(lib.goalnet_mean_annotations(t.data_ptr(), n_annot, full_n, skip, trimmed.data_ptr(), full.data_ptr(), _s()), "mean_annotations")
    return trimmed, full
