#!/usr/bin/env python3
"""Generate tests/golden/groundtruth_*.npz from the REFERENCE's own functions (build container only).

What `get_dataloaders` computes per video before the first training step:

  * the annotator summaries, utils.py:102-118: one `postprocess` per annotator on that annotator's per-frame scores. As in
    make_golden_postproc.py, `postprocess` itself opens HDF5 files and cannot be called; its pure-Python building blocks can
    (`expand_array`, `get_clip_information`, `knapsack`), imported with the recipe of SURVEY.md Appendix B (empty module
    objects for the absent I/O libraries; no reference source is edited or copied), and are chained per annotator exactly as
    utils.py:608-641 chains them. The glue statements are restated from the cited lines: round -> int8 (utils.py:611),
    capacity = int(0.15 n) (utils.py:629) and the end-inclusive mask loop (utils.py:638-641). The importances enter as
    `torch.tensor(annotator_gd[:, None])` of a float64 array (utils.py:111: the .mat file holds doubles).
  * the labels, `get_annotations` (utils.py:370-394), called as it is on a tsv written to a temporary directory from the same
    score matrix (`video_id \\t category \\t comma separated scores`, one row per annotator, as TVSum's ydata-tvsum50-anno.tsv).

Scores are TVSum-like: integers 1..5, piecewise constant over 2-second shots (60 frames); the fixtures store them as uint8
(the tests hand them on as float64, the dtype the reference sees). Before anything is written,
oracle/postproc_ref.postprocess must agree with the reference on every annotator.

Usage: python tests/golden/make_golden_groundtruth.py [case ...]
"""
from __future__ import annotations

import os
import sys
import tempfile

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
sys.path.insert(0, HERE)

from make_golden_postproc import import_reference  # noqa: E402
from oracle import postproc_ref  # noqa: E402

SHOT = 60                                                               # 2 seconds at 30 frames per second


def make_case(seed, full_n, skip, n_clips, n_users=20, flat_user=None, min_user=None):
    rng = np.random.default_rng(seed)
    n_shots = (full_n + SHOT - 1) // SHOT
    scores = np.repeat(rng.integers(1, 6, size=(n_users, n_shots)), SHOT, axis=1)[:, :full_n].astype(np.float64)
    if flat_user is not None:
        scores[flat_user, :] = 3.0                                     # every clip's value = 3 x its weight: ties in the DP
    if min_user is not None:
        scores[min_user, :] = 1.0
    cuts = np.sort(rng.choice(np.arange(1, full_n), size=n_clips - 1, replace=False)) if n_clips > 1 else np.array([], dtype=int)
    cps = np.stack([np.concatenate([[0], cuts]), np.concatenate([cuts - 1, [full_n - 1]])], axis=1).astype(np.int32)
    return dict(scores=scores, change_points=cps, skip=skip, full_n=full_n)


CASES = {
    "groundtruth_typical_n4500": dict(seed=21, full_n=4500, skip=15, n_clips=41),
    "groundtruth_long_n20000": dict(seed=22, full_n=20000, skip=15, n_clips=200),
    "groundtruth_ties_n1200": dict(seed=23, full_n=1200, skip=15, n_clips=25, flat_user=2, min_user=5),
    "groundtruth_tiny_n5": dict(seed=24, full_n=5, skip=2, n_clips=2, n_users=3),
}


def reference_summary(utils, annotator_gd, cps, skip, full_n):
    batch = torch.tensor(annotator_gd[:, None])                        # utils.py:111
    batch = batch[:, 0]                                                # utils.py:608-610
    imp = torch.round(batch).type(torch.int8).tolist()                 # utils.py:611
    expanded = utils.expand_array(arr=imp, expansion_rate=skip, length=full_n)
    vals, lens, _ = utils.get_clip_information(clip_intervals=cps, importances=expanded)
    cap = int(0.15 * full_n)                                           # utils.py:629
    sel = utils.knapsack(values=vals, weights=lens, capacity=cap)
    mask = np.zeros(shape=(full_n,), dtype=np.uint8)                   # utils.py:638-641
    for ci in sel:
        for f in range(cps[ci][0], cps[ci][1] + 1):
            mask[f] = 1
    return sel, mask


def reference_labels(utils, scores, skip):
    with tempfile.TemporaryDirectory() as d:
        fp = os.path.join(d, "anno.tsv")
        with open(fp, "w") as f:
            for other in scores[:2]:                                   # rows of another video: skipped by utils.py:376
                f.write("other_video\tXX\t" + ",".join(str(int(x)) for x in other) + "\n")
            for row in scores:
                f.write("the_video\tXX\t" + ",".join(str(int(x)) for x in row) + "\n")
        trimmed, full = utils.get_annotations(annotation_fp=fp, video_id="the_video", skip_frames=skip)
    return np.asarray(trimmed), np.asarray(full)


def main():
    utils = import_reference()
    names = sys.argv[1:] or list(CASES)
    for name in names:
        c = make_case(**CASES[name])
        cps, skip, full_n = c["change_points"], c["skip"], c["full_n"]
        flags = np.zeros((c["scores"].shape[0], cps.shape[0]), dtype=np.uint8)
        masks = np.zeros((c["scores"].shape[0], full_n), dtype=np.uint8)
        for a, annotator_gd in enumerate(c["scores"]):
            sel, mask = reference_summary(utils, annotator_gd, cps, skip, full_n)
            sel2, mask2 = postproc_ref.postprocess(annotator_gd[:, None], cps, skip, full_n)    # the restatement must agree
            assert sel2 == sel and np.array_equal(mask2, mask), (name, a)
            flags[a, sel] = 1
            masks[a] = mask
        trimmed, full = reference_labels(utils, c["scores"], skip)
        assert trimmed.dtype == np.float32 and full.dtype == np.float32, (trimmed.dtype, full.dtype)
        assert full.shape == (full_n,) and trimmed.shape == ((full_n + skip - 1) // skip,)
        np.savez_compressed(os.path.join(HERE, name + ".npz"), scores=c["scores"].astype(np.uint8), change_points=cps, skip=np.array([skip]),
                            full_n=np.array([full_n]), selected_flags=flags, masks=masks, labels_trimmed=trimmed, labels_full=full)
        print(f"{name}: annotators={masks.shape[0]} clips={cps.shape[0]} frames per summary {masks.sum(axis=1).tolist()[:6]}... "
              f"labels {np.unique(full).tolist()} size {os.path.getsize(os.path.join(HERE, name + '.npz'))} B")


if __name__ == "__main__":
    main()
