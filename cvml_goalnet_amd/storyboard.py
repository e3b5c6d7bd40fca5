"""The static summary of a video (csrc/storyboard.hip, include/goalnet_storyboard.h): one keyframe per chosen clip,
its thumbnail, and the thumbnails on a contact sheet. Everything it needs is in device memory after `VideoSummarizer` has run — the
importances, the change points, the knapsack's flags and the source video, BGR or NV12 — and everything it makes stays there.

    sb = VideoSummarizer(model, cps)(video, storyboard=dict(size=(160, 90), cols=4)).storyboard
    sb.frame_index, sb.clip, sb.score, sb.thumbnails, sb.sheet

EXTENSION, PARITY WITH cv2 UNPINNED: the reference only makes the skim. The keyframe of a clip is its sampled frame with the highest
importance (ties to the first; a clip between two samples gives its middle frame); the thumbnails come from an exact box filter in
integers, `out = (sum wy wx p + H0 W0 // 2) // (H0 W0)` with the weights the overlaps of output and source cells. Both are DEFINED in
include/goalnet_storyboard.h; parity with `cv2.resize(..., INTER_AREA)` is unpinned.
No CPU fallback: without the library / a GPU the calls raise.
"""
from __future__ import annotations

from dataclasses import dataclass
from typing import Optional

import numpy as np
import torch

from . import _lib, nv12
from ._lib import GoalnetError, check
from .ops import _s

OPTIONS = ("size", "cols", "gap", "background", "max_keyframes", "clips")
DEFAULT_SIZE = (160, 90)


@dataclass
class Storyboard:
    frame_index: torch.Tensor      # (K,) int32 on the device: the source frame of every keyframe, in clip order
    clip: torch.Tensor             # (K,) int32: the clip (row of change_points) it stands for
    score: torch.Tensor            # (K,) float32: the importance it was chosen by (-inf for a NaN prediction)
    thumbnails: torch.Tensor       # (K, th, tw, 3) uint8 BGR
    sheet: Optional[torch.Tensor] = None   # (Hs, Ws, 3) uint8 BGR: the thumbnails `cols` to a row, or None without `cols`


def _device(device):
    if not torch.cuda.is_available():
        raise GoalnetError("the storyboard is made on the GPU (torch.cuda.is_available() is False); there is no CPU fallback")
    return torch.device(device if device is not None else "cuda:0")


def sheet_shape(k: int, size, cols: int, gap: int):
    """(Hs, Ws) of a sheet of k thumbnails of size = (tw, th), `cols` to a row with `gap` pixels around and between them"""
    tw, th = int(size[0]), int(size[1])
    rows = -(-int(k) // int(cols))
    return gap + rows * (th + gap), gap + cols * (tw + gap)


def _check_size(size):
    try:
        tw, th = int(size[0]), int(size[1])
        ok = len(size) == 2
    except (TypeError, ValueError, IndexError):
        ok = False
    if not ok or not (1 <= tw <= _lib.STORYBOARD_MAX_DIM and 1 <= th <= _lib.STORYBOARD_MAX_DIM):
        raise ValueError(f"size must be (width, height) with both in 1 .. {_lib.STORYBOARD_MAX_DIM}, got {size!r}")
    return tw, th


def _check_sheet(cols, gap, background):
    if cols is not None and int(cols) < 1:
        raise ValueError("cols must be >= 1 (or None for no sheet)")
    if int(gap) < 0:
        raise ValueError("gap must be >= 0")
    try:
        bg = tuple(int(x) for x in background)
    except (TypeError, ValueError):
        bg = ()
    if len(bg) != 3 or min(bg) < 0 or max(bg) > 255:
        raise ValueError(f"background must be three values (B, G, R) in 0 .. 255, got {background!r}")
    return None if cols is None else int(cols), int(gap), bg


def _check_max(max_keyframes):
    if max_keyframes is not None and int(max_keyframes) < 1:
        raise ValueError("max_keyframes must be >= 1 (or None for no limit)")
    return 0 if max_keyframes is None else int(max_keyframes)


def check_options(options) -> dict:
    """the `storyboard=` dict of `VideoSummarizer.__call__` with defaults filled in; ValueError for a bad option"""
    if not isinstance(options, dict):
        raise ValueError("storyboard must be a dict of options: " + ", ".join(OPTIONS))
    unknown = sorted(set(options) - set(OPTIONS))
    if unknown:
        raise ValueError(f"unknown storyboard option(s) {unknown}: one of {', '.join(OPTIONS)}")
    o = dict(size=DEFAULT_SIZE, cols=None, gap=4, background=(0, 0, 0), max_keyframes=None, clips="selected")
    o.update(options)
    o["size"] = _check_size(o["size"])
    o["cols"], o["gap"], o["background"] = _check_sheet(o["cols"], o["gap"], o["background"])
    _check_max(o["max_keyframes"])
    if o["clips"] not in ("selected", "all"):
        raise ValueError(f"clips must be 'selected' or 'all', got {o['clips']!r}")
    return o


def _change_points(change_points) -> np.ndarray:
    cps = np.asarray(change_points)
    if cps.ndim != 2 or cps.shape[1] != 2 or not 1 <= cps.shape[0] <= _lib.STORYBOARD_MAX_CLIPS:
        raise ValueError(f"change_points must be [n_clips][2] with 1 <= n_clips <= {_lib.STORYBOARD_MAX_CLIPS}")
    return np.ascontiguousarray(cps.astype(np.int32))


def clip_lengths(change_points, full_n: int) -> np.ndarray:
    """the number of frames of every clip's slice [a:b), clamped to the video as the clip gather clamps it (csrc/clip_scan.h)"""
    cps = np.asarray(change_points).astype(np.int64)
    a, b = cps[:, 0], cps[:, 1]
    a = np.where(a < 0, np.maximum(a + full_n, 0), a)
    b = np.where(b < 0, np.maximum(b + full_n, 0), b)
    return np.maximum(np.minimum(b, full_n) - np.minimum(a, full_n), 0)


def _predictions(predictions) -> torch.Tensor:
    t = predictions if torch.is_tensor(predictions) else torch.as_tensor(np.asarray(predictions))
    if t.dim() == 2 and t.shape[-1] == 1:
        t = t[:, 0]
    if t.dim() != 1 or t.numel() < 1:
        raise ValueError("predictions must be (n_sampled,) or (n_sampled, 1) with at least one entry")
    return t


def _launch_keyframes(pred, skip, full_n, cps_dev, flags_dev, n_clips, max_keyframes, capacity, count):
    """one launch, no synchronisation: (frame_index, clip, score) of `capacity` entries, *count on the device"""
    dev = pred.device
    frame_index = torch.empty(capacity, dtype=torch.int32, device=dev)
    clip = torch.empty(capacity, dtype=torch.int32, device=dev)
    score = torch.empty(capacity, dtype=torch.float32, device=dev)
    with torch.cuda.device(dev):
        check(_lib.load().goalnet_storyboard_keyframes(pred.data_ptr(), pred.numel(), int(skip), int(full_n), cps_dev.data_ptr(),
                                                       0 if flags_dev is None else flags_dev.data_ptr(), int(n_clips), int(max_keyframes),
                                                       frame_index.data_ptr(), clip.data_ptr(), score.data_ptr(), int(capacity), count.data_ptr(),
                                                       _s()), "storyboard_keyframes")
    return frame_index, clip, score


def select_keyframes(predictions, change_points, skip_frames: int, full_n_frames: int, selected=None, max_keyframes=None, device=None):
    """One keyframe per chosen clip: (frame_index, clip, score), device tensors of K entries in clip order.
    predictions: (n_sampled,) or (n_sampled, 1), the importances of frames 0, skip_frames, 2 skip_frames, ...; change_points:
    [n_clips][2], taken as the clip gather takes them (end-exclusive, clamped to the video). selected: a list of clip indices
    (`VideoSummary.selected`), a device int32 flag tensor [n_clips] (nonzero = chosen), or None for every clip — a table of contents
    of the whole video. max_keyframes: keep only the highest-scoring ones (ties to the earlier clip), still in clip order.
    With a list or None the host knows K and nothing is read back; with a device flag tensor K is read back (one synchronisation)."""
    cps = _change_points(change_points)
    n_clips = int(cps.shape[0])
    skip, full_n = int(skip_frames), int(full_n_frames)
    if skip < 1 or full_n < 1:
        raise ValueError("skip_frames and full_n_frames must be positive")
    limit = _check_max(max_keyframes)
    pred = _predictions(predictions)
    flags_host = None
    if selected is not None and not torch.is_tensor(selected):
        idx = np.asarray(list(selected), dtype=np.int64).reshape(-1)
        if idx.size and (idx.min() < 0 or idx.max() >= n_clips):
            raise ValueError(f"selected holds a clip index outside 0 .. {n_clips - 1}")
        flags_host = np.zeros(n_clips, dtype=np.int32)
        flags_host[idx] = 1
    elif selected is not None and (selected.dtype != torch.int32 or selected.numel() != n_clips):
        raise ValueError("a flag tensor must be int32 with one entry per clip")
    dev = _device(device)
    pred = pred.detach().to(device=dev, dtype=torch.float32).contiguous()
    cps_dev = torch.from_numpy(cps).to(dev)
    count = torch.zeros(1, dtype=torch.int32, device=dev)
    if torch.is_tensor(selected):
        out = _launch_keyframes(pred, skip, full_n, cps_dev, selected.to(dev).contiguous(), n_clips, limit, n_clips, count)
        k = int(count.item())
    else:
        lengths = clip_lengths(cps, full_n)
        k = int(np.count_nonzero(lengths if flags_host is None else lengths * flags_host))
        k = min(k, limit) if limit else k
        if k < 1:
            raise ValueError("no keyframe: no chosen clip holds a frame of the video")
        out = _launch_keyframes(pred, skip, full_n, cps_dev, None if flags_host is None else torch.from_numpy(flags_host).to(dev), n_clips, limit,
                                k, count)
    if k < 1:
        raise ValueError("no keyframe: no chosen clip holds a frame of the video")
    return tuple(t[:k] for t in out)


def render_thumbnails(full_frames, frame_index, size=DEFAULT_SIZE, cols=None, gap: int = 4, background=(0, 0, 0), pixel_format: str = "bgr",
                      frame_size=None, uv_row=None, colorspace="bt601"):
    """The frames `frame_index` (a device int32 tensor, or a list) of the video scaled to size = (tw, th) with the box filter:
    (thumbnails (K, th, tw, 3) uint8, sheet). With cols the thumbnails are also laid out `cols` to a row on a sheet (Hs, Ws, 3) with
    `gap` pixels of `background` (B, G, R) around and between them; without, sheet is None. full_frames: (full_n, H0, W0, 3) uint8, or
    with pixel_format="nv12" (full_n, rows, pitch) with frame_size, uv_row and colorspace as in cvml_goalnet_amd/nv12.py; on the GPU
    (read in place, only the named frames) or on the host (uploaded). No synchronisation."""
    tw, th = _check_size(size)
    cols, gap, bg = _check_sheet(cols, gap, background)
    if pixel_format not in nv12.PIXEL_FORMATS:
        raise ValueError(f"unknown pixel_format {pixel_format!r}: one of {', '.join(nv12.PIXEL_FORMATS)}")
    t = full_frames if torch.is_tensor(full_frames) else torch.from_numpy(np.ascontiguousarray(full_frames))
    if pixel_format == "nv12":
        t = nv12._frames(t)
        h0, w0, pitch, uv_offset, frame_pitch = nv12.nv12_layout(t.shape, frame_size, uv_row)
        table = nv12._table(colorspace)
    else:
        if t.dtype != torch.uint8 or t.dim() != 4 or t.shape[3] != 3:
            raise ValueError("full_frames must be uint8 (full_n, H0, W0, 3)")
        h0, w0 = int(t.shape[1]), int(t.shape[2])
    if t.shape[0] < 1 or not (1 <= h0 <= _lib.STORYBOARD_MAX_DIM and 1 <= w0 <= _lib.STORYBOARD_MAX_DIM):
        raise ValueError(f"need at least one frame of 1 .. {_lib.STORYBOARD_MAX_DIM} pixels a side")
    idx = frame_index if torch.is_tensor(frame_index) else torch.as_tensor(np.asarray(frame_index).reshape(-1).astype(np.int32))
    if idx.dtype != torch.int32 or idx.dim() != 1 or idx.numel() < 1:
        raise ValueError("frame_index must be int32 (K,) with at least one entry")
    dev = _device(t.device if t.is_cuda else (idx.device if idx.is_cuda else None))
    t = t.to(dev).contiguous()
    idx = idx.to(dev).contiguous()
    k = int(idx.numel())
    thumbs = torch.empty(k, th, tw, 3, dtype=torch.uint8, device=dev)
    sheet = None if cols is None else torch.empty(*sheet_shape(k, (tw, th), cols, gap), 3, dtype=torch.uint8, device=dev)
    tail = (idx.data_ptr(), k, th, tw, thumbs.data_ptr(), 0 if sheet is None else sheet.data_ptr(), cols or 1, gap, bg[0], bg[1], bg[2], _s())
    lib = _lib.load()
    with torch.cuda.device(dev):
        if pixel_format == "nv12":
            check(lib.goalnet_storyboard_render_nv12(t.data_ptr(), t.shape[0], h0, w0, pitch, uv_offset, frame_pitch, nv12._cptr(table), *tail),
                  "storyboard_render_nv12")
        else:
            check(lib.goalnet_storyboard_render(t.data_ptr(), t.shape[0], h0, w0, *tail), "storyboard_render")
    return thumbs, sheet


def storyboard(predictions, change_points, skip_frames: int, full_frames, selected=None, max_keyframes=None, size=DEFAULT_SIZE, cols=None,
               gap: int = 4, background=(0, 0, 0), pixel_format: str = "bgr", frame_size=None, uv_row=None, colorspace="bt601",
               device=None) -> Storyboard:
    """`select_keyframes` and `render_thumbnails` in one call; full_n_frames is the video's length."""
    _check_size(size)
    _check_sheet(cols, gap, background)
    _check_max(max_keyframes)
    shape = full_frames.shape
    if len(shape) < 1 or shape[0] < 1:
        raise ValueError("full_frames holds no frame")
    if device is None and torch.is_tensor(full_frames) and full_frames.is_cuda:
        device = full_frames.device
    frame_index, clip, score = select_keyframes(predictions, change_points, skip_frames, int(shape[0]), selected, max_keyframes, device)
    if not (torch.is_tensor(full_frames) and full_frames.is_cuda):
        full_frames = (full_frames if torch.is_tensor(full_frames) else torch.from_numpy(np.ascontiguousarray(full_frames))).to(frame_index.device)
    thumbs, sheet = render_thumbnails(full_frames, frame_index, size, cols, gap, background, pixel_format, frame_size, uv_row, colorspace)
    return Storyboard(frame_index, clip, score, thumbs, sheet)


def from_summary(options: dict, predictions, cps_host, cps_dev, flags_dev, selected, skip: int, frames, layout=None) -> Storyboard:
    """The storyboard of one `VideoSummarizer` call, behind its read-back and with none of its own: predictions (N, 1), the change
    points on the host and on the device, the knapsack's flags on the device and as the list the host already holds, the resident
    video. options: what `check_options` returned. layout: (frame_size, uv_row, colorspace) of an NV12 video."""
    full_n = int(frames.shape[0])
    n_clips = int(cps_dev.numel() // 2)
    if n_clips > _lib.STORYBOARD_MAX_CLIPS:
        raise ValueError(f"a storyboard takes at most {_lib.STORYBOARD_MAX_CLIPS} clips, the video has {n_clips}")
    lengths = clip_lengths(cps_host, full_n)
    every = options["clips"] == "all"
    k = int(np.count_nonzero(lengths)) if every else int(np.count_nonzero(lengths[np.asarray(selected, dtype=np.int64)]))
    limit = _check_max(options["max_keyframes"])
    k = min(k, limit) if limit else k
    if k < 1:
        raise ValueError("no keyframe: no chosen clip holds a frame of the video")
    pred = predictions.view(-1)
    count = torch.empty(1, dtype=torch.int32, device=pred.device)
    frame_index, clip, score = _launch_keyframes(pred, skip, full_n, cps_dev, None if every else flags_dev, n_clips, limit, k, count)
    kw = {} if layout is None else dict(pixel_format="nv12", frame_size=layout[0], uv_row=layout[1], colorspace=layout[2])
    thumbs, sheet = render_thumbnails(frames, frame_index, options["size"], options["cols"], options["gap"], options["background"], **kw)
    return Storyboard(frame_index, clip, score, thumbs, sheet)
