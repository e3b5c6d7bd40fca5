"""NV12 frames, as a hardware decoder leaves them in device memory, as an input of the inference path (csrc/nv12.hip,
include/goalnet_nv12.h): a full-resolution Y plane followed by a half-resolution plane of interleaved U, V pairs,
1.5 bytes per pixel, usually with a row pitch wider than the picture and a padded plane height. `frames_to_tensor(...,
pixel_format="nv12")` and `VideoSummarizer(...)(..., pixel_format="nv12")` convert in registers where pixels are consumed — the
sampled frames for the model, the selected clips for the summary — and never make a BGR copy of the video; `nv12_to_bgr` is the
plain conversion.

EXTENSION, PARITY WITH cv2 UNPINNED: the reference decodes through cv2 / ffmpeg into packed BGR and OpenCV is not installed here.
The arithmetic is DEFINED in include/goalnet_nv12.h: nearest chroma and one int32 fixed-point table
`{y_off, cy, cub, cug, cvg, cvr, shift, 0}`, which is an argument of the C ABI; the presets below supply it.

Layout: a uint8 tensor or array (full_n, rows, pitch); `frame_size = (H0, W0)`, both even; the chroma plane starts at row `uv_row`
(default H0); rows >= uv_row + H0 / 2. The compact layout is (full_n, H0 * 3 / 2, W0).
No CPU fallback: without the library / a GPU the calls raise.
"""
from __future__ import annotations

import ctypes
from fractions import Fraction

import numpy as np
import torch

from . import _lib
from ._lib import GoalnetError, check
from .ops import _s

FIXED_SHIFT = 20
# (Kr, Kb) of the luma equation Y = Kr R + (1 - Kr - Kb) G + Kb B
_LUMA = {"bt601": (Fraction(299, 1000), Fraction(114, 1000)), "bt709": (Fraction(2126, 10000), Fraction(722, 10000))}
# the 3-decimal BT.601 limited-range constants 1.164, 2.018, -0.391, -0.813, 1.596 in 20-bit fixed point
_BT601 = (16, 1220542, 2116026, -409993, -852492, 1673527, FIXED_SHIFT, 0)
COLORSPACES = ("bt601", "bt709", "bt601-full", "bt709-full")
PIXEL_FORMATS = ("bgr", "nv12")


def _fixed(x: Fraction) -> int:
    """round(x * 2**20), half away from zero"""
    n = abs(x) * (1 << FIXED_SHIFT)
    r = int(n + Fraction(1, 2))
    return r if x >= 0 else -r


def nv12_coefficients(colorspace: str = "bt601") -> np.ndarray:
    """The int32[8] table {y_off, cy, cub, cug, cvg, cvr, shift, 0} of include/goalnet_nv12.h for a named colour space. "bt601" is
    the usual 3-decimal limited-range table; "bt709", "bt601-full" and "bt709-full" are round(x * 2**20) of the exact matrix of
    (Kr, Kb): luma gain 255/219 and chroma gain 255/224 with y_off = 16 for limited range, 1 and 1 with y_off = 0 for full range."""
    if colorspace == "bt601":
        return np.array(_BT601, dtype=np.int32)
    if not isinstance(colorspace, str) or colorspace not in COLORSPACES:
        raise ValueError(f"unknown colorspace {colorspace!r}: one of {', '.join(COLORSPACES)}")
    full = colorspace.endswith("-full")
    kr, kb = _LUMA[colorspace[:5]]
    kg = 1 - kr - kb
    sy, sc = (Fraction(1), Fraction(1)) if full else (Fraction(255, 219), Fraction(255, 224))
    return np.array([0 if full else 16, _fixed(sy), _fixed(2 * (1 - kb) * sc), _fixed(-2 * (1 - kb) * kb / kg * sc),
                     _fixed(-2 * (1 - kr) * kr / kg * sc), _fixed(2 * (1 - kr) * sc), FIXED_SHIFT, 0], dtype=np.int32)


def _table(colorspace) -> np.ndarray:
    """a preset's name, or the caller's own table of 8 integers (the C side checks its values)"""
    if isinstance(colorspace, str):
        return nv12_coefficients(colorspace)
    c = np.asarray(colorspace)
    if c.shape != (8,) or not np.issubdtype(c.dtype, np.integer):
        raise ValueError("colorspace must be a preset's name or an integer table of 8 entries")
    return np.ascontiguousarray(c, dtype=np.int32)


def _cptr(c: np.ndarray):
    return c.ctypes.data_as(ctypes.POINTER(ctypes.c_int32))


def nv12_layout(shape, frame_size, uv_row=None):
    """(H0, W0, pitch, uv_offset, frame_pitch) of frames shaped (full_n, rows, pitch); ValueError for a layout the C ABI refuses"""
    if frame_size is None:
        raise ValueError("NV12 frames need frame_size = (H0, W0): the tensor's rows and pitch may be padded")
    if len(shape) != 3:
        raise ValueError(f"NV12 frames must be (full_n, rows, pitch), got {tuple(shape)}")
    h0, w0 = int(frame_size[0]), int(frame_size[1])
    rows, pitch = int(shape[1]), int(shape[2])
    if h0 < 2 or w0 < 2 or h0 % 2 or w0 % 2:
        raise ValueError(f"frame_size = ({h0}, {w0}): H0 and W0 must be even and positive")
    uv = h0 if uv_row is None else int(uv_row)
    if pitch < w0:
        raise ValueError(f"the frames' pitch {pitch} is narrower than W0 = {w0}")
    if uv < h0:
        raise ValueError(f"uv_row = {uv} lies inside the Y plane of {h0} rows")
    if rows < uv + h0 // 2:
        raise ValueError(f"the frames have {rows} rows, the chroma plane needs uv_row + H0 / 2 = {uv + h0 // 2}")
    return h0, w0, pitch, uv * pitch, rows * pitch


def _frames(frames):
    t = frames if torch.is_tensor(frames) else torch.from_numpy(np.ascontiguousarray(frames))
    if t.dtype != torch.uint8 or t.dim() != 3:
        raise ValueError("NV12 frames must be uint8 (full_n, rows, pitch)")
    return t


def _device(device):
    if not torch.cuda.is_available():
        raise GoalnetError("the NV12 conversion runs on the GPU (torch.cuda.is_available() is False); there is no CPU fallback")
    return torch.device(device if device is not None else "cuda:0")


def nv12_to_bgr(frames, frame_size, uv_row=None, colorspace="bt601", device=None) -> torch.Tensor:
    """frames: uint8 (full_n, rows, pitch) NV12, numpy or torch, on the host or the device. Returns the (full_n, H0, W0, 3) uint8
    BGR frames on the GPU: what `cv2.VideoCapture` would hand to the rest of the package. No synchronisation."""
    t = _frames(frames)
    h0, w0, pitch, uv_offset, frame_pitch = nv12_layout(t.shape, frame_size, uv_row)
    if t.shape[0] < 1:
        raise ValueError("no frames")
    c = _table(colorspace)
    dev = _device(device)
    t = t.to(dev).contiguous()
    out = torch.empty(t.shape[0], h0, w0, 3, dtype=torch.uint8, device=dev)
    with torch.cuda.device(dev):
        check(_lib.load().goalnet_nv12_to_bgr(t.data_ptr(), t.shape[0], h0, w0, pitch, uv_offset, frame_pitch, _cptr(c), out.data_ptr(), _s()),
              "nv12_to_bgr")
    return out


def preprocess_strided(frames, stride, size, frame_size, uv_row, colorspace, minmax=None) -> torch.Tensor:
    """`preprocess.frames_to_tensor(..., pixel_format="nv12")` on a resident video: frames 0, stride, 2 stride, ... of the contiguous
    uint8 GPU tensor (n_total, rows, pitch) -> (ceil(n_total / stride), 3, height, width) float32, size = (width, height).
    minmax: optional int32 (n, 2) scratch, left holding every sampled frame's min and max over its converted B, G, R values."""
    h0, w0, pitch, uv_offset, frame_pitch = nv12_layout(frames.shape, frame_size, uv_row)
    if not (frames.is_cuda and frames.dtype == torch.uint8 and frames.is_contiguous()):
        raise GoalnetError("nv12 preprocess_strided: frames must be a contiguous uint8 GPU tensor")
    n_total, stride = int(frames.shape[0]), int(stride)
    if n_total < 1 or stride < 1:
        raise ValueError("nv12 preprocess_strided: stride and the number of frames must be >= 1")
    n = (n_total + stride - 1) // stride
    c = _table(colorspace)
    w, h = int(size[0]), int(size[1])
    dev = frames.device
    out = torch.empty(n, 3, h, w, dtype=torch.float32, device=dev)
    if minmax is None:
        minmax = torch.empty(n, 2, dtype=torch.int32, device=dev)
    elif not (minmax.is_cuda and minmax.dtype == torch.int32 and minmax.numel() == 2 * n and minmax.is_contiguous()):
        raise GoalnetError("nv12 preprocess_strided: minmax must be a contiguous int32 GPU tensor (n, 2)")
    with torch.cuda.device(dev):
        check(_lib.load().goalnet_nv12_preprocess_strided(frames.data_ptr(), n_total, stride, h0, w0, pitch, uv_offset, frame_pitch, _cptr(c),
                                                          out.data_ptr(), h, w, minmax.data_ptr(), _s()), "nv12_preprocess_strided")
    return out


def gather_clips_bgr(frames, frame_size, uv_row, colorspace, change_points, selected, out, capacity, src_index, count, status):
    """`ops.gather_clips` for NV12 frames (full_n, rows, pitch) with the conversion on the way: out (>= capacity, H0, W0, 3) uint8.
    count: int64[1] tensor (or a device address), status: int32[1]; all tensors on the frames' device, no synchronisation."""
    h0, w0, pitch, uv_offset, frame_pitch = nv12_layout(frames.shape, frame_size, uv_row)
    n_clips = selected.numel()
    ok = (frames.is_cuda and frames.dtype == torch.uint8 and frames.is_contiguous() and frames.shape[0] >= 1
          and out.is_cuda and out.dtype == torch.uint8 and out.is_contiguous() and tuple(out.shape[1:]) == (h0, w0, 3)
          and change_points.is_cuda and change_points.dtype == torch.int32 and change_points.numel() == 2 * n_clips and change_points.is_contiguous()
          and selected.is_cuda and selected.dtype == torch.int32 and selected.is_contiguous()
          and 0 <= capacity <= out.shape[0] and src_index.is_cuda and src_index.dtype == torch.int32 and src_index.numel() >= capacity
          and src_index.is_contiguous() and status.is_cuda and status.dtype == torch.int32 and status.numel() == 1)
    if not ok:
        raise GoalnetError("nv12 gather_clips_bgr: frames uint8 (full_n, rows, pitch), out uint8 (>= capacity, H0, W0, 3), change_points int32 "
                           "(n_clips, 2), selected int32 (n_clips), src_index int32 (>= capacity), status int32[1], contiguous on the GPU")
    if torch.is_tensor(count):
        if not (count.is_cuda and count.dtype == torch.int64 and count.numel() == 1):
            raise GoalnetError("nv12 gather_clips_bgr: count must be an int64[1] GPU tensor")
        count = count.data_ptr()
    c = _table(colorspace)
    lib = _lib.load()
    nbytes = lib.goalnet_nv12_gather_clips_bgr_ws_bytes(n_clips)
    ws = torch.empty(max(nbytes // 8, 1), dtype=torch.int64, device=frames.device)
    with torch.cuda.device(frames.device):
        check(lib.goalnet_nv12_gather_clips_bgr(frames.data_ptr(), frames.shape[0], h0, w0, pitch, uv_offset, frame_pitch, _cptr(c),
                                                change_points.data_ptr(), selected.data_ptr(), n_clips, out.data_ptr(), int(capacity),
                                                src_index.data_ptr(), count, status.data_ptr(), ws.data_ptr(), nbytes, _s()),
              "nv12_gather_clips_bgr")
    return out
