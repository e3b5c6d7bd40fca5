"""The oracle of the NV12 tests: the conversion of include/goalnet_nv12.h restated with numpy in int64, then clamped. No library
code is used here; the colour table is an argument, as in the C ABI."""
import numpy as np


def pixel(y, u, v, c):
    """(B, G, R) of one (Y, U, V) triple; Python integers, so nothing can overflow"""
    y_off, cy, cub, cug, cvg, cvr, shift = (int(x) for x in c[:7])
    yy = max(0, int(y) - y_off) * cy
    r0 = 1 << (shift - 1)
    u, v = int(u) - 128, int(v) - 128
    sat = lambda x: min(max(x, 0), 255)                                # noqa: E731
    return sat((yy + cub * u + r0) >> shift), sat((yy + cug * u + cvg * v + r0) >> shift), sat((yy + cvr * v + r0) >> shift)


def to_bgr(frames, frame_size, uv_row=None, coeffs=None):
    """frames (n, rows, pitch) uint8 -> (n, H0, W0, 3) uint8 BGR: nearest chroma, int64 arithmetic, floor shift, clamp"""
    f = np.asarray(frames)
    h0, w0 = frame_size
    uv_row = h0 if uv_row is None else uv_row
    y_off, cy, cub, cug, cvg, cvr, shift = (int(x) for x in coeffs[:7])
    Y = f[:, :h0, :w0].astype(np.int64)
    uv = f[:, uv_row:uv_row + h0 // 2, :w0].astype(np.int64)
    U = np.repeat(np.repeat(uv[:, :, 0::2], 2, axis=1), 2, axis=2) - 128
    V = np.repeat(np.repeat(uv[:, :, 1::2], 2, axis=1), 2, axis=2) - 128
    yy = np.maximum(0, Y - y_off) * cy
    r0 = 1 << (shift - 1)
    B = (yy + cub * U + r0) >> shift                                    # numpy's >> on int64 is arithmetic: floor
    G = (yy + cug * U + cvg * V + r0) >> shift
    R = (yy + cvr * V + r0) >> shift
    return np.clip(np.stack([B, G, R], axis=-1), 0, 255).astype(np.uint8)


def minmax(bgr):
    """(n, 2) int32: min and max of every frame over all three channels"""
    flat = bgr.reshape(bgr.shape[0], -1)
    return np.stack([flat.min(axis=1), flat.max(axis=1)], axis=1).astype(np.int32)
