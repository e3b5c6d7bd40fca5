"""The oracle of the storyboard tests, written from the formulas of include/goalnet_storyboard.h with Python integers and numpy
int64; no library code is used here. NV12 pixels come from tests/nv12_ref.py."""
import math

import numpy as np


# ---- keyframes --------------------------------------------------------------------------------------------------------------------
def clip_range(a, b, full_n):
    """[a, b) as a Python slice of a video of full_n frames takes it"""
    a, b = int(a), int(b)
    if a < 0:
        a = max(a + full_n, 0)
    if b < 0:
        b = max(b + full_n, 0)
    return min(a, full_n), min(b, full_n)


def key(p):
    p = float(p)
    return -math.inf if math.isnan(p) else p


def keyframes(pred, skip, full_n, change_points, flags=None, max_keyframes=0):
    """(frame_index int32 [K], clip int32 [K], score float32 [K]); flags None = every clip; max_keyframes <= 0 = no limit"""
    pred = np.asarray(pred, dtype=np.float32).reshape(-1)
    n_sampled = len(pred)
    at = np.arange(n_sampled, dtype=np.int64) * skip                    # the frame of every sample
    found = []                                                          # (frame, clip, score)
    for c, (a, b) in enumerate(np.asarray(change_points).tolist()):
        if flags is not None and int(flags[c]) == 0:
            continue
        a, b = clip_range(a, b, full_n)
        if b <= a:
            continue
        cand = np.nonzero((a <= at) & (at < b))[0].tolist()              # the samples j with a <= j skip < b, ascending
        if cand:
            best = cand[0]
            for j in cand[1:]:
                if key(pred[j]) > key(pred[best]):                      # strictly: ties stay with the smallest j
                    best = j
            found.append((best * skip, c, key(pred[best])))
        else:
            frame = a + (b - a) // 2
            found.append((frame, c, key(pred[min(frame // skip, n_sampled - 1)])))
    if max_keyframes > 0 and len(found) > max_keyframes:
        order = sorted(range(len(found)), key=lambda e: (-found[e][2], found[e][1]))      # highest score first, ties to the lower clip
        keep = sorted(order[:max_keyframes])
        found = [found[e] for e in keep]
    return (np.array([f[0] for f in found], dtype=np.int32), np.array([f[1] for f in found], dtype=np.int32),
            np.array([f[2] for f in found], dtype=np.float32))


# ---- the box filter ---------------------------------------------------------------------------------------------------------------
def weights(n_src, n_dst):
    """w[i][r] = max(0, min((i + 1) n_src, (r + 1) n_dst) - max(i n_src, r n_dst)): the overlap of output cell i and source cell r on
    a line of n_src * n_dst units. int64 (n_dst, n_src)."""
    i = np.arange(n_dst, dtype=np.int64)[:, None]
    r = np.arange(n_src, dtype=np.int64)[None, :]
    return np.maximum(0, np.minimum((i + 1) * n_src, (r + 1) * n_dst) - np.maximum(i * n_src, r * n_dst))


def box_resize(img, th, tw):
    """img (H0, W0, C) uint8 -> (th, tw, C) uint8: (sum_r sum_c wy wx p + H0 W0 // 2) // (H0 W0), int64 throughout
    (255 * 16384 * 16384 < 2^63)"""
    img = np.asarray(img)
    h0, w0 = img.shape[:2]
    wy, wx = weights(h0, th), weights(w0, tw)
    rows = np.einsum("jc,rck->rjk", wx, img.astype(np.int64))            # sum_c wx p, per source row
    s = np.einsum("ir,rjk->ijk", wy, rows)
    area = h0 * w0
    return ((s + area // 2) // area).astype(np.uint8)


def thumbnails(frames_bgr, frame_index, th, tw):
    """frames_bgr (full_n, H0, W0, 3) uint8 -> (K, th, tw, 3)"""
    cache = {}
    out = []
    for f in np.asarray(frame_index).tolist():
        if f not in cache:
            cache[f] = box_resize(frames_bgr[f], th, tw)
        out.append(cache[f])
    return np.stack(out)


# ---- the sheet --------------------------------------------------------------------------------------------------------------------
def sheet(thumbs, cols, gap, background):
    k, th, tw = thumbs.shape[:3]
    rows = -(-k // cols)
    out = np.empty((gap + rows * (th + gap), gap + cols * (tw + gap), 3), dtype=np.uint8)
    out[...] = np.asarray(background, dtype=np.uint8)
    for i in range(k):
        y, x = gap + (i // cols) * (th + gap), gap + (i % cols) * (tw + gap)
        out[y:y + th, x:x + tw] = thumbs[i]
    return out
