/*
 * goalnet_storyboard.h — the eleventh public header of libgoalnet_hip.so: the static summary of a video. One keyframe per chosen clip,
 * its thumbnail, and the thumbnails laid out on a contact sheet (EXTENSION: the reference only makes the dynamic summary, the skim. The
 * choice of keyframes and the box filter below are DEFINED here; parity with cv2.resize(..., INTER_AREA) is UNPINNED).
 *
 * Additions next to goalnet_hip.h, which stays frozen at GOALNET_ABI_VERSION 7; the older headers do not gain these names.
 * Conventions are those of goalnet_nv12.h: 0 = OK, negative = argument error (GOALNET_E_*), positive = hipError_t of the failed
 * launch, goalnet_last_error() gives the text; raw device pointers and explicit dims; `stream` is a hipStream_t passed as void*; no
 * allocation, no synchronisation, every argument check runs before any launch.
 *
 * Keyframes. Clip c covers the frames [a, b) = change_points[c][0 .. 1] taken as goalnet_gather_clips takes them: end-exclusive,
 * negative values count from the end, both clamped to 0 .. full_n; so a keyframe is always a frame the skim contains. A clip takes
 * part when flags[c] != 0 (flags == NULL: every clip) and b > a. With key(j) = pred[j], NaN counted as -infinity:
 *     candidates   the sampled frames j with a <= j * skip < b and j < n_sampled
 *     winner       the candidate with the largest key, ties to the smallest j:   frame = j * skip, score = key(j)
 *     no candidate frame = a + (b - a) / 2, score = key(min(frame / skip, n_sampled - 1))      (integer divisions)
 * When max_keyframes > 0 is smaller than the number found, the max_keyframes entries with the highest score stay (ties to the lower
 * clip index). The entries are written compact and in clip order.
 *
 * Thumbnails: an exact box (area) filter in integers. For output row i and source row r, output column j and source column c,
 *     wy(i, r) = max(0, min((i + 1) H0, (r + 1) th) - max(i H0, r th))       wx(j, c) likewise with W0, tw
 *     out[i][j][ch] = (sum_r sum_c wy wx p[r][c][ch] + (H0 W0) / 2) / (H0 W0)                     (integer division)
 * p is the source byte; for NV12 frames the B, G, R value goalnet_nv12.h defines for that pixel (each pixel is converted, then
 * averaged). The same formula enlarges (th > H0, tw > W0); th = H0 and tw = W0 is the identity.
 *
 * Sheet: rows = ceil(K / cols); Hs = gap + rows (th + gap); Ws = gap + cols (tw + gap); thumbnail k lies at row k / cols and column
 * k % cols, its top left corner at (gap + (k / cols) (th + gap), gap + (k % cols) (tw + gap)); every other byte of the sheet, unused
 * trailing cells included, holds the background.
 */
#ifndef GOALNET_STORYBOARD_H
#define GOALNET_STORYBOARD_H

#include "goalnet_nv12.h"

#ifdef __cplusplus
extern "C" {
#endif

#define GOALNET_STORYBOARD_MAX_CLIPS 4096
#define GOALNET_STORYBOARD_MAX_DIM 16384      /* H0, W0, th, tw: every product of two of them fits an int32 */

/* pred: float32 [n_sampled]; change_points: int32 [n_clips][2]; flags: int32 [n_clips] (what goalnet_postprocess writes as `selected`)
 * or NULL for every clip. frame_index, clip: int32 [capacity]; score: float32 [capacity]; *count: int32, the number of keyframes
 * found (after max_keyframes; <= 0: no limit). Nothing is written behind `capacity` entries: *count > capacity says that the
 * arrays were too short. One launch of one block.
 * GOALNET_E_NULL: a null pointer other than flags. GOALNET_E_SHAPE: n_sampled < 1, skip < 1, full_n < 1, capacity < 1, n_clips < 1
 * or n_clips > GOALNET_STORYBOARD_MAX_CLIPS. */
int goalnet_storyboard_keyframes(const float* pred, int n_sampled, int skip, int full_n, const int32_t* change_points,
                                 const int32_t* flags, int n_clips, int max_keyframes, int32_t* frame_index, int32_t* clip, float* score,
                                 int capacity, int32_t* count, void* stream);

/* frames: packed BGR uint8 [full_n][H0][W0][3] at any alignment; frame_index: DEVICE int32 [K], the frames to render (an index
 * outside 0 .. full_n - 1 is clamped into the video; repeated and unordered entries are fine). thumbs: [K][th][tw][3] or NULL;
 * sheet: [Hs][Ws][3] or NULL (cols and gap are read only with a sheet); bg_b, bg_g, bg_r: the sheet's background.
 * Only the named frames are read. One launch, two with a sheet (the background first).
 * GOALNET_E_NULL: frames or frame_index null, or both destinations null. GOALNET_E_SHAPE: full_n < 1, K < 1, any of H0, W0, th, tw
 * outside 1 .. GOALNET_STORYBOARD_MAX_DIM, with a sheet cols < 1, gap < 0 or Hs or Ws past 2^31 - 1. GOALNET_E_VALUE: a background
 * value outside 0 .. 255. */
int goalnet_storyboard_render(const uint8_t* frames, int full_n, int H0, int W0, const int32_t* frame_index, int K, int th, int tw,
                              uint8_t* thumbs, uint8_t* sheet, int cols, int gap, int bg_b, int bg_g, int bg_r, void* stream);

/* The same from NV12 frames: layout arguments, HOST colour table, layout rules, table rules and read contract of goalnet_nv12.h (no
 * padding byte influences a result; 16-byte loads where frames, pitch, uv_offset and frame_pitch are multiples of 16).
 * Refusals: those of goalnet_storyboard_render and the layout (GOALNET_E_SHAPE) and table (GOALNET_E_VALUE) rules; coeffs null:
 * GOALNET_E_NULL. */
int goalnet_storyboard_render_nv12(const uint8_t* frames, int full_n, int H0, int W0, int64_t pitch, int64_t uv_offset,
                                   int64_t frame_pitch, const int32_t* coeffs, const int32_t* frame_index, int K, int th, int tw,
                                   uint8_t* thumbs, uint8_t* sheet, int cols, int gap, int bg_b, int bg_g, int bg_r, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* GOALNET_STORYBOARD_H */
