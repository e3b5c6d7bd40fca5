#!/usr/bin/env python3
"""Time of `goalnet_storyboard_render` (csrc/storyboard.hip) against its traffic floor: 24 keyframes of a 1080 x 1920
video resident on the device scaled to 320 x 180 thumbnails,

  (a) from packed BGR            floor: 24 * 1080 * 1920 * 3   bytes read once
  (b) from NV12 (pitch 1920)     floor: 24 * 1080 * 1920 * 1.5 bytes read once
  (c), (d) a device-to-device copy of exactly those bytes (a contiguous block of the same video), for the same window

The video has --frames frames (240: 1.49 GB of BGR, 0.75 GB of NV12) and every launch of a window takes another set of 24 frames
(set s = frames s, s + 10, s + 20, ...; the copies take block s of 24 frames), so that no launch finds its frames in the 256 MiB
Infinity Cache. Device events around --steps launches, the four sides alternating after warm-up, median of --reps windows. The
thumbnails of (a) and (b) are held against each other's source (the NV12 video converted by goalnet_nv12_to_bgr) before anything is
timed. Nothing here is asserted by the test suite.

    python scripts/bench_storyboard.py [--out FILE.json] [--frames 240] [--steps 20] [--reps 7]
"""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

H0, W0, TH, TW, K = 1080, 1920, 180, 320, 24


def _timed(torch, fn, steps):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for s in range(steps):
        fn(s)
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / steps


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out")
    ap.add_argument("--frames", type=int, default=240)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--reps", type=int, default=7)
    args = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("bench_storyboard.py measures on the GPU: none found")
    from cvml_goalnet_amd import _lib, nv12
    from cvml_goalnet_amd._lib import check
    from cvml_goalnet_amd.storyboard import render_thumbnails
    dev = torch.device("cuda:0")
    sets = args.frames // K
    assert sets >= 1, "need at least 24 frames"
    g = torch.Generator(device=dev).manual_seed(21)
    yuv = torch.randint(0, 256, (args.frames, H0 * 3 // 2, W0), dtype=torch.uint8, device=dev, generator=g)
    bgr = nv12.nv12_to_bgr(yuv, (H0, W0))
    index = [torch.arange(s, s + sets * K, sets, dtype=torch.int32, device=dev) for s in range(sets)]
    assert all(i.numel() == K and int(i.max()) < args.frames for i in index)
    copy_bgr, copy_yuv = torch.empty_like(bgr[:K]), torch.empty_like(yuv[:K])
    a = render_thumbnails(bgr, index[0], size=(TW, TH))[0]
    b = render_thumbnails(yuv, index[0], size=(TW, TH), pixel_format="nv12", frame_size=(H0, W0))[0]
    assert tuple(a.shape) == (K, TH, TW, 3) and torch.equal(a, b), "the BGR and the NV12 path disagree"
    # the timed calls go through the raw C ABI into one preallocated output: a launch costs the host a few microseconds, not the
    # validation and the allocation of the Python wrapper
    lib = _lib.load()
    stream = torch.cuda.current_stream().cuda_stream
    coeffs = nv12.nv12_coefficients("bt601")                           # host memory: stays alive as long as `table` is used
    table = nv12._cptr(coeffs)
    out = torch.empty_like(a)

    def render_bgr(s):
        check(lib.goalnet_storyboard_render(bgr.data_ptr(), args.frames, H0, W0, index[s % sets].data_ptr(), K, TH, TW, out.data_ptr(), 0, 1, 0,
                                            0, 0, 0, stream))

    def render_nv12(s):
        check(lib.goalnet_storyboard_render_nv12(yuv.data_ptr(), args.frames, H0, W0, W0, H0 * W0, H0 * W0 * 3 // 2, table, index[s % sets].data_ptr(),
                                                 K, TH, TW, out.data_ptr(), 0, 1, 0, 0, 0, 0, stream))

    for fn in (render_bgr, render_nv12):
        out.zero_()
        fn(0)
        assert torch.equal(out, a), "the raw call and the Python call disagree"
    sides = {
        "a_render_bgr": render_bgr,
        "b_render_nv12": render_nv12,
        "c_copy_bgr_bytes": lambda s: copy_bgr.copy_(bgr[(s % sets) * K:(s % sets + 1) * K]),
        "d_copy_nv12_bytes": lambda s: copy_yuv.copy_(yuv[(s % sets) * K:(s % sets + 1) * K]),
    }
    for fn in sides.values():
        _timed(torch, fn, args.warmup)
    times = {k: [] for k in sides}
    for _ in range(args.reps):
        for k, fn in sides.items():
            times[k].append(_timed(torch, fn, args.steps))
    med = {k: statistics.median(v) for k, v in times.items()}
    read = {"bgr": K * H0 * W0 * 3, "nv12": K * H0 * W0 * 3 // 2}
    res = {"metric": "goalnet_storyboard_render against a device-to-device copy of the bytes it must read: ms per call (device events), "
                     "median of reps",
           "shape": f"{K} keyframes of {H0} x {W0} -> {TH} x {TW}; video of {args.frames} frames, {sets} rotating sets",
           "device": torch.cuda.get_device_name(0), "steps": args.steps, "warmup": args.warmup, "reps": args.reps,
           "bytes_read": read, "ms": {k: round(v, 4) for k, v in med.items()}, "all_ms": {k: [round(t, 4) for t in v] for k, v in times.items()},
           "read_TBps": {"a_render_bgr": round(read["bgr"] / med["a_render_bgr"] / 1e9, 3), "b_render_nv12": round(read["nv12"] / med["b_render_nv12"] / 1e9, 3),
                         "c_copy_bgr_bytes": round(read["bgr"] / med["c_copy_bgr_bytes"] / 1e9, 3),
                         "d_copy_nv12_bytes": round(read["nv12"] / med["d_copy_nv12_bytes"] / 1e9, 3)},
           "ratio_a_over_c": round(med["a_render_bgr"] / med["c_copy_bgr_bytes"], 3),
           "ratio_b_over_d": round(med["b_render_nv12"] / med["d_copy_nv12_bytes"], 3)}
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(json.dumps(res) + "\n")
    print(json.dumps(res))


if __name__ == "__main__":
    main()
