"""GPU: NV12 frames in, BGR or NV12 out (csrc/nv12.hip, cvml_goalnet_amd/nv12.py). Integer arithmetic, byte copies
and frame_resize.h's one float sequence: every comparison here is exact. The conversion is held against the numpy restatement of
its definition (tests/nv12_ref.py), the pre-processing against the BGR entry point on the converted frames and against
oracle/preproc_ref on the oracle's BGR, the converting gather against goalnet_gather_clips on the converted video, and the
summariser against itself on the converted video. Frames are drawn with a seeded generator per case; padding bytes are random
unless a test fills them."""
import ctypes
import functools

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import nv12_ref as R  # noqa: E402
from cvml_goalnet_amd import AVM, TemporalSegmenter, VideoSummarizer, _lib, nv12, ops, synth  # noqa: E402
from cvml_goalnet_amd.nv12 import nv12_coefficients, nv12_to_bgr  # noqa: E402
from cvml_goalnet_amd.preprocess import frames_to_tensor  # noqa: E402
from oracle import preproc_ref  # noqa: E402

# (H0, W0, pitch, uv_row): 2 x 2 and 4 x 6 (one partial block); rows not 16-byte aligned (byte loads); aligned rows (16-byte loads);
# padded pitch and padded plane height; a multiple of the block; several min / max thread blocks per frame
GEOMETRIES = [(2, 2, 2, 2), (4, 6, 6, 4), (18, 34, 34, 18), (36, 64, 64, 36), (36, 64, 80, 40), (90, 160, 160, 96), (270, 480, 512, 272)]
PADDED = [(36, 64, 80, 40), (270, 480, 512, 272)]
STRIDES = [(1, 1), (7, 3), (31, 15), (150, 60)]                        # (n_total, stride)
CONTENTS = ("uniform", "low", "constant", "saturating")
SIZES = [(40, 40), (52, 41)]


def _rows(geom):
    h0, _, _, uv_row = geom
    return uv_row + h0 // 2 + (2 if geom in PADDED else 0)             # the padded geometries also have rows behind the chroma plane


def _fill(frame, geom, content, rng):
    """the picture bytes of one frame (rows, pitch); everything else keeps what it held"""
    h0, w0, _, uv_row = geom
    y, uv = frame[:h0, :w0], frame[uv_row:uv_row + h0 // 2, :w0]
    if content == "uniform":
        y[...] = rng.integers(0, 256, size=y.shape)
        uv[...] = rng.integers(0, 256, size=uv.shape)
    elif content == "low":                                             # min / max of the converted values are not 0 / 255
        y[...] = rng.integers(60, 181, size=y.shape)
        uv[...] = rng.integers(100, 151, size=uv.shape)
    elif content == "constant":                                        # mn == mx: an all-zero tensor
        y[...] = rng.integers(30, 220)                                  # grey: B = G = R, so the min and max over all three channels meet
        uv[...] = 128
    else:                                                              # B and R saturate both ways, Y below 16 and at 255
        y[...] = rng.choice(np.array([0, 3, 15, 16, 17, 254, 255], dtype=np.uint8), size=y.shape)
        uv[...] = rng.choice(np.array([0, 1, 128, 254, 255], dtype=np.uint8), size=uv.shape)


@functools.lru_cache(maxsize=4)
def _video(geom, n, stride=1, seed=0):
    """n frames (n, rows, pitch) uint8; frame j * stride has content class j % 4, so every class is among the sampled frames"""
    rng = np.random.default_rng(1000 * seed + 7 * n + geom[1] + geom[2])
    f = rng.integers(0, 256, size=(n, _rows(geom), geom[2]), dtype=np.uint8)      # random padding
    for i in range(n):
        _fill(f[i], geom, CONTENTS[(i // stride + i % stride) % 4], rng)
    return f


def _ref_bgr(f, geom, colorspace="bt601"):
    return R.to_bgr(f, geom[:2], geom[3], nv12_coefficients(colorspace))


def _with_padding(f, geom, value):
    """a copy with every padding byte set to `value`: columns >= W0 of both planes, rows between and behind the planes"""
    h0, w0, _, uv_row = geom
    g = np.full_like(f, value)
    g[:, :h0, :w0] = f[:, :h0, :w0]
    g[:, uv_row:uv_row + h0 // 2, :w0] = f[:, uv_row:uv_row + h0 // 2, :w0]
    return g


# ---- 1. the conversion ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("colorspace", ["bt601", "bt709-full"])
@pytest.mark.parametrize("geom", GEOMETRIES)
def test_nv12_to_bgr_equals_the_definition(geom, colorspace):
    rng = np.random.default_rng(geom[0] * 31 + geom[2])
    f = rng.integers(0, 256, size=(2 * len(CONTENTS), _rows(geom), geom[2]), dtype=np.uint8)
    for i in range(f.shape[0]):                                         # every content class twice
        _fill(f[i], geom, CONTENTS[i % 4], rng)
    want = _ref_bgr(f, geom, colorspace)
    assert len(np.unique(want[2].reshape(-1, 3), axis=0)) == 1 and want[1].max() < 255                     # the constant and the low-contrast frame
    dev = torch.from_numpy(f).cuda()
    got = nv12_to_bgr(dev, geom[:2], geom[3], colorspace)
    assert got.is_cuda and got.dtype == torch.uint8 and tuple(got.shape) == want.shape
    assert np.array_equal(got.cpu().numpy(), want)
    assert np.array_equal(nv12_to_bgr(f, geom[:2], geom[3], colorspace).cpu().numpy(), want)               # host frames
    # frames whose base is not 16-byte aligned (a view 5 bytes into a larger allocation): the byte-load path, and for the same
    # reason an output the caller cannot see; the result is the same
    flat = torch.zeros(f.size + 5, dtype=torch.uint8, device="cuda")
    flat[5:] = dev.view(-1)
    odd = flat[5:].view(f.shape)
    assert odd.data_ptr() % 16 == 5
    assert np.array_equal(nv12_to_bgr(odd, geom[:2], geom[3], colorspace).cpu().numpy(), want)


def test_a_custom_table_at_the_shift_limits():
    geom = (18, 34, 34, 18)
    f = _video(geom, 4)
    for table in ([16, 298, 516, -100, -208, 409, 8, 0], [0, 4000000, 3000000, -700000, -1500000, 2500000, 24, 0]):
        want = R.to_bgr(f, geom[:2], geom[3], table)
        assert np.array_equal(nv12_to_bgr(f, geom[:2], geom[3], table).cpu().numpy(), want)


# ---- 2. padding is inert --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("geom", PADDED)
def test_padding_is_inert(geom):
    n_total, stride = 7, 3
    f = _video(geom, n_total, stride)
    lo, hi = _with_padding(f, geom, 0), _with_padding(f, geom, 255)
    assert (lo != hi).any() and not np.array_equal(lo, f)
    results = []
    for g in (lo, hi, f):
        dev = torch.from_numpy(g).cuda()
        bgr = nv12_to_bgr(dev, geom[:2], geom[3])
        n = -(-n_total // stride)
        minmax = torch.full((n, 2), -1, dtype=torch.int32, device="cuda")
        pre = nv12.preprocess_strided(dev, stride, (40, 40), geom[:2], geom[3], "bt601", minmax)
        results.append((bgr.cpu().numpy(), minmax.cpu().numpy(), pre.cpu().numpy()))
    want_bgr = _ref_bgr(f, geom)
    for bgr, minmax, pre in results:
        assert np.array_equal(bgr, results[0][0]) and np.array_equal(minmax, results[0][1]) and np.array_equal(pre, results[0][2])
        assert np.array_equal(bgr, want_bgr)
        assert np.array_equal(minmax, R.minmax(want_bgr[::stride]))
    # with a low-contrast picture a padding byte of 255 would raise the maximum if it were read
    dark = np.full_like(f[:2], 255)
    for i in range(2):
        _fill(dark[i], geom, "low", np.random.default_rng(i))
    minmax = torch.empty((2, 2), dtype=torch.int32, device="cuda")
    nv12.preprocess_strided(torch.from_numpy(dark).cuda(), 1, (40, 40), geom[:2], geom[3], "bt601", minmax)
    want = R.minmax(_ref_bgr(dark, geom))
    assert np.array_equal(minmax.cpu().numpy(), want) and want.max() < 255


# ---- 3. pre-processing ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n_total,stride", STRIDES)
@pytest.mark.parametrize("geom", GEOMETRIES)
def test_nv12_preprocess_is_bit_identical_to_the_bgr_path_and_the_oracle(geom, n_total, stride):
    f = _video(geom, n_total, stride)
    dev = torch.from_numpy(f).cuda()
    bgr = nv12_to_bgr(dev, geom[:2], geom[3])
    want_bgr = _ref_bgr(f[::stride], geom)
    n_out = -(-n_total // stride)
    for size in SIZES:
        got = frames_to_tensor(dev, size, stride=stride, pixel_format="nv12", frame_size=geom[:2], uv_row=geom[3])
        assert tuple(got.shape) == (n_out, 3, size[1], size[0]) and got.dtype == torch.float32 and got.is_cuda
        assert torch.equal(got, frames_to_tensor(bgr, size, stride=stride))
        # the oracle on the oracle's BGR: the criterion of tests/test_gpu_summary.py's strided test
        assert np.array_equal(got.cpu().numpy(), preproc_ref.frames_to_tensor(want_bgr, size))
    if n_out > 2:
        assert not got[2].any()                                         # the constant frame: mn == mx, 0 / 1e-7


def test_nv12_preprocess_other_colorspace_and_unaligned_base():
    geom, n_total, stride = (36, 64, 80, 40), 7, 3
    f = _video(geom, n_total, stride)
    dev = torch.from_numpy(f).cuda()
    got = frames_to_tensor(dev, (40, 40), stride=stride, pixel_format="nv12", frame_size=geom[:2], uv_row=geom[3], colorspace="bt709-full")
    assert np.array_equal(got.cpu().numpy(), preproc_ref.frames_to_tensor(_ref_bgr(f[::stride], geom, "bt709-full"), (40, 40)))
    assert not torch.equal(got, frames_to_tensor(dev, (40, 40), stride=stride, pixel_format="nv12", frame_size=geom[:2], uv_row=geom[3]))
    flat = torch.zeros(f.size + 3, dtype=torch.uint8, device="cuda")
    flat[3:] = dev.view(-1)
    odd = flat[3:].view(f.shape)
    assert odd.data_ptr() % 16 == 3
    assert torch.equal(frames_to_tensor(odd, (40, 40), stride=stride, pixel_format="nv12", frame_size=geom[:2], uv_row=geom[3],
                                        colorspace="bt709-full"), got)


def test_host_nv12_uploads_only_the_kept_frames():
    geom, n_total, stride = (90, 160, 160, 96), 150, 60
    f = _video(geom, n_total, stride)
    want = frames_to_tensor(torch.from_numpy(f).cuda(), (40, 40), stride=stride, pixel_format="nv12", frame_size=geom[:2], uv_row=geom[3])
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    before = torch.cuda.memory_allocated()
    got = frames_to_tensor(f, (40, 40), stride=stride, pixel_format="nv12", frame_size=geom[:2], uv_row=geom[3])
    torch.cuda.synchronize()
    peak = torch.cuda.max_memory_allocated() - before
    assert torch.equal(got, want)
    kept = 3 * f[0].size
    assert f.size == 50 * kept and peak < 8 * kept, f"peak {peak} B for {kept} B of kept frames: the whole video ({f.size} B) was uploaded"


# ---- 4. the converting gather -----------------------------------------------------------------------------------------------------
def _gather_both(f, geom, cps, selected, capacity, sentinel=0xAB):
    """goalnet_nv12_gather_clips_bgr on the NV12 video and goalnet_gather_clips on the converted one, both with two guard frames"""
    dev = torch.device("cuda")
    h0, w0 = geom[:2]
    t = torch.from_numpy(f).to(dev)
    bgr = nv12_to_bgr(t, geom[:2], geom[3])
    cp = torch.tensor(cps, dtype=torch.int32, device=dev)
    sel = torch.tensor(selected, dtype=torch.int32, device=dev)
    res = []
    for which in ("nv12", "bgr"):
        out = torch.full((max(capacity, 1) + 2, h0, w0, 3), sentinel, dtype=torch.uint8, device=dev)
        src = torch.full((max(capacity, 1) + 2,), -7, dtype=torch.int32, device=dev)
        count = torch.full((1,), -1, dtype=torch.int64, device=dev)
        status = torch.full((1,), -1, dtype=torch.int32, device=dev)
        if which == "nv12":
            nv12.gather_clips_bgr(t, geom[:2], geom[3], "bt601", cp, sel, out, capacity, src, count, status)
        else:
            ops.gather_clips(bgr, cp, sel, out, capacity, src, count, status)
        res.append((out.cpu().numpy(), src.cpu().numpy(), int(count.item()), int(status.item())))
    (out, src, count, status), (out2, src2, count2, status2) = res
    assert np.array_equal(out, out2) and np.array_equal(src, src2) and (count, status) == (count2, status2)
    return out, src, count, status


@pytest.mark.parametrize("geom", [(4, 6, 6, 4), (18, 34, 34, 18), (36, 64, 80, 40), (90, 160, 160, 96)])
def test_nv12_gather_clips_direct(geom):
    full_n = 50
    f = _video(geom, full_n, seed=3)
    want_all = _ref_bgr(f, geom)
    # the clip table of tests/test_gpu_summary.py::test_gather_clips_direct
    cps = [[40, 57], [9, 9], [0, 30], [10, 13], [60, 70]]
    selected = [1, 1, 0, 1, 1]
    want = np.concatenate([want_all[40:57], want_all[10:13]])
    want_src = np.concatenate([np.arange(40, 50), np.arange(10, 13)])
    out, src, count, status = _gather_both(f, geom, cps, selected, 13)
    assert (count, status) == (13, 0)
    assert np.array_equal(out[:13], want) and np.array_equal(src[:13], want_src)
    assert (out[13:] == 0xAB).all() and (src[13:] == -7).all()          # the guard band
    out, src, count, status = _gather_both(f, geom, cps, selected, 12)  # one frame short
    assert count == 13 and status != 0
    assert np.array_equal(out[:12], want[:12]) and (out[12:] == 0xAB).all() and (src[12:] == -7).all()
    out, src, count, status = _gather_both(f, geom, cps, [0, 0, 0, 0, 0], 13)
    assert (count, status) == (0, 0) and (out == 0xAB).all()
    out, src, count, status = _gather_both(f, geom, cps, selected, 0)   # no copy is launched at all
    assert count == 13 and status != 0 and (out == 0xAB).all()


def test_nv12_gather_300_clips():
    """more clips than the scan block has threads; frames of more than one tile of 256 blocks (270 x 480: 4050 blocks)"""
    rng = np.random.default_rng(4)
    for geom, full_n, share in (((36, 64, 80, 40), 1200, 0.1), ((270, 480, 512, 272), 330, 0.03)):
        n_clips = 300
        f = _video(geom, full_n, seed=5)
        cuts = np.sort(rng.choice(np.arange(1, full_n), size=n_clips - 1, replace=False))
        cps = np.stack([np.concatenate([[0], cuts]), np.concatenate([cuts - 1, [full_n - 1]])], axis=1)
        selected = (rng.random(n_clips) < share).astype(np.int32)
        idx = np.nonzero(selected)[0]
        want_src = np.concatenate([np.arange(full_n)[a:b] for a, b in cps[idx]])
        assert 1 <= len(want_src) <= 200
        out, src, count, status = _gather_both(f, geom, cps.tolist(), selected.tolist(), len(want_src) + 3)
        assert (count, status) == (len(want_src), 0)
        assert np.array_equal(src[:count], want_src) and np.array_equal(out[:count], _ref_bgr(f[want_src], geom))
        assert (out[count:] == 0xAB).all()


def test_gather_refuses_a_small_workspace_on_the_device_too():
    lib = _lib.load()
    c = (ctypes.c_int32 * 8)(*nv12_coefficients("bt601").tolist())
    t = torch.zeros(64, dtype=torch.int64, device="cuda")
    p = t.data_ptr()
    assert lib.goalnet_nv12_gather_clips_bgr(p, 2, 2, 2, 2, 4, 6, c, p, p, 3, p, 1, p, p, p, p, 8, None) == -4
    torch.cuda.synchronize()
    assert not t.any()                                                  # refused before any launch


# ---- 5. end to end ----------------------------------------------------------------------------------------------------------------
E2E = (36, 64, 80, 40)


def _clips(full_n, n_clips, seed):
    rng = np.random.default_rng(seed)
    cuts = np.sort(rng.choice(np.arange(1, full_n), size=n_clips - 1, replace=False))
    return np.stack([np.concatenate([[0], cuts]), np.concatenate([cuts - 1, [full_n - 1]])], axis=1).astype(np.int32)


def _same(a, b):
    assert torch.equal(a.predictions, b.predictions) and np.array_equal(a.frame_indices, b.frame_indices)
    assert a.selected == b.selected and torch.equal(a.src_index, b.src_index) and torch.equal(a.frames, b.frames)
    assert (a.change_points is None) == (b.change_points is None)
    if a.change_points is not None:
        assert np.array_equal(a.change_points, b.change_points)


@pytest.mark.parametrize("audio", [False, True])
def test_video_summarizer_nv12_end_to_end(audio):
    torch.manual_seed(41)
    full_n, skip = 150, 15
    f = _video(E2E, full_n, skip, seed=6)
    cps = _clips(full_n, 15, seed=7)
    n = full_n // skip
    aud = torch.from_numpy(synth.make_audio(n)).cuda() if audio else None
    model = AVM(audio_included=audio, device="cuda:0", seed=synth.BASE_SEED).eval()
    dev = torch.from_numpy(f).cuda()
    bgr = nv12_to_bgr(dev, E2E[:2], E2E[3])
    kw = dict(pixel_format="nv12", frame_size=E2E[:2], uv_row=E2E[3])
    vs = VideoSummarizer(model, cps, skip_frames=skip, size=(40, 40))
    want = vs(bgr, audio_features=aud)
    got = vs(dev, audio_features=aud, **kw)
    assert len(want.selected) >= 1 and want.frames.shape[0] >= 1
    assert tuple(got.frames.shape[1:]) == (36, 64, 3) and got.frames.dtype == torch.uint8
    _same(got, want)
    assert np.array_equal(got.frames.cpu().numpy(), _ref_bgr(f[got.src_index.cpu().numpy()], E2E))
    _same(vs(f, audio_features=aud, **kw), want)                        # host-resident NV12
    # NV12 out: the source frames' bytes, padding and all
    raw = vs(dev, audio_features=aud, output_format="nv12", **kw)
    assert tuple(raw.frames.shape[1:]) == f.shape[1:] and torch.equal(raw.src_index, want.src_index)
    assert torch.equal(raw.predictions, want.predictions) and raw.selected == want.selected
    assert np.array_equal(raw.frames.cpu().numpy(), f[want.src_index.cpu().numpy()])
    # another colour space is another video
    other = vs(dev, audio_features=aud, colorspace="bt709-full", **kw)
    _same(other, vs(nv12_to_bgr(dev, E2E[:2], E2E[3], "bt709-full"), audio_features=aud))


def test_video_summarizer_nv12_with_a_segmenter():
    """TemporalSegmenter's default arguments find no change point in the descriptors of a randomly initialised model (see
    tests/test_gpu_kts.py) and the knapsack cannot take a clip of the whole video; lmax = 1 makes every sample a segment, so that a
    summary exists. The path through the summariser is the same."""
    torch.manual_seed(43)
    full_n, skip = 150, 15
    f = _video(E2E, full_n, skip, seed=8)
    model = AVM(audio_included=False, device="cuda:0", seed=synth.BASE_SEED).eval()
    dev = torch.from_numpy(f).cuda()
    vs = VideoSummarizer(model, None, skip_frames=skip, segmenter=TemporalSegmenter(max_change_points=9, lmax=1))
    want = vs(nv12_to_bgr(dev, E2E[:2], E2E[3]))
    got = vs(dev, pixel_format="nv12", frame_size=E2E[:2], uv_row=E2E[3])
    assert want.change_points is not None and want.change_points.shape == (10, 2) and len(want.selected) >= 1
    _same(got, want)
    raw = vs(dev, pixel_format="nv12", frame_size=E2E[:2], uv_row=E2E[3], output_format="nv12")
    assert np.array_equal(raw.change_points, want.change_points)
    assert np.array_equal(raw.frames.cpu().numpy(), f[want.src_index.cpu().numpy()])
