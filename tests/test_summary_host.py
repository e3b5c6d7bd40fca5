"""CPU: the inference-mode entry points (csrc/summary.hip, cvml_goalnet_amd/summarize.py) check their arguments before any launch,
and the Python surface fails loudly without a GPU (no compute calls)."""
import numpy as np
import pytest
import torch

from cvml_goalnet_amd import _lib

P = 16      # any non-NULL address: the argument checks return before a pointer is used


def test_strided_preprocess_argument_errors():
    lib = _lib.load()
    assert lib.goalnet_frames_preprocess_strided(None, 10, 2, 8, 8, P, 4, 4, P, None) == -1 and b"null" in lib.goalnet_last_error()
    assert lib.goalnet_frames_preprocess_strided(P, 10, 2, 8, 8, None, 4, 4, P, None) == -1
    assert lib.goalnet_frames_preprocess_strided(P, 10, 2, 8, 8, P, 4, 4, None, None) == -1
    assert lib.goalnet_frames_preprocess_strided(P, 10, 0, 8, 8, P, 4, 4, P, None) == -2 and b"frame_stride" in lib.goalnet_last_error()
    assert lib.goalnet_frames_preprocess_strided(P, 0, 2, 8, 8, P, 4, 4, P, None) == -2 and b"n_total" in lib.goalnet_last_error()
    assert lib.goalnet_frames_preprocess_strided(P, 10, 2, 0, 8, P, 4, 4, P, None) == -2 and b"dim" in lib.goalnet_last_error()


def test_gather_clips_argument_errors():
    lib = _lib.load()
    ws = lib.goalnet_gather_clips_ws_bytes(7)
    assert ws > 0 and lib.goalnet_gather_clips_ws_bytes(1) > 0 and lib.goalnet_gather_clips_ws_bytes(5000) >= 5001 * 8 + 5000 * 4
    good = dict(frames=P, full_n=100, frame_bytes=180, cps=P, sel=P, n_clips=7, out=P, cap=15, src=P, count=P, status=P, ws=P, ws_bytes=ws)

    def call(**kw):
        a = {**good, **kw}
        return lib.goalnet_gather_clips(a["frames"], a["full_n"], a["frame_bytes"], a["cps"], a["sel"], a["n_clips"], a["out"], a["cap"],
                                        a["src"], a["count"], a["status"], a["ws"], a["ws_bytes"], None)

    for name in ("frames", "cps", "sel", "out", "src", "count", "status", "ws"):
        assert call(**{name: None}) == -1 and b"null" in lib.goalnet_last_error(), name
    assert call(frame_bytes=0) == -2 and b"frame_bytes" in lib.goalnet_last_error()
    assert call(full_n=0) == -2 and b"full_n" in lib.goalnet_last_error()
    assert call(n_clips=0) == -2 and b"n_clips" in lib.goalnet_last_error()
    assert call(cap=-1) == -2
    assert call(ws_bytes=ws - 1) == -4 and b"workspace" in lib.goalnet_last_error()


def test_fails_loudly_without_a_gpu(monkeypatch):
    monkeypatch.setattr(torch.cuda, "is_available", lambda: False)
    from cvml_goalnet_amd import AVM, GoalnetError, VideoSummarizer
    from cvml_goalnet_amd.preprocess import frames_to_tensor
    frames = np.zeros((6, 8, 8, 3), dtype=np.uint8)
    with pytest.raises(GoalnetError):
        frames_to_tensor(frames, (4, 4), stride=2)
    cps = np.array([[0, 2], [3, 5]])
    with pytest.raises(GoalnetError):
        VideoSummarizer(AVM(audio_included=False), cps, skip_frames=2)(frames)


def test_argument_checks_come_first(monkeypatch):
    monkeypatch.setattr(torch.cuda, "is_available", lambda: False)
    from cvml_goalnet_amd import AVM, VideoSummarizer
    frames = np.zeros((6, 8, 8, 3), dtype=np.uint8)
    cps = np.array([[0, 2], [3, 5]])
    vs = VideoSummarizer(AVM(audio_included=True), cps, skip_frames=2)
    assert vs.skip_frames == 2 and VideoSummarizer(AVM(audio_included=True), cps).skip_frames == 60     # main.py:311
    with pytest.raises(ValueError, match="audio_features or a waveform"):
        vs(frames)                                                       # audio_included=True with neither audio argument
    with pytest.raises(ValueError, match="bin_length"):
        vs(frames, waveform=np.zeros(22050, dtype=np.float32))           # main.py:321 omits it: nothing is guessed
    with pytest.raises(ValueError, match="N = 3 sampled frames"):
        vs(frames, audio_features=torch.zeros(6, 30, 30))                # one row per raw frame instead of per sampled frame
    with pytest.raises(ValueError):
        vs(np.zeros((6, 8, 8), dtype=np.uint8), audio_features=torch.zeros(3, 30, 30))
    with pytest.raises(ValueError):
        VideoSummarizer(AVM(audio_included=False), np.zeros((0, 2)))
    with pytest.raises(ValueError):
        VideoSummarizer(AVM(audio_included=False, head="classifier"), cps)
    with pytest.raises(ValueError):
        VideoSummarizer(AVM(audio_included=False), cps, skip_frames=0)
