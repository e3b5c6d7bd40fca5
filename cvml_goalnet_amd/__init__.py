"""cvml_goalnet_amd — MI355X-native implementation of CVML-GoalNet's one hot path: the `AVM`
frame-importance model (forward, broadcast-MSE, backward, Adam) behind the reference's own Python
surface. See DESIGN.md / INTEGRATION.md.

    from cvml_goalnet_amd import AVM               # drop-in for /root/reference/utils.py:229 `AVM`
    from cvml_goalnet_amd import VideoSummarizer   # /root/reference/main.py:315-345 (`--infer`) on a video resident on the GPU
    from cvml_goalnet_amd import epoch_plan, gather_augmented  # shuffled / augmented passes drawn on the GPU (extension)
    from cvml_goalnet_amd import epoch_plan2, gather_audio_augmented, gather_mixed, mix_rows  # audio augmentation and mixup on such a pass (extension)
    from cvml_goalnet_amd import load_audio, to_mono, read_wav, resample_plan, resample_taps  # the audio front end: downmix and resample to 22 050 Hz on the GPU (extension)
    from cvml_goalnet_amd import nv12_to_bgr, nv12_coefficients  # NV12 frames of a hardware decoder in, BGR or NV12 out (extension)
    from cvml_goalnet_amd import storyboard, select_keyframes, render_thumbnails, Storyboard  # the static summary: keyframes, thumbnails and a contact sheet; storyboard.storyboard(...) does both steps (extension)
    from cvml_goalnet_amd import EmaOptions        # a weight average behind the fused step; exact save / resume (extension)
    from cvml_goalnet_amd import TemporalSegmenter # KTS change points for a video outside the dataset (extension, parity unpinned)
"""
from . import synth  # noqa: F401
from ._lib import GoalnetError, LIB_PATH  # noqa: F401
from .avm import AVM  # noqa: F401
from . import optim  # noqa: F401
from .optim import EmaOptions, OptimOptions, ParamGroup  # noqa: F401
from .summarize import VideoSummarizer, VideoSummary  # noqa: F401
from . import groundtruth  # noqa: F401
from .segment import Segmentation, TemporalSegmenter  # noqa: F401
from .rankcorr import HumanConsistency, RankCorrelation, RankEvaluator, rank_correlation  # noqa: F401
from .augment import epoch_plan, gather_augmented  # noqa: F401
from .augment import epoch_plan2, gather_audio_augmented, gather_mixed, mix_rows  # noqa: F401
from .waveform import load_audio, read_wav, resample_plan, resample_taps, to_mono  # noqa: F401
from . import nv12  # noqa: F401
from .nv12 import nv12_coefficients, nv12_to_bgr  # noqa: F401
from . import storyboard  # noqa: F401
from .storyboard import Storyboard, render_thumbnails, select_keyframes  # noqa: F401

__all__ = ["storyboard", "Storyboard", "select_keyframes", "render_thumbnails", "nv12", "nv12_coefficients", "nv12_to_bgr", "load_audio", "read_wav", "resample_plan", "resample_taps", "to_mono", "epoch_plan", "gather_augmented", "epoch_plan2", "gather_audio_augmented", "gather_mixed", "mix_rows", "AVM", "GoalnetError", "synth", "LIB_PATH", "optim", "OptimOptions", "ParamGroup", "EmaOptions","VideoSummarizer", "VideoSummary", "groundtruth", "TemporalSegmenter",
           "Segmentation", "RankEvaluator", "RankCorrelation", "HumanConsistency", "rank_correlation"]
