"""motioncraft_amd: MI355X-native (gfx950) STMoGen sampling hot path behind the reference's
mogen registry / mmcv-Config API.  See DESIGN.md and INTEGRATION.md."""
from .builder import (ARCHITECTURES, ATTENTIONS, LOSSES, MODELS, SUBMODULES, build_architecture, build_attention,
                      build_loss, build_submodule)
from .config import Config, ConfigDict
from .registry import Registry, build_from_cfg
from . import models as _models  # registers MotionDiffusion / STMoGenTransformer / STMA / MSELoss
from .models import ControlT2MHalf, wrap_fp16_model
from .checkpoint import load_checkpoint
from . import scoring
from .scoring import BeatAlignment, M2DScorer, OnsetDetector, S2GScorer, face_errors
from . import audio
from .audio import Resampler, load_wav
from . import render
from .render import DirectionalLight, MeshRenderer, OrthographicCamera
from . import skeleton
from .skeleton import KIT_CHAINS, T2M_CHAINS, Mplot3dCamera, SkeletonRenderer
from . import video
from .video import AviWriter, JpegEncoder, save_avi
from . import embmetrics
from . import speech
from .speech import AudioCondition, sample_speech, speech_frames, speech_prompt

__all__ = ['embmetrics', 'video', 'AviWriter', 'JpegEncoder', 'save_avi', 'skeleton', 'KIT_CHAINS', 'T2M_CHAINS', 'Mplot3dCamera', 'SkeletonRenderer', 'render', 'DirectionalLight', 'MeshRenderer', 'OrthographicCamera', 'audio', 'Resampler', 'load_wav', 'AudioCondition', 'sample_speech', 'speech', 'speech_frames', 'speech_prompt', 'BeatAlignment', 'M2DScorer', 'OnsetDetector', 'S2GScorer', 'face_errors', 'scoring','ARCHITECTURES', 'ATTENTIONS', 'LOSSES', 'MODELS', 'SUBMODULES', 'build_architecture',
           'build_attention', 'build_loss', 'build_submodule', 'Config', 'ConfigDict', 'Registry', 'build_from_cfg', 'ControlT2MHalf',
           'load_checkpoint', 'wrap_fp16_model']
