"""The scoring half of the speech-to-gesture (S2G) and music-to-dance (M2D) tests: what the reference prints at the end of
``tools/s2g_test.py`` (``CustomTrainer.test``, lines 262-483) and ``tools/m2d_test.py`` (``finedance_eval``, lines 234-309).

  * ``BeatAlignment``: ``alignment.load_pose`` + ``alignment.calculate_align`` of ``mogen/datasets/EMAGE_2024/utils/metric.py``
    (lines 78-127, 199-242) on the device (``mc_beat_mask`` / ``mc_beat_align``, ``csrc/mc_metrics.hip``), fed the 55 joints
    ``SMPLXBodyModel.joints`` leaves there.
  * ``OnsetDetector`` / ``BeatAlignment.load_audio``: ``alignment.load_audio`` (metric.py:64-76), i.e. librosa 0.10.1's
    ``onset.onset_detect(y, sr, hop_length=512, units='time')`` with its defaults, on the device (``mc_onset_strength`` /
    ``mc_onset_pick``, ``csrc/mc_onset.hip``) from a waveform that is already decoded and at the detector's rate.  librosa is not
    a dependency: parity is pinned to the float64 restatement ``tests/onset_ref.py``.  Decoding an integer PCM wav and resampling it
    to the detector's rate is ``motioncraft_amd.audio.load_wav``, also on the device: the reference's ``librosa.load`` +
    ``librosa.resample`` in librosa's ``polyphase`` mode (``scipy.signal.resample_poly``), not ``soxr_hq``, whose parity stays
    unpinned.  Compressed and float files stay with the caller.
  * ``face_errors``: the face ``l2`` / ``lvel`` errors of ``s2g_test.py:377-412``; the two vertex sets are reduced to the two
    sums on the device (``mc_smplx_vertex_errors``) and never leave it.
  * ``S2GScorer`` / ``M2DScorer``: the accumulation and the printed numbers of the two tools, on the existing ``L1div``, FID and
    diversity functions of ``evaluation`` and the device embedding model.

Nothing here falls back to the host: the kernels are the only implementation, and a missing library or GPU is an error.
"""
import ctypes

import numpy as np
import torch

from . import embmetrics, lib as _lib
from .lib import ptr as _p, stream as _stream
from .body_model import DEFAULT_WORK_BYTES, NUM_JOINTS
from .evaluation import L1div, calculate_activation_statistics, calculate_diversity, calculate_frechet_distance

UPPER_BODY = (3, 6, 9, 12, 13, 14, 15, 16, 17, 18, 19, 20, 21)           # metric.py:55
MAX_ORDER, MAX_UPPER = _lib.MC_BEAT_MAX_ORDER, _lib.MC_BEAT_MAX_UPPER
M2D_MAX_FRAMES = 4096                                                    # m2d_test.py:243


class Beats:
    """What ``load_pose`` returns: the beat mask uint8 [55, t_end - t_start] on the device.  Iterating (or ``lists()``) gives the
    reference's form, one int64 array of slice-relative beat frames per joint."""

    def __init__(self, mask):
        self.mask = mask

    def lists(self):
        m = self.mask.cpu().numpy()
        return [np.flatnonzero(row).astype(np.int64) for row in m]

    def __iter__(self):
        return iter(self.lists())

    def __len__(self):
        return self.mask.shape[0]


def _check_onsets(onset_times):
    on = np.ascontiguousarray(np.asarray(onset_times, dtype=np.float64).reshape(-1))
    if on.size < 1:
        raise ValueError('no onset times: the align score is a mean over the onsets')
    return on


def mel_filter_bank(sr, n_fft, n_mels):
    """librosa.filters.mel with its defaults (Slaney scale and norm, fmin 0, fmax sr / 2): float32 [n_mels, n_fft // 2 + 1], computed
    in float64.  The scale is f / (200 / 3) below 1 kHz and logarithmic above, 27 steps per factor 6.4."""
    step = np.log(6.4) / 27
    top = sr / 2
    mel_top = 15.0 + np.log(top / 1000.0) / step if top >= 1000.0 else top / (200.0 / 3)
    mels = np.linspace(0.0, mel_top, n_mels + 2)
    edges = np.where(mels >= 15.0, 1000.0 * np.exp(step * (mels - 15.0)), (200.0 / 3) * mels)
    freqs = np.arange(n_fft // 2 + 1) * (sr / n_fft)
    lower = (freqs[None, :] - edges[:-2, None]) / (edges[1:-1] - edges[:-2])[:, None]
    upper = (edges[2:, None] - freqs[None, :]) / (edges[2:] - edges[1:-1])[:, None]
    return (np.maximum(0.0, np.minimum(lower, upper)) * (2.0 / (edges[2:] - edges[:-2]))[:, None]).astype(np.float32)


def dft_table(n_fft):
    """float32 [n_fft, 2 (n_fft // 2 + 1)], computed in float64: column 2b = w[k] cos(2 pi k b / n_fft), column 2b + 1 =
    -w[k] sin(2 pi k b / n_fft) with w the periodic Hann window; the angle is reduced as the integer k b mod n_fft first."""
    k = np.arange(n_fft, dtype=np.int64)
    ang = (2 * np.pi / n_fft) * ((k[:, None] * np.arange(n_fft // 2 + 1, dtype=np.int64)[None, :]) % n_fft)
    w = (0.5 - 0.5 * np.cos(2 * np.pi * k / n_fft))[:, None]
    return np.stack([w * np.cos(ang), -w * np.sin(ang)], axis=-1).reshape(n_fft, -1).astype(np.float32)


class OnsetDetector:
    """``librosa.onset.onset_detect`` of librosa 0.10.1 with its defaults, on the device: log-power mel spectrogram (periodic Hann
    window, ``center=True`` with zero padding, 128 Slaney mel bands, top_db 80), spectral flux with lag 1 averaged over the bands,
    min/max normalisation, ``peak_pick`` with pre_max 0.03 s, post_max 0, pre_avg 0.1 s, post_avg 0.1 s, wait 0.03 s, delta 0.07.
    The waveform is taken as float32 at ``sr``; ``audio.Resampler`` / ``audio.load_wav`` bring one there."""
    DELTA = 0.07
    N_FFT, MAX_HOP, MAX_MELS = _lib.MC_ONSET_N_FFT, _lib.MC_ONSET_MAX_HOP, _lib.MC_ONSET_MAX_MELS

    def __init__(self, sr=16000, hop_length=512, n_fft=2048, n_mels=128):
        self.sr, self.hop_length, self.n_fft, self.n_mels = float(sr), int(hop_length), int(n_fft), int(n_mels)
        if not self.sr > 0:
            raise ValueError(f'sr={sr}: must be positive')
        if self.n_fft != self.N_FFT:
            raise ValueError(f'n_fft={n_fft}: the kernel is written for {self.N_FFT}')
        if not 4 <= self.hop_length <= self.MAX_HOP or self.hop_length % 4:
            raise ValueError(f'hop_length={hop_length}: a multiple of 4 in 4..{self.MAX_HOP}')
        if not 1 <= self.n_mels <= self.MAX_MELS:
            raise ValueError(f'n_mels={n_mels}: 1..{self.MAX_MELS}')
        self.mel_basis = mel_filter_bank(self.sr, self.n_fft, self.n_mels)
        sec = lambda t, extra=0: int(t * self.sr // self.hop_length + extra)      # onset_detect's defaults, in frames
        self.pre_max, self.post_max, self.pre_avg, self.post_avg, self.wait = sec(0.03), sec(0.00, 1), sec(0.10), sec(0.10, 1), sec(0.03)
        self._dft = None
        self._dev = {}

    def num_frames(self, n_samples):
        return 1 + int(n_samples) // self.hop_length

    @staticmethod
    def _check_wave(y):
        t = torch.as_tensor(y)
        if t.dim() != 1:
            raise ValueError(f'audio must be 1-D (mono samples), got {tuple(t.shape)}')
        if t.numel() < 1:
            raise ValueError('audio holds no sample')
        if not t.is_floating_point():
            raise ValueError(f'audio must be floating point, got {t.dtype}')
        if not bool(torch.isfinite(t).all()):
            raise ValueError('audio is not finite everywhere')
        return t

    def _tables(self, device):
        if device not in self._dev:
            if self._dft is None:
                self._dft = dft_table(self.n_fft)
            self._dev[device] = (torch.from_numpy(self._dft).to(device), torch.from_numpy(self.mel_basis).to(device))
            torch.cuda.current_stream(device).synchronize()                # the upload is done before any stream reads the cache
        return self._dev[device]

    def _strength(self, t):
        lib = _lib.load(require_gpu=True)
        t = t.to(device=t.device if t.is_cuda else 'cuda', dtype=torch.float32).contiguous()
        dft, mel = self._tables(t.device)
        n = t.numel()
        wb = int(lib.mc_onset_work_bytes(n, self.n_fft, self.hop_length, self.n_mels))
        if wb < 0:
            raise ValueError(f'{n} samples at hop {self.hop_length}: more frames than the kernels take')
        work = torch.empty(wb // 4, device=t.device, dtype=torch.float32)
        env = torch.empty(self.num_frames(n), device=t.device, dtype=torch.float32)
        _lib.check(lib.mc_onset_strength(_p(t), n, _p(dft), _p(mel), self.n_fft, self.hop_length, self.n_mels, _p(work), wb, _p(env), _stream()),
                   'mc_onset_strength')
        return env

    def strength(self, y):
        """y [N] (device tensor, or anything ``torch.as_tensor`` takes) -> the un-normalised onset envelope, device fp32
        [1 + N // hop_length] (``librosa.onset.onset_strength``)."""
        return self._strength(self._check_wave(y))

    def pick(self, env):
        """envelope [F] on the device -> (onset mask uint8 [F], count int32 [1]), both on the device."""
        if not isinstance(env, torch.Tensor) or not env.is_cuda or env.dtype != torch.float32 or env.dim() != 1 or env.numel() < 1:
            raise ValueError('env must be a float32 device tensor [F] with at least one frame (what strength returns)')
        env = env.contiguous()
        lib = _lib.load(require_gpu=True)
        mask = torch.empty(env.numel(), device=env.device, dtype=torch.uint8)
        count = torch.empty(1, device=env.device, dtype=torch.int32)
        _lib.check(lib.mc_onset_pick(_p(env), env.numel(), self.pre_max, self.post_max, self.pre_avg, self.post_avg, self.DELTA, self.wait, 1,
                                     _p(mask), _p(count), _stream()), 'mc_onset_pick')
        return mask, count

    def detect(self, y, units='time'):
        """-> the onsets as float64 seconds (``units='time'``) or int64 frames (``units='frames'``), a numpy array."""
        if units not in ('time', 'frames'):
            raise ValueError(f"units={units!r}: 'time' or 'frames'")
        mask, _ = self.pick(self._strength(self._check_wave(y)))
        frames = np.flatnonzero(mask.cpu().numpy()).astype(np.int64)
        return frames if units == 'frames' else (frames * self.hop_length).astype(np.int64) / self.sr


class BeatAlignment:
    """``alignment(sigma, order, mmae, upper_body)`` of metric.py:54-62 with its method names.  ``mean_vel`` [55]: float32 divides
    the fp32 speeds in fp32, anything else in float64, as numpy would."""

    def __init__(self, sigma, order, mean_vel, upper_body=UPPER_BODY):
        self.sigma, self.order = float(sigma), int(order)
        self.upper_body = [int(j) for j in upper_body]
        self.threshold = 0.3                                             # metric.py:62
        mv = np.asarray(mean_vel)
        if mv.shape != (NUM_JOINTS,):
            raise ValueError(f'mean_vel must be [{NUM_JOINTS}], got {mv.shape}')
        if not 1 <= self.order <= MAX_ORDER:
            raise ValueError(f'order={self.order}: 1..{MAX_ORDER}')
        if not self.sigma > 0:
            raise ValueError(f'sigma={self.sigma}: must be positive')
        if not 1 <= len(self.upper_body) <= MAX_UPPER or any(not 0 <= j < NUM_JOINTS for j in self.upper_body):
            raise ValueError(f'upper_body: 1..{MAX_UPPER} joint indices below {NUM_JOINTS}, got {self.upper_body}')
        self.mean_vel_fp32 = int(mv.dtype == np.float32)
        self.mean_vel = np.ascontiguousarray(mv, dtype=np.float64)       # an fp32 value widens exactly
        self._mv_dev = None
        self._detectors = {}

    def load_audio(self, wave, t_start=None, t_end=None, sr_audio=16000):
        """metric.py:64-76 with ``without_file=True``: the onset times (float64 seconds, relative to the slice) of
        ``wave[t_start:t_end]``, or of the whole wave without ``t_start``; hop 512 as there."""
        if sr_audio not in self._detectors:
            self._detectors[sr_audio] = OnsetDetector(sr=sr_audio, hop_length=512)
        wave = torch.as_tensor(wave)
        if wave.dim() != 1:
            raise ValueError(f'audio must be 1-D (mono samples), got {tuple(wave.shape)}')
        return self._detectors[sr_audio].detect(wave if t_start is None else wave[t_start:t_end])

    @staticmethod
    def _check_pose(joints, t_start, t_end, pose_fps):
        shape = tuple(joints.shape)
        if len(shape) != 3 or shape[1:] != (NUM_JOINTS, 3):
            raise ValueError(f'joints must be [T, {NUM_JOINTS}, 3], got {shape}')
        t_start, t_end = int(t_start), int(t_end)
        if t_end - t_start < 1:
            raise ValueError(f'the slice [{t_start}, {t_end}) holds no frame')
        if shape[0] < 2 or t_start < 0 or t_end > shape[0]:
            raise ValueError(f'the slice [{t_start}, {t_end}) must lie within the {shape[0]} frames (at least 2)')
        if not float(pose_fps) > 0:
            raise ValueError(f'pose_fps={pose_fps}: must be positive')
        return t_start, t_end

    def load_pose(self, joints, t_start, t_end, pose_fps):
        """joints fp32 [T, 55, 3] (device tensor, or anything ``torch.as_tensor`` takes) -> ``Beats`` of the frames
        ``t_start:t_end`` (metric.py:78-127 with ``without_file=True``)."""
        t_start, t_end = self._check_pose(joints, t_start, t_end, pose_fps)
        lib = _lib.load(require_gpu=True)
        j = torch.as_tensor(joints)
        j = j.to(device=j.device if j.is_cuda else 'cuda', dtype=torch.float32).contiguous()
        if self._mv_dev is None or self._mv_dev.device != j.device:
            self._mv_dev = torch.from_numpy(self.mean_vel).to(j.device)
        mask = torch.empty(NUM_JOINTS, t_end - t_start, device=j.device, dtype=torch.uint8)
        _lib.check(lib.mc_beat_mask(_p(j), j.shape[0], NUM_JOINTS, _p(self._mv_dev), self.mean_vel_fp32, t_start, t_end, float(pose_fps),
                                    self.order, self.threshold, _p(mask), _stream()), 'mc_beat_mask')
        return Beats(mask)

    def _align(self, onsets, beats, pose_fps):
        lib = _lib.load(require_gpu=True)
        mask = beats.mask
        on = torch.from_numpy(onsets).to(mask.device)
        nj, n, nu = mask.shape[0], mask.shape[1], len(self.upper_body)
        wb = int(lib.mc_beat_align_work_bytes(n, nu))
        work = torch.empty(wb // 8 + 1, device=mask.device, dtype=torch.float64)
        score = torch.empty(1, device=mask.device, dtype=torch.float64)
        upper = (ctypes.c_int32 * nu)(*self.upper_body)
        _lib.check(lib.mc_beat_align(_p(mask), nj, n, upper, nu, _p(on), on.numel(), float(pose_fps), self.sigma, _p(work), work.numel() * 8,
                                     _p(score), _stream()), 'mc_beat_align')
        return float(score.item())

    def calculate_align(self, onset_times, beats, pose_fps=30):
        """onset times in seconds + the ``Beats`` of ``load_pose`` -> the align score (metric.py:228-242)."""
        onsets = _check_onsets(onset_times)
        if not isinstance(beats, Beats):
            raise TypeError('beats: the object load_pose returned')
        if not float(pose_fps) > 0:
            raise ValueError(f'pose_fps={pose_fps}: must be positive')
        return self._align(onsets, beats, pose_fps)

    def score(self, joints, t_start, t_end, pose_fps, onset_times, return_beats=False):
        """``calculate_align(onset_times, load_pose(joints, t_start, t_end, pose_fps), pose_fps)`` in one call."""
        onsets = _check_onsets(onset_times)
        self._check_pose(joints, t_start, t_end, pose_fps)
        beats = self.load_pose(joints, t_start, t_end, pose_fps)
        s = self._align(onsets, beats, pose_fps)
        return (s, beats) if return_beats else s


# ---- the channel packings of tools/s2g_test.py ---------------------------------------------------------------------------
def _rows(x, width, name):
    x = torch.as_tensor(x)
    if x.dim() != 2 or x.shape[1] != width:
        raise ValueError(f'{name} must be [T, {width}], got {tuple(x.shape)}')
    return x.float()


def unpack_rec_motion(rec_motion):
    """The sampled 322-d motion -> (rec_pose [T,165], rec_exp [T,100], rec_trans [T,3]), s2g_test.py:290-297: body 0:66 stays,
    the jaw comes from 156:159, the hands (motion 66:156) go to 75:165, the eyes stay zero."""
    m = _rows(rec_motion, 322, 'rec_motion')
    pose = m.new_zeros(m.shape[0], 165)
    pose[:, :66] = m[:, :66]
    pose[:, 66:69] = m[:, 156:159]
    pose[:, 75:165] = m[:, 66:156]
    return pose, m[:, 209:309], m[:, 309:312]


def pack_motion(pose, exps, trans):
    """The inverse for the target (s2g_test.py:306-311): poses / expressions / trans -> the 322-d embedding input; channels
    159:209 and 312:322 stay zero."""
    pose, exps, trans = _rows(pose, 165, 'pose'), _rows(exps, 100, 'expressions'), _rows(trans, 3, 'trans')
    m = pose.new_zeros(pose.shape[0], 322)
    m[:, :66] = pose[:, :66]
    m[:, 66:156] = pose[:, 75:165]
    m[:, 156:159] = pose[:, 66:69]
    m[:, 209:309] = exps
    m[:, 309:312] = trans
    return m


def hand_only_motion(pose, trans):
    """The hand-only embedding input of s2g_test.py:328-342: global orientation, the two hands and the translation; body, jaw
    and expressions zero."""
    pose, trans = _rows(pose, 165, 'pose'), _rows(trans, 3, 'trans')
    m = pose.new_zeros(pose.shape[0], 322)
    m[:, :3] = pose[:, :3]
    m[:, 66:156] = pose[:, 75:165]
    m[:, 309:312] = trans
    return m


def m2d_hand_only_motion(motion):
    """m2d_test.py:265-268: channels 66:156 only."""
    motion = _rows(motion, 322, 'motion')
    m = torch.zeros_like(motion)
    m[:, 66:156] = motion[:, 66:156]
    return m


def face_errors(model, rec_pose, rec_exp, tar_pose, tar_exp, betas, work_bytes=DEFAULT_WORK_BYTES):
    """``(l2, lvel)`` of s2g_test.py:377-412: both body-model calls keep the jaw and the expressions only (every other rotation
    and the translation are subtracted from themselves there), with one beta row per frame; ``model`` adds its mean hand pose to
    the zeroed hands like the package.  l2 = mean (rec - tar)^2, lvel = mean |(rec[1:] - tar[:-1]) - (tar[1:] - tar[:-1])| over
    the vertices, reduced on the device."""
    rec_pose, tar_pose = _rows(rec_pose, 165, 'rec_pose'), _rows(tar_pose, 165, 'tar_pose')
    n = rec_pose.shape[0]
    if tar_pose.shape[0] != n:
        raise ValueError(f'rec_pose holds {n} frames, tar_pose {tar_pose.shape[0]}')
    if n < 2:
        raise ValueError('lvel is a mean over frame pairs: at least 2 frames')

    def jaw_only(p):
        z = torch.zeros_like(p)
        z[:, 66:69] = p[:, 66:69]
        return z
    sums = model.vertex_error_sums(jaw_only(rec_pose), rec_exp, None, jaw_only(tar_pose), tar_exp, None, betas, work_bytes=work_bytes)
    s2, sv = sums.tolist()
    per_frame = 3 * model.num_vertices
    return s2 / (n * per_frame), sv / ((n - 1) * per_frame)


def _fid(gt_emb, pred_emb):
    gt_mu, gt_cov = calculate_activation_statistics(gt_emb, 1.0)
    pr_mu, pr_cov = calculate_activation_statistics(pred_emb, 1.0)
    return calculate_frechet_distance(gt_mu, gt_cov, pr_mu, pr_cov)


def _embed_device(evaluator_model, motion):
    m = motion.float().cuda().unsqueeze(0)
    length = torch.tensor([m.shape[1]], device=m.device)
    return evaluator_model.encode_motion(motion=m, motion_length=length, motion_mask=m, device=m.device).detach()


def _embed(evaluator_model, motion):
    return _embed_device(evaluator_model, motion).cpu().numpy()


def _tables(emb, on_device):
    """the per-sequence embeddings of a scorer as one table per key; ``fid`` reduces a (gt, pred) pair of them"""
    if on_device:
        return {k: torch.cat(v, dim=0) for k, v in emb.items()}, lambda gt, pred: float(embmetrics.frechet_distance(gt, pred).item())
    return {k: np.concatenate(v, axis=0) for k, v in emb.items()}, _fid


class S2GScorer:
    """The accumulators of ``CustomTrainer.test`` (s2g_test.py:262-483): ``add_sequence`` per test sequence, ``summary`` for the
    six numbers it logs.  ``align_mask`` frames are cut from both ends before the beat alignment (:88, :420).  ``on_device``: the
    embeddings stay on the device and the two FIDs are reduced there (``embmetrics.frechet_distance``)."""

    def __init__(self, body_model, evaluator_model, mean_vel, align_mask=60, sigma=0.3, order=7, pose_fps=30, on_device=False):
        self.body_model, self.evaluator_model, self.on_device = body_model, evaluator_model, bool(on_device)
        self.aligner = BeatAlignment(sigma, order, mean_vel)              # s2g_test.py:87
        self.align_mask, self.pose_fps = int(align_mask), pose_fps
        self.l1_calculator = L1div()
        self.align = self.l2_all = self.lvel = 0.0
        self.total_length = self.num_sequences = 0
        self.emb = dict(pred=[], gt=[], hand_pred=[], hand_gt=[])

    def add_sequence(self, rec_motion, tar_pose, tar_exps, tar_trans, tar_beta, onset_times=None, audio=None, audio_sr=16000):
        """rec_motion [T,322] (the sample), tar_pose [T,165], tar_exps [T,100], tar_trans [T,3], tar_beta [T,300] | [300], and
        exactly one of: onset_times [n_on] seconds within the masked window, or audio [N] at ``audio_sr``, from which they are
        detected as :416-419 does: the audio cut to int(audio_sr / pose_fps * T) samples, then
        ``load_audio(cut, a, len(audio) - a)`` with a = int(align_mask * (audio_sr / pose_fps)) -- ``len`` of the UNCUT audio, as
        there; for audio as long as the motion that drops ``a`` samples on both sides."""
        if (onset_times is None) == (audio is None):
            raise ValueError('exactly one of onset_times and audio must be given')
        if audio is not None:
            audio = OnsetDetector._check_wave(audio)
            if not float(audio_sr) > 0:
                raise ValueError(f'audio_sr={audio_sr}: must be positive')
        rec_pose, rec_exp, rec_trans = unpack_rec_motion(rec_motion)
        tar_pose, tar_exps, tar_trans = _rows(tar_pose, 165, 'tar_pose'), _rows(tar_exps, 100, 'tar_exps'), _rows(tar_trans, 3, 'tar_trans')
        T = tar_pose.shape[0]
        if rec_pose.shape[0] != T or tar_exps.shape[0] != T or tar_trans.shape[0] != T:
            raise ValueError('rec_motion, tar_pose, tar_exps and tar_trans must hold the same number of frames')
        onsets = _check_onsets(onset_times) if audio is None else None
        if T - 2 * self.align_mask < 1:
            raise ValueError(f'{T} frames leave nothing between the two masks of {self.align_mask}')
        if audio is not None:
            a_offset = int(self.align_mask * (audio_sr / self.pose_fps))
            cut = audio[:int(audio_sr / self.pose_fps * T)]
            onsets = _check_onsets(self.aligner.load_audio(cut, a_offset, audio.shape[0] - a_offset, sr_audio=audio_sr))
        ev, embed = self.evaluator_model, _embed_device if self.on_device else _embed
        self.emb['pred'].append(embed(ev, _rows(rec_motion, 322, 'rec_motion')))                      # :313-325
        self.emb['gt'].append(embed(ev, pack_motion(tar_pose, tar_exps, tar_trans)))
        self.emb['hand_pred'].append(embed(ev, hand_only_motion(rec_pose, rec_trans)))                 # :328-356
        self.emb['hand_gt'].append(embed(ev, hand_only_motion(tar_pose, tar_trans)))
        beta = torch.as_tensor(tar_beta)
        beta = beta if beta.dim() == 2 else beta.reshape(1, -1).expand(T, -1)
        joints = self.body_model.joints(rec_pose, None, None, beta)                                    # :364-376, :406
        l2, lvel = face_errors(self.body_model, rec_pose, rec_exp, tar_pose, tar_exps, beta)           # :377-412
        self.l2_all += l2 * T
        self.lvel += lvel * T
        self.l1_calculator.run(joints.reshape(T, -1))                                                  # :414
        score = self.aligner.score(joints, self.align_mask, T - self.align_mask, self.pose_fps, onsets)
        self.align += score * (T - 2 * self.align_mask)                                                # :420-422
        self.total_length += T
        self.num_sequences += 1
        return dict(l2=l2, lvel=lvel, align=score)

    def summary(self):
        """The numbers of :451-483 under the names the reference logs them with."""
        if not self.num_sequences:
            raise ValueError('no sequence was added')
        cat, fid = _tables(self.emb, self.on_device)
        return {'l2 loss': self.l2_all / self.total_length,
                'lvel loss': self.lvel / self.total_length,
                'align score': self.align / (self.total_length - 2 * self.num_sequences * self.align_mask),
                'l1div score': self.l1_calculator.avg(),
                'FID(Whole Body) score': fid(cat['gt'], cat['pred']),
                'FID (Hands) score': fid(cat['hand_gt'], cat['hand_pred'])}


class M2DScorer:
    """``finedance_eval``'s scoring loop (m2d_test.py:234-309): whole-body FID, hands FID (channels 66:156 only) and the
    diversity of the sampled embeddings with ``diversity_times = N - 1``.  ``on_device``: as for ``S2GScorer``, the diversity included."""

    def __init__(self, evaluator_model, on_device=False):
        self.evaluator_model, self.on_device = evaluator_model, bool(on_device)
        self.emb = dict(pred=[], gt=[], hand_pred=[], hand_gt=[])

    def add_sequence(self, rec_motion, gt_motion):
        rec, gt = _rows(rec_motion, 322, 'rec_motion')[:M2D_MAX_FRAMES], _rows(gt_motion, 322, 'gt_motion')     # :243
        if rec.shape[0] != gt.shape[0]:
            raise ValueError(f'the sample holds {rec.shape[0]} frames, the ground truth {gt.shape[0]} (m2d_test.py:246)')
        ev, embed = self.evaluator_model, _embed_device if self.on_device else _embed
        self.emb['pred'].append(embed(ev, rec))
        self.emb['gt'].append(embed(ev, gt))
        self.emb['hand_pred'].append(embed(ev, m2d_hand_only_motion(rec)))
        self.emb['hand_gt'].append(embed(ev, m2d_hand_only_motion(gt)))

    def summary(self):
        if len(self.emb['pred']) < 2:
            raise ValueError('the diversity needs at least two sequences')
        cat, fid = _tables(self.emb, self.on_device)
        times = cat['pred'].shape[0] - 1
        return {'FID(Whole Body) score': fid(cat['gt'], cat['pred']),
                'FID (Hands) score': fid(cat['hand_gt'], cat['hand_pred']),
                'Diversity score': (float(embmetrics.diversity(cat['pred'], times).item()) if self.on_device else
                                    calculate_diversity(cat['pred'], diversity_times=times, emb_scale=1.0, norm_scale=1.0))}
