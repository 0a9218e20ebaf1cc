"""The audio condition of the speech-to-gesture configs restated in numpy: the ``onset+amplitude`` representation
(``audio_rep`` of the EMAGE / BEAT2 data loader) that the S2G WavEncoder reads, float32 [N, 2].  ``csrc/mc_audiocond.hip`` and
``motioncraft_amd.speech.AudioCondition`` are pinned to this file, bit for bit: a maximum of float32 magnitudes has no rounding.

  column 0  the amplitude envelope: e[i] = max |y[i .. i + window - 1]| for the N - window + 1 FULL windows, then the last value
            repeated window - 1 times to length N.  The tail is a repeat, not a window that shrinks at the end of the clip.
  column 1  zeros with ones at the onset FRAME indices (hop 512), written into the sample-indexed column as they are: the reference
            indexes its per-sample array with what ``onset_detect(units='frames')`` returns, and the model was trained on that.

``envelope`` takes one ``np.maximum`` per window offset; ``envelope_loops`` is the double loop it is checked against, and
``envelope_shrinking`` is the definition this is NOT.  ``window_rows`` gives the rows of the condition each window of the S2G test
loop reads (``tools/s2g_test.py:144-155``).
"""
import numpy as np

WINDOW = 1024
SAMPLES_PER_FRAME = 16000 // 30


def envelope(y, window=WINDOW):
    """float32 [N] -> float32 [N]"""
    a = np.abs(np.asarray(y, np.float32))
    n = a.size
    if not 1 <= window <= n:
        raise ValueError(f'window {window} over {n} samples')
    full = a[:n - window + 1].copy()
    for k in range(1, window):
        np.maximum(full, a[k:k + n - window + 1], out=full)
    return np.concatenate([full, np.full(window - 1, full[-1], np.float32)])


def envelope_loops(y, window):
    a = [abs(float(v)) for v in np.asarray(y, np.float32)]
    n = len(a)
    out = []
    for i in range(n):
        s = min(i, n - window)
        m = a[s]
        for k in range(1, window):
            m = max(m, a[s + k])
        out.append(m)
    return np.array(out, np.float32)


def envelope_shrinking(y, window):
    """what the tail would be if the window were cut at the end of the clip; the condition does NOT do this"""
    a = np.abs(np.asarray(y, np.float32))
    return np.array([a[i:i + window].max() for i in range(a.size)], np.float32)


def condition(y, onset_frames, window=WINDOW):
    """y [N], onset frame indices -> float32 [N, 2]"""
    y = np.asarray(y, np.float32)
    onset = np.zeros(y.size, np.float32)
    onset[np.asarray(onset_frames, np.int64)] = 1.0
    return np.stack([envelope(y, window), onset], axis=1)


def window_rows(n_frames, motion_length, pre_frames, rows_per_frame=SAMPLES_PER_FRAME):
    """[(lo, hi)]: the rows of the condition that each window of an n_frames sequence reads, in the form the S2G test loop indexes its
    audio with: window i starts i * stride frames in and is stride + pre_frames frames long, stride = motion_length - pre_frames"""
    stride = motion_length - pre_frames
    per_window = rows_per_frame * stride
    return [(i * per_window, (i + 1) * per_window + rows_per_frame * pre_frames) for i in range((n_frames - pre_frames) // stride)]
