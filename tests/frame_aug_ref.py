"""One augmented frame of pca_frame_points_ex restated in numpy (test helper, beside frame_ref.py).

    y        the clip resampled by ``ratio`` = 1 / speed: the resampling oracle without its level
             scaling, cut to int(L * ratio) samples and rounded to float32; ratio 1.0: the clip itself
    samples  y at centre - n_fft/2 + n under frame_ref's reflect rule on [0, len(y))
    mix      (float32)((float64)sample + (float64)alpha * (float64)bg[(start + n) mod len(bg)]): the
             background read circularly; alpha 0: the sample itself
    value    frame_ref's: log(1e-8 + |FFT(sample * window * gain)| / norm)
"""
import numpy as np

from frame_ref import hann_padded, reflect_index
from oracle import resample_oracle


def speed_clip(wave: np.ndarray, speed: float) -> np.ndarray:
    """float32 [int(L / speed)]: ``wave`` played at ``speed`` (ratio = 1.0 / speed, as the dataset has it)."""
    ratio = 1.0 / float(speed)
    if ratio == 1.0:
        return np.asarray(wave, dtype=np.float32)
    y = resample_oracle.resample(wave, float(speed), 1.0, scale=False)
    return y[:int(len(wave) * ratio)].astype(np.float32)


def speed_centre(nominal: int, ratio: float, Ly: int) -> int:
    """Centre in y's timeline of the frame whose centre in the clip's is ``nominal`` (before the clamp
    when it is frame 0 of a chunk: the chunk's other frames add j * hop to the unclamped value)."""
    q = int(nominal) if ratio == 1.0 else int(np.floor(float(nominal) * ratio + 0.5))
    return min(max(q, 0), Ly)


def aug_samples(y: np.ndarray, centre: int, n_fft: int, bg=None, start: int = 0, alpha=0.0) -> np.ndarray:
    """float32 [n_fft]: the samples of the frame centred at ``centre`` of y, mixed with ``bg``."""
    n = np.arange(n_fft, dtype=np.int64)
    v = np.asarray(y, dtype=np.float32)[reflect_index(int(centre) - n_fft // 2 + n, len(y))]
    alpha = np.float32(alpha)
    if alpha != 0:
        b = np.asarray(bg, dtype=np.float32)[(int(start) + n) % len(bg)]
        v = (v.astype(np.float64) + np.float64(alpha) * b.astype(np.float64)).astype(np.float32)
    return v


def frame_of_samples(samples: np.ndarray, win_length: int, gain, norm, n_bins: int) -> np.ndarray:
    """float32 [n_bins]: frame_ref's value of n_fft samples already cut."""
    n_fft = len(samples)
    seg = np.asarray(samples).astype(np.float64) * hann_padded(win_length, n_fft) * np.float64(gain)
    mag = np.abs(np.fft.rfft(seg)) / np.float64(norm)
    return np.log(1.0e-8 + mag)[:n_bins].astype(np.float32)


def frame_aug_ref(y, centre, n_fft, win_length, gain, norm, n_bins, bg=None, start=0, alpha=0.0):
    return frame_of_samples(aug_samples(y, centre, n_fft, bg, start, alpha), win_length, gain, norm,
                            n_bins)
