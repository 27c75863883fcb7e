"""One STFT log-magnitude frame restated in numpy (test helper, like trim_ref.py): the frame
pca_frame_points cuts for a given centre, window length and gain.

    samples  centre - n_fft/2 + n, n < n_fft, of the clip; an index below 0 reflects to -index, one at
             or beyond L to 2 (L - 1) - index
    window   periodic Hann of win_length samples, centred in n_fft and zero-padded
    value    log(1e-8 + |FFT(sample * window * gain)| / norm), bins 0 .. n_bins - 1

All of it in float64, rounded to float32 at the end."""
import numpy as np


def reflect_index(i: np.ndarray, L: int) -> np.ndarray:
    i = np.where(i < 0, -i, i)
    i = np.where(i >= L, 2 * (L - 1) - i, i)
    return np.maximum(i, 0)


def hann_padded(win_length: int, n_fft: int) -> np.ndarray:
    win = np.zeros(n_fft)
    lpad = (n_fft - win_length) // 2
    win[lpad:lpad + win_length] = 0.5 - 0.5 * np.cos(2.0 * np.pi * np.arange(win_length) / win_length)
    return win


def frame_ref(wave: np.ndarray, centre: int, n_fft: int, win_length: int, gain, norm,
              n_bins: int) -> np.ndarray:
    """float32 [n_bins]: the frame of ``wave`` centred at sample ``centre``."""
    L = len(wave)
    idx = reflect_index(int(centre) - n_fft // 2 + np.arange(n_fft, dtype=np.int64), L)
    seg = wave[idx].astype(np.float64) * hann_padded(win_length, n_fft) * np.float64(gain)
    mag = np.abs(np.fft.rfft(seg)) / np.float64(norm)
    return np.log(1.0e-8 + mag)[:n_bins].astype(np.float32)
