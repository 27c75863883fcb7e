"""One slot of pca_frame_points_bands restated in numpy (test helper, on tests/frame_ref.py): the band values
of the frames a slot cut, given what ``meta`` says it drew, and the mel formulae written out independently of
pca_hip/ops.py.

    frame   frame_ref's samples, window and gain at the given centre; mag = |FFT| / norm, all n_fft/2 + 1 bins
    band    E_m = sum_k W[m, k] * mag[k]^power with the dense W
    value   log(amin + E_m)

All of it in float64, rounded to float32 once at the end."""
import math

import numpy as np

from frame_ref import hann_padded, reflect_index


def frame_mag(wave: np.ndarray, centre: int, n_fft: int, win_length: int, gain, norm) -> np.ndarray:
    """float64 [n_fft/2 + 1]: |FFT| / norm of the frame of ``wave`` centred at sample ``centre``."""
    idx = reflect_index(int(centre) - n_fft // 2 + np.arange(n_fft, dtype=np.int64), len(wave))
    seg = wave[idx].astype(np.float64) * hann_padded(win_length, n_fft) * np.float64(gain)
    return np.abs(np.fft.rfft(seg)) / np.float64(norm)


def band_values(wave: np.ndarray, centres, n_fft: int, win_length: int, gain, norm, W: np.ndarray,
                power: int, amin: float) -> np.ndarray:
    """float32 [len(centres), n_bands]: the value column of the frames centred at ``centres``."""
    W = np.asarray(W, dtype=np.float64)
    assert W.shape[1] == n_fft // 2 + 1 and power in (1, 2)
    rows = []
    for c in centres:
        p = frame_mag(wave, c, n_fft, win_length, gain, norm) ** power
        rows.append(np.log(np.float64(np.float32(amin)) + W @ p).astype(np.float32))
    return np.stack(rows)


def slot_rows(wave: np.ndarray, s: int, delta: int, Nt: int, hop: int, n_fft: int, win_length: int, gain,
              norm, W, power: int, amin: float, farr, tarr=None) -> np.ndarray:
    """float32 [Nt * n_bands, din]: set ``s`` of the clip shifted by ``delta``; frame j centred at
    clamp((s * Nt + j) * hop + delta, 0, L); point j * n_bands + m = (farr[m], [tarr[j],] value)."""
    L = len(wave)
    centres = [min(max((int(s) * Nt + j) * hop + int(delta), 0), L) for j in range(Nt)]
    val = band_values(wave, centres, n_fft, win_length, gain, norm, W, power, amin)
    f32 = np.asarray(farr, dtype=np.float64).astype(np.float32)
    cols = [np.tile(f32, Nt)]
    if tarr is not None:
        cols.append(np.repeat(np.asarray(tarr, dtype=np.float64).astype(np.float32)[:Nt], len(f32)))
    return np.stack(cols + [val.reshape(-1)], axis=1)


# ---- the mel formulae (Slaney's Auditory Toolbox scale and HTK's), loops and scalars on purpose -----------
def hz_to_mel(f: float, htk: bool = False) -> float:
    if htk:
        return 2595.0 * math.log10(1.0 + f / 700.0)
    if f < 1000.0:
        return f / (200.0 / 3.0)
    return 15.0 + math.log(f / 1000.0) / (math.log(6.4) / 27.0)


def mel_to_hz(m: float, htk: bool = False) -> float:
    if htk:
        return 700.0 * (10.0 ** (m / 2595.0) - 1.0)
    if m < 15.0:
        return m * (200.0 / 3.0)
    return 1000.0 * math.exp((m - 15.0) * (math.log(6.4) / 27.0))


def mel_points(fs: float, n_mels: int, fmin: float = 0.0, fmax=None, htk: bool = False) -> np.ndarray:
    """The n_mels + 2 band edges in Hz, equally spaced in mel."""
    fmax = fs / 2.0 if fmax is None else fmax
    lo, hi = hz_to_mel(fmin, htk), hz_to_mel(fmax, htk)
    return np.array([mel_to_hz(lo + (hi - lo) * i / (n_mels + 1), htk) for i in range(n_mels + 2)])


def mel_matrix(fs: float, n_fft: int, n_mels: int, fmin: float = 0.0, fmax=None, htk: bool = False,
               norm="slaney") -> np.ndarray:
    """float64 [n_mels, n_fft/2 + 1]: triangle i rises from p_i to p_i+1 and falls to p_i+2."""
    p = mel_points(fs, n_mels, fmin, fmax, htk)
    W = np.zeros((n_mels, n_fft // 2 + 1))
    for i in range(n_mels):
        for k in range(n_fft // 2 + 1):
            f = k * fs / n_fft
            W[i, k] = max(0.0, min((f - p[i]) / (p[i + 1] - p[i]), (p[i + 2] - f) / (p[i + 2] - p[i + 1])))
        if norm == "slaney":
            W[i] *= 2.0 / (p[i + 2] - p[i])
    return W
