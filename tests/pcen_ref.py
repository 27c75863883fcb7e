"""One slot of pca_frame_points_pcen restated in numpy (test helper, on tests/bands_ref.py): the header's
definition, given what ``meta`` says the slot drew.

    frame   bands_ref.frame_mag at clamp(first + (u - W) * hop, 0, L), u = 0 .. W + Nt - 1
    band    E[u][m] = sum_k W[m, k] * mag[k]^power with the dense W
    pcen    x = scale * E;  M[0] = x[0], M[u] = (1 - s) M[u-1] + s x[u];
            y = (bias + x * exp(-gain * log(eps + M)))^r - bias^r,  rows for u >= W

All of it in float64, rounded to float32 once at the end.  ``fp32_mag=True`` is the second mode: each bin's
magnitude formed as the kernel forms it (re and im scaled by 1 / norm and rounded to fp32, sqrtf(re^2 + im^2)
in fp32) - the distance between the two modes is what the device test sizes its bar with.  The spec's
parameters are the fp32 values the C struct holds."""
import numpy as np

from bands_ref import frame_mag
from frame_ref import hann_padded, reflect_index

FIELDS = ("context", "s", "gain", "bias", "r", "eps", "scale")


def spec(context, s, gain=0.98, bias=2.0, r=0.5, eps=1e-6, scale=1.0) -> dict:
    """The launch's PcaPcen as a dict, the floats rounded to fp32 as the struct holds them."""
    f = lambda v: float(np.float32(v))                                       # noqa: E731
    return dict(context=int(context), s=f(s), gain=f(gain), bias=f(bias), r=f(r), eps=f(eps), scale=f(scale))


def frame_mag32(wave: np.ndarray, centre: int, n_fft: int, win_length: int, gain, norm) -> np.ndarray:
    """frame_mag with the kernel's rounding of a bin: float64 [n_fft/2 + 1] holding fp32 magnitudes."""
    idx = reflect_index(int(centre) - n_fft // 2 + np.arange(n_fft, dtype=np.int64), len(wave))
    seg = wave[idx].astype(np.float64) * hann_padded(win_length, n_fft) * np.float64(gain)
    X = np.fft.rfft(seg) * (1.0 / np.float64(norm))
    re, im = X.real.astype(np.float32), X.imag.astype(np.float32)
    return np.sqrt(re * re + im * im, dtype=np.float32).astype(np.float64)


def energies(wave: np.ndarray, centres, n_fft: int, win_length: int, gain, norm, W: np.ndarray, power: int,
             fp32_mag: bool = False) -> np.ndarray:
    """float64 [len(centres), n_bands]: the band sums of the frames centred at ``centres``."""
    W = np.asarray(W, dtype=np.float64)
    assert W.shape[1] == n_fft // 2 + 1 and power in (1, 2)
    mag = frame_mag32 if fp32_mag else frame_mag
    return np.stack([W @ (mag(wave, c, n_fft, win_length, gain, norm) ** power) for c in centres])


def pcen(E: np.ndarray, p: dict) -> np.ndarray:
    """float64 [T - context, n_bands] from the band sums E [T, n_bands] of context + Nt frames."""
    E = np.asarray(E, dtype=np.float64)
    s, gain, bias, r, eps = (np.float64(p[k]) for k in ("s", "gain", "bias", "r", "eps"))
    x = np.float64(p["scale"]) * E
    M = np.empty_like(x)
    M[0] = x[0]
    for u in range(1, len(x)):
        M[u] = (1.0 - s) * M[u - 1] + s * x[u]
    y = np.power(bias + x * np.exp(-gain * np.log(eps + M)), r) - np.power(bias, r)
    return y[p["context"]:]


def steady_state(x, p: dict):
    """What a band of constant scaled energy x settles at: M = x."""
    x = np.asarray(x, dtype=np.float64)
    gain, bias, r, eps = (np.float64(p[k]) for k in ("gain", "bias", "r", "eps"))
    return np.power(bias + x / np.power(eps + x, gain), r) - np.power(bias, r)


def slot_centres(L: int, s_set: int, delta: int, Nt: int, hop: int, context: int) -> list:
    first = int(s_set) * Nt * hop + int(delta)
    return [min(max(first + (u - context) * hop, 0), L) for u in range(context + Nt)]


def slot_values(wave: np.ndarray, s_set: int, delta: int, Nt: int, hop: int, n_fft: int, win_length: int, gain,
                norm, W, power: int, p: dict, fp32_mag: bool = False) -> np.ndarray:
    """float64 [Nt, n_bands], not yet rounded: the value column of set ``s_set`` shifted by ``delta``."""
    centres = slot_centres(len(wave), s_set, delta, Nt, hop, p["context"])
    return pcen(energies(wave, centres, n_fft, win_length, gain, norm, W, power, fp32_mag), p)


def rows(values: np.ndarray, farr, tarr=None) -> np.ndarray:
    """float32 [Nt * n_bands, din]: point j * n_bands + m = (farr[m], [tarr[j],] value), rounded once."""
    Nt = values.shape[0]
    f32 = np.asarray(farr, dtype=np.float64).astype(np.float32)
    cols = [np.tile(f32, Nt)]
    if tarr is not None:
        cols.append(np.repeat(np.asarray(tarr, dtype=np.float64).astype(np.float32)[:Nt], len(f32)))
    return np.stack(cols + [values.astype(np.float32).reshape(-1)], axis=1)
