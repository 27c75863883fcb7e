"""One slot of pca_frame_points_multires restated in numpy (test helper, on tests/frame_ref.py): the rows of
a multi-resolution set, given what the slot drew.

    anchor   first = s * span + delta
    frame    j of level r centred at clamp(first + offset_r + j * hop_r, 0, L), frame_ref's transform at
             n_fft_r with window clamp(win_lengths_r[wi], 1, n_fft_r), gain g, norm n_fft_r or the window
    rows     levels back to back in the order given; inside a level point j * n_bins + f =
             (farr[f], tarr[j], value), or (farr[f], value) when the levels carry no tarr

A level is a dict of n_fft, hop, n_bins, Nt, offset, farr, tarr (or None) and win_lengths."""
import numpy as np

from frame_ref import frame_ref


def multires_ref(wave: np.ndarray, s: int, delta: int, g, wi: int, levels, span: int,
                 norm_mode: int = 0) -> np.ndarray:
    """float32 [N, din]: set ``s`` of the clip ``wave`` shifted by ``delta`` samples."""
    L = len(wave)
    first = int(s) * int(span) + int(delta)
    rows = []
    for lv in levels:
        n_fft, hop, n_bins, Nt = (int(lv[k]) for k in ("n_fft", "hop", "n_bins", "Nt"))
        win = min(max(int(lv["win_lengths"][wi]), 1), n_fft)
        farr = np.asarray(lv["farr"], dtype=np.float64).astype(np.float32)[:n_bins]
        for j in range(Nt):
            centre = min(max(first + int(lv.get("offset", 0)) + j * hop, 0), L)
            val = frame_ref(wave, centre, n_fft, win, g, n_fft if norm_mode == 0 else win, n_bins)
            cols = [farr]
            if lv.get("tarr") is not None:
                t = np.asarray(lv["tarr"], dtype=np.float64).astype(np.float32)[j]
                cols.append(np.full(n_bins, t, dtype=np.float32))
            rows.append(np.stack(cols + [val], axis=1))
    return np.concatenate(rows, axis=0)
