"""Time-frequency reassignment of one STFT frame restated in numpy (test helper, on frame_ref.py's
helpers): the rules of pca_frame_points_reassigned, in float64 with np.fft.fft.

    x[n]     the frame's samples (frame_ref's reflect rule) times the gain
    h[n]     frame_ref's periodic Hann of win_length samples, centred in n_fft and zero-padded
    dh[n]    (pi / w) sin(2 pi nw / w) inside the window, 0 outside: h's derivative per sample
    th[n]    (n - n_fft/2) h[n]
    db       -Im(X_dh conj(X_h)) / |X_h|^2 * n_fft / (2 pi)      bins
    dt        Re(X_th conj(X_h)) / |X_h|^2 / hop                 frames

The value column is NOT recomputed: the caller passes the float32 values of the plain launch (or of
frame_ref), so the floor decisions are taken on the same numbers on both sides."""
import numpy as np

from frame_ref import hann_padded, reflect_index

AXES = {"f": 1, "t": 2, "ft": 3}


def windows(win_length: int, n_fft: int):
    """(h, dh, th), float64 [n_fft] each."""
    h = hann_padded(win_length, n_fft)
    lpad = (n_fft - win_length) // 2
    dh = np.zeros(n_fft)
    dh[lpad:lpad + win_length] = (np.pi / win_length) * np.sin(
        2.0 * np.pi * np.arange(win_length) / win_length)
    th = (np.arange(n_fft, dtype=np.float64) - n_fft // 2) * h
    return h, dh, th


def shifts(wave: np.ndarray, centre: int, n_fft: int, win_length: int, gain, hop: int, n_bins: int):
    """(db [n_bins] in bins, dt [n_bins] in frames, p = |X_h|^2 [n_bins]) of the frame of ``wave`` centred
    at sample ``centre``; non-finite where p is 0."""
    L = len(wave)
    idx = reflect_index(int(centre) - n_fft // 2 + np.arange(n_fft, dtype=np.int64), L)
    x = wave[idx].astype(np.float64) * np.float64(gain)
    h, dh, th = windows(win_length, n_fft)
    Xh = np.fft.fft(x * h)[:n_bins]
    Xdh = np.fft.fft(x * dh)[:n_bins]
    Xth = np.fft.fft(x * th)[:n_bins]
    p = Xh.real ** 2 + Xh.imag ** 2
    with np.errstate(divide="ignore", invalid="ignore"):
        db = -np.imag(Xdh * np.conj(Xh)) / p * n_fft / (2.0 * np.pi)
        dt = np.real(Xth * np.conj(Xh)) / p / hop
    return db, dt, p


def reassign_frame(wave, centre, n_fft, win_length, gain, hop, values, farr, tarr, j, axes="f",
                   rel_floor=np.log(1e3), abs_floor=-np.inf, max_df=2.0, max_dt=1.0, strength=1.0):
    """Coordinates of frame ``j`` of a set: (f float32 [n_bins], t float32 [n_bins] or None, moved bool
    [n_bins], sdb float64 [n_bins]: the scaled frequency shift of the moved bins, 0 elsewhere).
    ``values`` float32 [n_bins]: the frame's value column; farr float32 [>= n_bins]; tarr float32 [Nt] or
    None.  Spec fields are taken to float32 first, as the C struct holds them."""
    values = np.asarray(values, dtype=np.float32)
    n_bins = values.size
    farr = np.asarray(farr, dtype=np.float32)
    bits = AXES[axes]
    rel_floor, abs_floor = np.float32(rel_floor), np.float32(abs_floor)
    max_df, max_dt, strength = (np.float64(np.float32(v)) for v in (max_df, max_dt, strength))
    db, dt, p = shifts(wave, centre, n_fft, win_length, gain, hop, n_bins)
    vmax = np.fmax.reduce(values, initial=np.float32(-np.inf))      # fmax: NaN loses
    with np.errstate(invalid="ignore"):
        thr = np.float32(vmax - rel_floor)            # one fp32 subtraction
        ok = (values >= thr) & (values >= abs_floor) & (p > 0) & np.isfinite(db) & np.isfinite(dt)
    f = farr[:n_bins].copy()
    t = None if tarr is None else np.full(n_bins, np.asarray(tarr, dtype=np.float32)[j], dtype=np.float32)
    sdb = np.zeros(n_bins)
    k = np.arange(n_bins, dtype=np.float64)
    if bits & 1:
        sh = np.where(ok, strength * np.clip(np.where(ok, db, 0.0), -max_df, max_df), 0.0)
        sdb = sh
        pos = np.clip(k + sh, 0.0, n_bins - 1.0)
        i = np.minimum(np.floor(pos).astype(np.int64), n_bins - 2)
        f0, f1 = farr[i].astype(np.float64), farr[i + 1].astype(np.float64)
        f = np.where(sh != 0.0, (f0 + (pos - i) * (f1 - f0)).astype(np.float32), f)
    if bits & 2:
        tarr = np.asarray(tarr, dtype=np.float32)
        Nt = tarr.size
        sh = np.where(ok, strength * np.clip(np.where(ok, dt, 0.0), -max_dt, max_dt), 0.0)
        pos = j + sh
        i = np.clip(np.floor(pos).astype(np.int64), 0, Nt - 2)
        t0, t1 = tarr[i].astype(np.float64), tarr[i + 1].astype(np.float64)
        t = np.where(sh != 0.0, (t0 + (pos - i) * (t1 - t0)).astype(np.float32), t)
    return f, t, ok, sdb


def first_centres(clips, set_off, idx, meta, values, n_fft, hop, Nt, jitter, norm_is_win=False):
    """The centre of frame 0 of every slot BEFORE the clamp into [0, L]: meta holds the clamped one, and a
    chunk's later frames sit ``hop`` apart from the unclamped one.  Where frame 0 of a clip's first chunk
    was clamped at 0, the shift is any of [-jitter, 0]: the one whose frame 1 (frame_ref) is nearest to the
    launched ``values`` [B, Nt * n_bins] is taken."""
    from frame_ref import frame_ref
    n_bins = values.shape[1] // Nt
    first = np.empty(len(idx), dtype=np.int64)
    for b, i in enumerate(idx):
        c, centre0, win = (int(v) for v in meta[b][:3])
        g = np.array([meta[b][3]], dtype=np.int32).view(np.float32)[0]
        nominal = (int(i) - set_off[c]) * Nt * hop
        first[b] = centre0
        if centre0 == 0 and nominal == 0 and Nt > 1 and jitter > 0:
            L = len(clips[c])
            norm = win if norm_is_win else n_fft
            errs = [np.abs(frame_ref(clips[c], min(max(d + hop, 0), L), n_fft, win, g, norm, n_bins)
                           - values[b, n_bins:2 * n_bins]).max() for d in range(-jitter, 1)]
            first[b] = int(np.argmin(errs)) - jitter
    return first


def reassign_batch(clips, first, meta, values, n_fft, hop, Nt, farr, tarr, **spec):
    """The coordinates of a whole batch from what ``meta`` [B, 4] (pca_frame_points' meta: clip, centre,
    window, bits of the gain) says was cut and ``first`` (first_centres) [B].  values float32
    [B, Nt * n_bins].  Returns (f [B, Nt * n_bins] float32, t likewise or None, moved bool, sdb float64: the
    scaled frequency shift in bins)."""
    B = len(first)
    n_bins = values.shape[1] // Nt
    fo = np.empty((B, Nt * n_bins), dtype=np.float32)
    to = None if tarr is None else np.empty((B, Nt * n_bins), dtype=np.float32)
    mv = np.zeros((B, Nt * n_bins), dtype=bool)
    sd = np.zeros((B, Nt * n_bins))
    for b in range(B):
        c, win = int(meta[b][0]), int(meta[b][2])
        g = np.array([meta[b][3]], dtype=np.int32).view(np.float32)[0]
        L = len(clips[c])
        for j in range(Nt):
            cj = min(max(int(first[b]) + j * hop, 0), L)
            sl = slice(j * n_bins, (j + 1) * n_bins)
            f, t, ok, sdb = reassign_frame(clips[c], cj, n_fft, win, g, hop, values[b, sl], farr, tarr, j,
                                           **spec)
            fo[b, sl], mv[b, sl], sd[b, sl] = f, ok, sdb
            if to is not None:
                to[b, sl] = t
    return fo, to, mv, sd
