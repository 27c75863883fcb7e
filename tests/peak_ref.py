"""numpy restatement of pca_peak_points (include/pca_hip.h): plain loops, fp32 comparisons, fp64 refinement,
a stable argsort of the negated values over the mask.  Shared by the host and the GPU tests."""
import numpy as np


def peak_mask(v, F, Tv, radius_f=1, radius_t=0, rel_floor=np.inf, abs_floor=-np.inf):
    """bool [Tv * F]: which points of one set (fp32 values v, point p = t * F + f, Tv valid frames) are
    peaks."""
    v = np.asarray(v, dtype=np.float32)[:Tv * F]
    ok = ~np.isnan(v)
    vmax = np.max(v[ok]) if ok.any() else np.float32(-np.inf)
    rel_floor, abs_floor = np.float32(rel_floor), np.float32(abs_floor)
    with np.errstate(invalid="ignore"):
        rel_cut = np.float32(vmax - rel_floor)                 # one fp32 subtraction
    mask = np.zeros(Tv * F, dtype=bool)
    rel_on = bool(np.isfinite(rel_floor))
    # fp32 values as Python floats: the widening is exact, so every comparison below is the fp32 one
    v, rel_cut, abs_floor = v.tolist(), float(rel_cut), float(abs_floor)
    for t in range(Tv):
        for f in range(1, F - 1):
            p = t * F + f
            x = v[p]
            if x != x or not x >= abs_floor:
                continue
            if rel_on and not x >= rel_cut:
                continue
            win = True
            for tt in range(max(0, t - radius_t), min(Tv - 1, t + radius_t) + 1):
                for ff in range(max(0, f - radius_f), min(F - 1, f + radius_f) + 1):
                    q = tt * F + ff
                    if q == p:
                        continue
                    w = v[q]                                   # NaN: both comparisons are False, it loses
                    if w > x or (w == x and q < p):
                        win = False
                        break
                if not win:
                    break
            mask[p] = win
    return mask


def maxk_order(v):
    """Point order of max-K: values descending, -0 == +0, equal values in ascending index order, NaN last
    (a stable argsort of the negated values)."""
    return np.argsort(-(np.asarray(v, dtype=np.float32) + np.float32(0)), kind="stable")


def refine(a, b, c, xm, x0, xp):
    """(frequency, value) as float32 of the parabola through the fp32 values a, b, c at the fp32
    frequencies xm, x0, xp; the raw (x0, b) when a value is not finite."""
    if not (np.isfinite(a) and np.isfinite(b) and np.isfinite(c)):
        return np.float32(x0), np.float32(b)
    a, b, c, xm, x0, xp = (np.float64(z) for z in (a, b, c, xm, x0, xp))
    den = (a - b) + (c - b)
    delta = 0.5 * (a - c) / den
    step = (xp - x0) if delta >= 0.0 else (x0 - xm)
    return np.float32(x0 + delta * step), np.float32(b - 0.25 * (a - c) * delta)


def peak_points(X, F, Nt, K, radius_f=1, radius_t=0, rel_floor=np.inf, abs_floor=-np.inf, refine_on=True,
                lengths=None):
    """X float32 [B, F * Nt, din] -> dict(out [B, K, din] float32, lengths int32 [B], count int32 [B],
    sel int32 [B, K], mask bool [B, N])."""
    X = np.asarray(X, dtype=np.float32)
    B, N, din = X.shape
    assert N == F * Nt and F >= 3 and 1 <= K <= N and (din == 3 or Nt == 1)
    out = np.zeros((B, K, din), dtype=np.float32)
    sel = np.full((B, K), -1, dtype=np.int32)
    lens = np.zeros(B, dtype=np.int32)
    count = np.zeros(B, dtype=np.int32)
    masks = np.zeros((B, N), dtype=bool)
    for b in range(B):
        Tv = Nt if lengths is None else int(lengths[b]) // F
        v = X[b, :Tv * F, din - 1]
        mask = peak_mask(v, F, Tv, radius_f, radius_t, rel_floor, abs_floor)
        masks[b, :Tv * F] = mask
        order = maxk_order(v)
        peaks = order[mask[order]]
        count[b] = len(peaks)
        if len(peaks) == 0:                                    # the fallback row: max-K's first, unrefined
            out[b, 0] = X[b, order[0]]
            sel[b, 0] = order[0]
            lens[b] = 1
            continue
        n = min(len(peaks), K)
        lens[b] = n
        for q, p in enumerate(peaks[:n]):
            out[b, q] = X[b, p]
            sel[b, q] = p
            if refine_on:
                fh, vh = refine(v[p - 1], v[p], v[p + 1], X[b, p - 1, 0], X[b, p, 0], X[b, p + 1, 0])
                out[b, q, 0], out[b, q, din - 1] = fh, vh
    return dict(out=out, lengths=lens, count=count, sel=sel, mask=masks)
