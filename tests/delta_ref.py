"""The delta columns of pca_frame_points_delta restated in numpy (test helper): the header's definition, on
the fp32 values of a slot's T = Nt + 2 Wt frames.

    Wt = width with "t" among the axes, else 0;  D = 2 (1 + 4 + .. + width^2)
    dt[j][m] = (float)((sum_n n * ((double)v[Wt+j+n][m] - (double)v[Wt+j-n][m])) / D)
    df[j][m] = (float)((sum_n n * ((double)v[Wt+j][min(m+n, F-1)] - (double)v[Wt+j][max(m-n, 0)])) / D)

n = 1 .. width ascending, the accumulator starting at 0.0, every step a float64 subtraction, a multiplication by
n and an addition, then one division and one rounding to float32.  Every step is a basic IEEE operation, so the
device's bits and these are the same.  The values themselves - the context rows - come from frame_ref.frame_ref
and bands_ref.band_values at ``slot_centres``."""
import numpy as np

AXES = ("t", "f", "tf")


def context(axes: str, width: int) -> int:
    assert axes in AXES and 1 <= int(width) <= 4
    return int(width) if "t" in axes else 0


def divisor(width: int) -> int:
    return 2 * sum(n * n for n in range(1, int(width) + 1))


def deltas(values: np.ndarray, Nt: int, axes: str, width: int) -> np.ndarray:
    """float32 [Nt, F, len(axes)] from the float32 values [Nt + 2 Wt, F] of a slot, dt before df."""
    values = np.asarray(values)
    assert values.dtype == np.float32 and values.ndim == 2
    Wt, W = context(axes, width), int(width)
    T, F = values.shape
    assert T == Nt + 2 * Wt, (T, Nt, Wt)
    v = values.astype(np.float64)
    D = np.float64(divisor(W))
    cols = []
    if "t" in axes:
        acc = np.zeros((Nt, F), dtype=np.float64)
        for n in range(1, W + 1):
            acc = acc + np.float64(n) * (v[Wt + n:Wt + n + Nt] - v[Wt - n:Wt - n + Nt])
        cols.append((acc / D).astype(np.float32))
    if "f" in axes:
        own = v[Wt:Wt + Nt]
        m = np.arange(F)
        acc = np.zeros((Nt, F), dtype=np.float64)
        for n in range(1, W + 1):
            acc = acc + np.float64(n) * (own[:, np.minimum(m + n, F - 1)] - own[:, np.maximum(m - n, 0)])
        cols.append((acc / D).astype(np.float32))
    return np.stack(cols, axis=2)


def slot_centres(L: int, s: int, delta: int, Nt: int, hop: int, Wt: int) -> list:
    """The centres of the Nt + 2 Wt frames of set ``s`` of a clip of L samples shifted by ``delta``."""
    first = int(s) * Nt * hop + int(delta)
    return [min(max(first + (u - Wt) * hop, 0), L) for u in range(Nt + 2 * Wt)]
