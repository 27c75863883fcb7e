"""The point masks of pca_frame_points_masked restated in numpy (test helper, beside frame_aug_ref.py):
what a dense set becomes once the bands and stripes the mask meta reports are removed."""
import numpy as np

DROP, FLOOR = 0, 1


def masked_axes(mask_meta_row, n_bins, Nt):
    """(bins masked [n_bins] bool, frames masked [Nt] bool): the union of the intervals of a mask meta row,
    int32 [16] = (f0, w) x 4 bands, then (t0, w) x 4 stripes."""
    m = np.asarray(mask_meta_row).astype(np.int64).reshape(2, 4, 2)
    bins, frames = np.zeros(n_bins, dtype=bool), np.zeros(Nt, dtype=bool)
    for axis, extent, (which) in ((bins, n_bins, 0), (frames, Nt, 1)):
        for start, width in m[which]:
            assert 0 <= width and 0 <= start and start + width <= extent, (which, start, width, extent)
            axis[start:start + width] = True
    return bins, frames


def mask_rows(dense_rows, mask_meta_row, n_bins, Nt, mode, floor_value=None):
    """dense_rows [Nt * n_bins, din], point p = j * n_bins + f -> (rows [Nt * n_bins, din], length).
    mode DROP: the points whose bin lies in no band and whose frame lies in no stripe, in point order, then
    zeros; length = their number.  mode FLOOR: every row in place, the last column of a masked point set to
    ``floor_value``; length = Nt * n_bins."""
    dense_rows = np.asarray(dense_rows)
    assert dense_rows.shape[0] == Nt * n_bins and dense_rows.ndim == 2
    bins, frames = masked_axes(mask_meta_row, n_bins, Nt)
    gone = (frames[:, None] | bins[None, :]).reshape(-1)                # [Nt * n_bins], point order
    if mode == FLOOR:
        out = dense_rows.copy()
        out[gone, -1] = floor_value
        return out, dense_rows.shape[0]
    assert mode == DROP
    out = np.zeros_like(dense_rows)
    kept = dense_rows[~gone]
    out[:len(kept)] = kept
    return out, len(kept)
