"""Seeded inputs of golden_baselines*.npz (tests/golden/make_golden_baselines.py): the generator and
the tests both build them from here, so only the reference's outputs are stored.

Every set is tie-free (a random permutation of evenly spaced log-magnitudes between log(1e-8) and
0): numpy's default argsort, which the reference's max-K selections use, is not stable, so its order
among equal values is not a contract.  Tie order is pinned against pca_subsample_points instead."""
import numpy as np

FB_FRAMES = 64          # frames of the shipped FB (F = 1025)
CNN_CHUNKS = 16         # chunks of the shipped CNN_temp (Nt = 10, Nf = 512)
FB_DIMS, CNN_DIMS, NT, NF, NCLASS = [1025, 513, 256], [512, 256, 100], 10, 512, 10
MAXK_K = {"fb": [1, 51, 501, 1025], "cnn": [1, 51, 501, 5120]}
MAXK_SETS = 4           # sets whose max-K items are stored
FB_PARTS = 3            # the FB state_dict is stored as a flat vector split over this many files
FB_CKPT = "FB(2021-04-26 17_45_43.476736)"
CNN_CKPT = "CNNTemp(2021-04-27 00_35_22.823854)"


def _tie_free(rng, n):
    return rng.permutation(np.linspace(np.log(1e-8), -0.25, n)).astype(np.float32)


def fb_frames():
    """float32 [64, 1025]: FB input frames (batch-major, as the reference's loader stacks them)."""
    rng = np.random.Generator(np.random.PCG64(2031))
    return np.stack([_tie_free(rng, FB_DIMS[0]) for _ in range(FB_FRAMES)])


def cnn_chunks():
    """float32 [16, 10, 512]: CNN_temp input chunks [Nt, Nf] (the reference's item layout)."""
    rng = np.random.Generator(np.random.PCG64(2032))
    return np.stack([_tie_free(rng, NT * NF).reshape(NT, NF) for _ in range(CNN_CHUNKS)])
