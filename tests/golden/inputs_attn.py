"""Seeded inputs of the pooling-attention fixtures (golden_attn*.npz), shared by make_golden_attn.py
(which ran the reference on them) and by the tests (which regenerate them instead of storing them)."""
import numpy as np

import inputs as gi

# ---- (a), (b): the shipped checkpoints (golden_ckpt.npz) on seeded log-magnitude sets -----------------
# tag -> (key prefix in golden_ckpt.npz, din, B, N, seed of inputs.pc_input, mid length of the lengths
# variant).  FST: points (linspace(0, .5, 1025), clip(N(-9, 3^2), -18.4, 0)).
SHIPPED = {
    "fst": ("fst/p/module.", 2, 4, 1025, 7101, 515),
    "tst": ("tst/p/module.", 3, 2, 5120, 7102, 1000),
}
SHIPPED_ARCH = dict(d=64, h=8, m=64, k=1)


def shipped_input(tag: str) -> np.ndarray:
    _, din, B, N, seed, _ = SHIPPED[tag]
    return gi.pc_input(seed, B, N, din)


# ---- (c): one pooling block with random weights ----------------------------------------------------------
BLOCK_DH = [(64, 8), (128, 4), (256, 8)]
BLOCK_N = [1, 7, 65, 513]
BLOCK_K = [1, 2]
BLOCK_B = 2
BLOCK_CASES = [(f"d{d}h{h}N{N}k{k}", d, h, N, k) for (d, h) in BLOCK_DH for N in BLOCK_N for k in BLOCK_K]


def block_case(name: str, gain: float = 1.0):
    """dict(S [k, d], wq, bq, wk, bk, X [BLOCK_B, N, d]) float32 of case ``name``; ``gain`` (a power of two
    found by the generator and stored in the fixture: the multiplication is exact) scales S and fc_k.weight
    until the map is peaked."""
    ci = [c[0] for c in BLOCK_CASES].index(name)
    _, d, h, N, k = BLOCK_CASES[ci]
    rng = np.random.Generator(np.random.PCG64(7200 + ci))
    lim = 1.0 / np.sqrt(d)
    out = dict(
        S=rng.uniform(-1, 1, size=(k, d)) * np.sqrt(6.0 / (k + d)),
        wq=rng.uniform(-lim, lim, size=(d, d)), bq=rng.uniform(-lim, lim, size=(d,)),
        wk=rng.uniform(-lim, lim, size=(d, d)), bk=rng.uniform(-lim, lim, size=(d,)),
        X=rng.standard_normal((BLOCK_B, N, d)))
    out = {n: v.astype(np.float32) for n, v in out.items()}
    g = np.float32(gain)
    out["S"] = out["S"] * g
    out["wk"] = out["wk"] * g
    return out


def lengths_variant(N: int, mid=None):
    """(source set of each batch slot, lengths) of the lengths variant: B = 3 with a full set, a set of
    one point and a set cut in the middle (all 1 at N = 1)."""
    mid = N // 2 + 1 if mid is None else mid
    return np.array([0, 1, 1]), np.array([N, 1, min(mid, N)], dtype=np.int32)
