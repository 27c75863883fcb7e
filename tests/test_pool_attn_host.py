"""Pooling attention and selection by an external key, without a GPU: the new symbols are declared,
exported and bound; the workspace queries and the argument errors answer on the host; the ABI version stays
2; and the numpy restatement the GPU tests lean on (tests/attn_ref.py) reproduces the reference's own maps
(golden_attn*.npz, tests/golden/make_golden_attn.py) to float64 accuracy."""
import ctypes
import os
import re

import numpy as np
import pytest

from conftest import GOLDEN, ROOT

import attn_ref
import inputs_attn as ga
import pca_hip
from pca_hip import _lib

NEW = ["pca_pma_attention_ws_bytes", "pca_pma_attention", "pca_select_points",
       "pca_st_pool_attention_ws_bytes", "pca_st_pool_attention"]


def _golden(name):
    return np.load(os.path.join(GOLDEN, name), allow_pickle=False)


def _pma_shape(B=4, k=1, N=1025, d=64, h=8, q_shared=1, dq=None, ln=0):
    return _lib.MabShape(B, k, N, d if dq is None else dq, d, d, h, q_shared, 0, 0, 0, 0, 0, ln)


# ---- the new symbols ------------------------------------------------------------------------------------
def test_new_symbols_are_declared_exported_and_bound():
    txt = open(os.path.join(ROOT, "include", "pca_hip.h")).read()
    txt = re.sub(r"/\*.*?\*/", "", txt, flags=re.S)
    handle = ctypes.CDLL(_lib.LIB_PATH)
    for s in NEW:
        assert re.search(r"\b" + s + r"\s*\(", txt), f"{s} not declared in pca_hip.h"
        assert hasattr(handle, s), f"{s} not exported"
        assert s in _lib.SIGNATURES, f"{s} not bound"
    for name in ("pma_attention", "select_points"):
        assert callable(getattr(pca_hip, name))
    import evalsweep
    import models
    import modules
    from pca_hip.trainer import STEngine
    assert callable(modules.PMA.attention) and callable(models.ST.attention)
    assert callable(STEngine.attention) and callable(evalsweep.attention_sweep)
    for fn in (modules.PMA.attention, models.ST.attention, STEngine.attention, pca_hip.pma_attention):
        assert "ot differentiable" in fn.__doc__


def test_abi_version_is_still_2():
    assert pca_hip.lib().pca_abi_version() == 2


# ---- queries and argument errors answer without a device --------------------------------------------------
def test_ws_queries_without_gpu():
    L = pca_hip.lib()
    s = _pma_shape()
    n = L.pca_pma_attention_ws_bytes(ctypes.byref(s))
    # u [8, 64] + c [8] + one (max, sum) pair per row and 64-point tile
    assert n >= 4 * (8 * 64 + 8 + 2 * 4 * 8 * 17) and n % 256 == 0
    big = _pma_shape(B=2, k=1, N=16384, d=256, h=8)           # h k = 8 rows of 16384: no LDS limit applies
    assert L.pca_pma_attention_ws_bytes(ctypes.byref(big)) > 0
    odd = _pma_shape(B=1, k=3, N=1, d=6, h=2)
    assert L.pca_pma_attention_ws_bytes(ctypes.byref(odd)) > 0
    for arch in (dict(B=128, N=1025, din=2), dict(B=16, N=5120, din=3)):
        for mode in (_lib.MODE_F32, _lib.MODE_BF16):
            cfg = _lib.StConfig(arch["B"], arch["N"], arch["din"], 64, 8, 64, 1, 10, mode)
            fwd = L.pca_st_ws_bytes(ctypes.byref(cfg), 0)
            both = L.pca_st_pool_attention_ws_bytes(ctypes.byref(cfg))
            s = _pma_shape(B=arch["B"], N=arch["N"])
            scratch = L.pca_pma_attention_ws_bytes(ctypes.byref(s))
            assert fwd > 0 and both >= fwd + scratch + 4 * arch["B"] * 8 * arch["N"]
    wide = _lib.StConfig(2, 64, 2, 512, 8, 16, 1, 10, 0)
    assert L.pca_st_pool_attention_ws_bytes(ctypes.byref(wide)) == 0


@pytest.mark.parametrize("kw,word", [
    (dict(q_shared=0), b"q_shared"),
    (dict(dq=32), b"dq="),
    (dict(ln=1), b"LayerNorm"),
    (dict(d=260, h=4), b"max 256"),
    (dict(d=64, h=7), b"divisible"),
    (dict(N=0), b"extent"),
])
def test_pma_attention_argument_errors(kw, word):
    L = pca_hip.lib()
    s = _pma_shape(**kw)
    assert L.pca_pma_attention_ws_bytes(ctypes.byref(s)) == 0
    pp = _lib.MabParams()
    rc = L.pca_pma_attention(ctypes.byref(s), None, None, ctypes.byref(pp), None, None, None, None)
    assert rc == -1 and word in L.pca_last_error(), L.pca_last_error()


def test_pma_attention_null_pointers_are_errors():
    L = pca_hip.lib()
    s = _pma_shape()
    pp = _lib.MabParams()
    assert L.pca_pma_attention(ctypes.byref(s), None, None, ctypes.byref(pp), None, None, None, None) == -1
    assert b"null" in L.pca_last_error()
    assert L.pca_pma_attention(None, None, None, None, None, None, None, None) == -1
    cfg = _lib.StConfig(2, 64, 2, 64, 8, 64, 1, 10, 0)
    assert L.pca_st_pool_attention(ctypes.byref(cfg), None, None, None, None, None, None, None, None) == -1
    assert b"null" in L.pca_last_error()


@pytest.mark.parametrize("B,N,din,K,word", [
    (2, 100, 2, 101, b"K=101"),          # K > N
    (2, 100, 2, 0, b"K=0"),
    (2, 16385, 3, 10, b"16384"),         # N > 16384
    (2, 100, 4, 10, b"din=4"),
    (0, 100, 2, 10, b"B=0"),
])
def test_select_points_argument_errors(B, N, din, K, word):
    L = pca_hip.lib()
    one = ctypes.c_void_p(256)            # non-null, never dereferenced: the arguments are refused first
    rc = L.pca_select_points(one, one, None, B, N, din, K, one, None, None)
    assert rc == -1 and word in L.pca_last_error(), L.pca_last_error()
    assert L.pca_select_points(None, one, None, 2, 100, 2, 10, one, None, None) == -1


# ---- the numpy restatement against the reference's own maps --------------------------------------------
def _check_restatement(S, Xb, p, h, g, pre, lens_src):
    A64 = g[pre + "A64"]
    mine = attn_ref.pma_attention(S, Xb, p["wq"], p["bq"], p["wk"], p["bk"], h)
    assert mine.shape == A64.shape
    assert attn_ref.row_err(mine, A64) <= 1e-10, pre
    # ... and measures the reference's float32 error as the fixture recorded it
    err = attn_ref.row_err(g[pre + "A"], mine)
    assert abs(err - float(g[pre + "err_ref"])) <= 1e-9 + 1e-3 * err, (pre, err, float(g[pre + "err_ref"]))
    np.testing.assert_allclose(g[pre + "A64"].sum(-1), 1.0, rtol=0, atol=1e-12)
    # lengths variant: the valid prefix is the truncated set's map, zeros beyond
    src, lens = lens_src
    assert np.array_equal(lens, g[pre + "len/lengths"])
    ml = attn_ref.pma_attention(S, Xb[src], p["wq"], p["bq"], p["wk"], p["bk"], h, lengths=lens)
    N = Xb.shape[1]
    for b, n in enumerate(lens):
        assert np.all(ml[b, :, :, n:] == 0.0)
        if n == N:
            ref = A64[src[b]]
        elif n == 1:
            ref = np.ones_like(ml[b, :, :, :1])
        else:
            ref = g[pre + f"len/A64_{b}"]
        assert attn_ref.row_err(ml[b, :, :, :n], ref) <= 1e-10, (pre, b)


@pytest.mark.parametrize("name", [c[0] for c in ga.BLOCK_CASES])
def test_restatement_reproduces_block_golden(name):
    g = _golden("golden_attn.npz")
    _, d, h, N, k = ga.BLOCK_CASES[[c[0] for c in ga.BLOCK_CASES].index(name)]
    c = ga.block_case(name, float(g[f"block/{name}/gain"]))
    A64 = g[f"block/{name}/A64"]
    assert A64.shape == (ga.BLOCK_B, k, h, N) and A64.dtype == np.float64
    if N >= 65:       # the fixture is peaked: a near-uniform softmax cannot stand in for it
        assert ((A64.max(-1) * N) >= 8).mean() >= 0.5
    _check_restatement(c["S"], c["X"], c, h, g, f"block/{name}/", ga.lengths_variant(N))


@pytest.mark.parametrize("tag", ["fst", "tst"])
def test_restatement_reproduces_shipped_golden(tag, golden_ckpt):
    g = _golden(f"golden_attn_{tag}.npz")
    prefix, din, B, N, seed, mid = ga.SHIPPED[tag]
    a = ga.SHIPPED_ARCH
    sd = golden_ckpt.sub(prefix)
    Xb = attn_ref.shipped_block_input(ga.shipped_input(tag), sd, a["h"])
    assert Xb.shape == (B, N, a["d"])
    A64 = g["A64"]
    assert A64.shape == (B, 1, a["h"], N)
    peak = A64.max(-1) * N
    assert (peak >= 16).any(axis=(0, 1)).sum() == 7           # 7 of 8 heads are peaked, one is uniform
    p = dict(wq=sd["dec.0.mab.fc_q.weight"], bq=sd["dec.0.mab.fc_q.bias"],
             wk=sd["dec.0.mab.fc_k.weight"], bk=sd["dec.0.mab.fc_k.bias"])
    _check_restatement(sd["dec.0.S"][0], Xb, p, a["h"], g, "", ga.lengths_variant(N, mid))
    assert float(g["err_enc"]) > 0 and g["logits"].shape == (B, 10)


def test_key_and_order_restatements():
    rng = np.random.Generator(np.random.PCG64(1))
    A = rng.random((2, 2, 3, 5)).astype(np.float32)
    key = attn_ref.key_of(A)
    assert key.dtype == np.float32 and key.shape == (2, 5)
    np.testing.assert_allclose(key, A.reshape(2, 6, 5).mean(1), rtol=1e-6)
    k = np.array([1.0, np.nan, 3.0, -0.0, 0.0, 3.0, -np.inf, 2.0], dtype=np.float32)
    assert attn_ref.desc_order(k).tolist() == [2, 5, 7, 0, 3, 4, 6, 1]
    assert attn_ref.desc_order(k, 6).tolist() == [2, 5, 0, 3, 4, 1, 6, 7]
    assert attn_ref.desc_order(k, 2).tolist() == [0, 1, 2, 3, 4, 5, 6, 7]
