"""pca_pma_attention and pca_select_points on the device.

Block level: every case of golden_attn*.npz (tests/golden/make_golden_attn.py: the reference's own `A`, in
float32 and float64, on peaked maps) against A64.  The error of a row is max_n |A_dev - A64| / max_n A64 and
the bar is 8 x err_ref of the case, err_ref being the same figure for the reference's float32 `A`: the device
sums X . (Wk^T q) where the reference sums (X Wk^T) . q, both float32 sums of the same length.  Every figure is
printed before it is asserted (run with -s to read them).

Shapes no fixture holds (a width that is no multiple of 4, more than 64 rows, a row of 16384 keys) are compared
with the float64 restatement tests/attn_ref.py under a bound worked out from the inputs (``_score_bound``)."""
import ctypes as C
import functools
import os

import numpy as np
import pytest
import torch

from conftest import GOLDEN, Golden
from util import T

import attn_ref
import inputs_attn as ga

pytestmark = pytest.mark.gpu

BAR = 8.0
BLOCK = [c[0] for c in ga.BLOCK_CASES]


@pytest.fixture(scope="module")
def dev():
    return torch.device("cuda", 0)


@functools.lru_cache(maxsize=None)
def _golden(name):
    return np.load(os.path.join(GOLDEN, name), allow_pickle=False)


@functools.lru_cache(maxsize=None)
def _case(name):
    """(S, X, (wq, bq, wk, bk), h, golden file, key prefix, (src, lengths)) of a fixture case, host arrays."""
    if name in ga.SHIPPED:
        prefix, din, B, N, seed, mid = ga.SHIPPED[name]
        a = ga.SHIPPED_ARCH
        sd = Golden("golden_ckpt.npz").sub(prefix)
        Xb = attn_ref.shipped_block_input(ga.shipped_input(name), sd, a["h"])
        p = tuple(sd["dec.0.mab." + n] for n in ("fc_q.weight", "fc_q.bias", "fc_k.weight", "fc_k.bias"))
        return sd["dec.0.S"][0], Xb, p, a["h"], _golden(f"golden_attn_{name}.npz"), "", \
            ga.lengths_variant(N, mid)
    g = _golden("golden_attn.npz")
    _, d, h, N, k = ga.BLOCK_CASES[BLOCK.index(name)]
    c = ga.block_case(name, float(g[f"block/{name}/gain"]))
    return c["S"], c["X"], (c["wq"], c["bq"], c["wk"], c["bk"]), h, g, f"block/{name}/", \
        ga.lengths_variant(N)


def _run(dev, S, X, p, h, lengths=None):
    import pca_hip
    kl = None if lengths is None else torch.as_tensor(lengths, dtype=torch.int32)
    attn, key = pca_hip.pma_attention(T(S, dev), T(X, dev), [T(a, dev) for a in p], h, kl, want_key=True)
    torch.cuda.synchronize()
    return attn.cpu().numpy(), key.cpu().numpy()


def _structure(attn, key, lengths=None):
    """Rows sum to 1 within n 2^-23 over their n valid keys, one key gives exactly 1, everything beyond
    lengths[b] is an exact zero, and key is the fixed-order float32 mean of attn, bit for bit."""
    B, k, h, N = attn.shape
    assert attn.dtype == np.float32 and np.all(np.isfinite(attn)) and np.all(attn >= 0)
    for b in range(B):
        n = N if lengths is None else int(lengths[b])
        sums = attn[b, :, :, :n].astype(np.float64).sum(-1)
        dev1 = float(np.abs(sums - 1.0).max())
        assert dev1 <= n * 2.0 ** -23, (b, n, dev1)
        if n == 1:
            assert np.all(attn[b, :, :, 0] == 1.0)
        assert np.all(attn[b, :, :, n:] == 0.0) and np.all(key[b, n:] == 0.0)
        assert not np.any(np.signbit(attn[b, :, :, n:]))
    assert np.array_equal(key.view(np.uint32), attn_ref.key_of(attn).view(np.uint32))


@pytest.mark.parametrize("name", BLOCK + ["fst", "tst"])
def test_against_the_reference_map(dev, name):
    S, X, p, h, g, pre, _ = _case(name)
    attn, key = _run(dev, S, X, p, h)
    A64, err_ref = g[pre + "A64"], float(g[pre + "err_ref"])
    err = attn_ref.row_err(attn, A64)
    print(f"\n{name}: row error {err:.3e}, err_ref {err_ref:.3e}, ratio {err / err_ref if err_ref else 0:.2f}"
          f", peak A N {A64.max() * A64.shape[-1]:.0f}")
    _structure(attn, key)
    attn2, key2 = _run(dev, S, X, p, h)                        # the same call, the same bits
    assert np.array_equal(attn.view(np.uint32), attn2.view(np.uint32))
    assert np.array_equal(key.view(np.uint32), key2.view(np.uint32))
    assert err <= BAR * err_ref, (name, err, err_ref)


@pytest.mark.parametrize("name", BLOCK + ["fst", "tst"])
def test_lengths_match_the_truncated_sets(dev, name):
    S, X, p, h, g, pre, (src, lens) = _case(name)
    N = X.shape[1]
    assert np.array_equal(lens, g[pre + "len/lengths"])
    Xl = X[src].copy()
    rng = np.random.Generator(np.random.PCG64(99))
    for b, n in enumerate(lens):                               # padding rows: finite garbage, not zeros
        Xl[b, n:] = (1.0e3 * rng.standard_normal((N - n, X.shape[2]))).astype(np.float32)
    attn, key = _run(dev, S, Xl, p, h, lens)
    _structure(attn, key, lens)
    errs = g[pre + "len/err_ref"]
    for b, n in enumerate(lens):
        if n == N:
            ref = g[pre + "A64"][src[b]]
        elif n == 1:
            ref = np.ones((attn.shape[1], attn.shape[2], 1))
        else:
            ref = g[pre + f"len/A64_{b}"]
        err = attn_ref.row_err(attn[b, :, :, :n], ref)
        print(f"\n{name} set {b} length {n}: row error {err:.3e}, err_ref {errs[b]:.3e}, "
              f"ratio {err / errs[b] if errs[b] else 0:.2f}")
        assert err <= BAR * float(errs[b]), (name, b, n, err, float(errs[b]))


# ---- shapes outside the fixtures, against the float64 restatement ----------------------------------------
def _score_bound(S, X, p, h, chain):
    """A bound on the row error of the device map from float32 rounding alone.  score = X . u + c is a
    float32 sum of `chain` + 3 additions per partial sum (4 partial sums joined pairwise on the vector path,
    one on the scalar path), u and c are rounded once and the query once: |d score| <= (chain + 6) 2^-24
    sum_c |x_c u_c| (+ the same factor on |c|), to first order.  An error e of the scores moves a softmax
    value by at most 2 e relative to it; the exponentials, the sums of the tiles and the division add a few
    2^-24 each, 16 2^-24 together is generous.  Evaluated on the inputs in float64."""
    wq, bq, wk, bk = (np.asarray(a, np.float64) for a in p)
    d = wq.shape[0]
    dh = d // h
    q = np.asarray(S, np.float64) @ wq.T + bq                              # [k, d]
    worst = 0.0
    for s in range(q.shape[0]):
        for j in range(h):
            sl = slice(j * dh, (j + 1) * dh)
            u = q[s, sl] @ wk[sl] / np.sqrt(d)
            c = abs(q[s, sl] @ bk[sl]) / np.sqrt(d)
            worst = max(worst, float((np.abs(np.asarray(X, np.float64)) @ np.abs(u)).max() + c))
    return 2.0 * (chain + 6) * 2.0 ** -24 * worst + 16 * 2.0 ** -24


@pytest.mark.parametrize("d,h,k,N,B,gain", [
    (6, 2, 3, 70, 3, 4.0),         # d % 4 != 0: the scalar path, two tiles, an odd tail
    (64, 8, 9, 130, 2, 4.0),       # 72 rows: more than one pass of the normalising launch, uneven waves
    (256, 8, 1, 16384, 1, 8.0),    # a row no LDS could hold
    (12, 3, 1, 64, 2, 4.0),        # exactly one full tile
])
def test_other_shapes_against_float64(dev, d, h, k, N, B, gain):
    rng = np.random.Generator(np.random.PCG64(1000 + d + N))
    lim = 1.0 / np.sqrt(d)
    S = (gain * rng.uniform(-1, 1, (k, d)) * np.sqrt(6.0 / (k + d))).astype(np.float32)
    p = tuple(a.astype(np.float32) for a in (rng.uniform(-lim, lim, (d, d)), rng.uniform(-lim, lim, d),
                                             gain * rng.uniform(-lim, lim, (d, d)),
                                             rng.uniform(-lim, lim, d)))
    X = rng.standard_normal((B, N, d)).astype(np.float32)
    lens = None if B == 1 else np.array([N, 1, N // 2 + 3][:B], dtype=np.int32)
    attn, key = _run(dev, S, X, p, h, lens)
    _structure(attn, key, lens)
    ref = attn_ref.pma_attention(S, X, *p, h, lengths=lens)
    bound = _score_bound(S, X, p, h, d // 4 if d % 4 == 0 else d)
    for b in range(B):
        n = N if lens is None else int(lens[b])
        err = attn_ref.row_err(attn[b, :, :, :n], ref[b, :, :, :n])
        print(f"\nd={d} h={h} k={k} N={N} set {b} (length {n}): row error {err:.3e}, bound {bound:.3e}, "
              f"peak A n {ref[b].max() * n:.0f}")
        assert err <= bound, (b, err, bound)


def test_graph_replay_gives_the_eager_bits(dev):
    import pca_hip
    from pca_hip import _lib
    S, X, p, h, g, pre, _ = _case("d64h8N513k2")
    eager, eager_key = _run(dev, S, X, p, h)
    B, N, d = X.shape
    k = S.shape[0]
    L = pca_hip.lib()
    Sd, Xd = T(S, dev), T(X, dev)
    pd = [T(a, dev) for a in p]
    shape = _lib.MabShape(B, k, N, d, d, d, h, 1, _lib.MODE_BF16, 0, 0, 0, 0, 0)   # mode: accepted, ignored
    ws = torch.empty(L.pca_pma_attention_ws_bytes(C.byref(shape)), dtype=torch.uint8, device=dev)
    attn = torch.empty((B, k, h, N), dtype=torch.float32, device=dev)
    key = torch.empty((B, N), dtype=torch.float32, device=dev)
    pp = _lib.MabParams(*([a.data_ptr() for a in pd] + [None] * 8))

    def call(stream):
        _lib.check(L.pca_pma_attention(C.byref(shape), Sd.data_ptr(), Xd.data_ptr(), C.byref(pp),
                                       attn.data_ptr(), key.data_ptr(), ws.data_ptr(),
                                       C.c_void_p(stream.cuda_stream)), "pca_pma_attention")

    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        call(side)                                              # warm-up outside the capture
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        call(torch.cuda.current_stream())
    for _ in range(2):
        attn.fill_(7.0)
        key.fill_(7.0)
        graph.replay()
        torch.cuda.synchronize()
        assert np.array_equal(attn.cpu().numpy().view(np.uint32), eager.view(np.uint32))
        assert np.array_equal(key.cpu().numpy().view(np.uint32), eager_key.view(np.uint32))
    # the key alone: attn is required, key is not
    _lib.check(L.pca_pma_attention(C.byref(shape), Sd.data_ptr(), Xd.data_ptr(), C.byref(pp), attn.data_ptr(),
                                   None, ws.data_ptr(), None), "pca_pma_attention")
    torch.cuda.synchronize()
    assert np.array_equal(attn.cpu().numpy().view(np.uint32), eager.view(np.uint32))


# ---- pca_select_points -----------------------------------------------------------------------------------
@pytest.mark.parametrize("din", [2, 3])
@pytest.mark.parametrize("N", [7, 1025, 5120, 16384])
def test_select_points_order(dev, N, din):
    import pca_hip
    rng = np.random.Generator(np.random.PCG64(50 + N + din))
    d, h, B = 8, 2, 3
    # device-made keys: the mean pooling attention of a small block over N keys
    S = (4.0 * rng.uniform(-1, 1, (1, d))).astype(np.float32)
    p = [rng.uniform(-1, 1, s).astype(np.float32) for s in ((d, d), (d,), (d, d), (d,))]
    _, key = pca_hip.pma_attention(T(S, dev), T(rng.standard_normal((B, N, d)).astype(np.float32), dev),
                                   [T(a, dev) for a in p], h, want_key=True)
    # planted ties, +-0, a NaN
    key[0, N // 2] = key[0, 1]
    key[0, N - 1] = key[0, 1]
    key[1, 0] = 0.0
    key[1, N - 2] = -0.0
    key[1, N // 3] = 0.0
    key[2, N // 2] = float("nan")
    key[2, :3] = key[2, 5]
    kh = key.cpu().numpy()
    X = rng.standard_normal((B, N, din)).astype(np.float32)
    Xd = T(X, dev)
    for K in sorted({1, max(1, N // 10), N}):
        for lens in (None, np.array([N, max(1, K // 2), max(1, N - 1)], dtype=np.int32)):   # one shorter than K
            ld = None if lens is None else T(lens, dev)
            out, sel = pca_hip.select_points(Xd, key, K, ld)
            torch.cuda.synchronize()
            out, sel = out.cpu().numpy(), sel.cpu().numpy()
            for b in range(B):
                want = attn_ref.desc_order(kh[b], None if lens is None else lens[b])[:K]
                assert np.array_equal(sel[b], want), (N, din, K, b, lens is not None)
                assert np.array_equal(out[b].view(np.uint32), X[b, want].view(np.uint32))
    o2 = torch.empty((B, 1, din), dtype=torch.float32, device=dev)
    s2 = torch.empty((B, 1), dtype=torch.int32, device=dev)
    r = pca_hip.select_points(Xd, key, 1, out=o2, sel=s2)
    assert r[0] is o2 and r[1] is s2
    with pytest.raises(pca_hip.PcaHipError):
        pca_hip.select_points(Xd, key, N + 1)
