"""Logits and pooling attention of a whole model in one call (pca_st_pool_attention, STEngine.attention),
the module route (ST.attention) and evalsweep.attention_sweep, on the shipped FST and 3ST weights.

F32 mode: the logits are pca_st_forward's bit for bit; the map meets golden_attn_{fst,tst}.npz under
8 x err_ref + err_enc, both from the fixture (err_ref: the reference's float32 pooling block against float64;
err_enc: what the reference's own float32 encoder adds - here the encoder output comes from the device).
BF16 mode has no reference: only structure (sums, zeros beyond lengths, determinism); its distance from the
F32 map is printed.  The sweep is checked as a composition: its per-K counts equal those recomputed from
STEngine.attention, select_points, STEngine.forward and argmax with the same sets per call."""
import json
import os

import numpy as np
import pytest
import torch

from conftest import GOLDEN, Golden
from util import T

import attn_ref
import inputs_attn as ga

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def dev():
    return torch.device("cuda", 0)


def _shipped_net(tag, dev):
    import models
    prefix, din = ga.SHIPPED[tag][0], ga.SHIPPED[tag][1]
    a = ga.SHIPPED_ARCH
    net = models.ST(dim_input=din, dim_hidden=a["d"], num_heads=a["h"], num_inds=a["m"])
    net.load_state_dict({k: T(v) for k, v in Golden("golden_ckpt.npz").sub(prefix).items()})
    return net.to(dev).eval()


def _structure(attn, key, lengths=None):
    B, k, h, N = attn.shape
    for b in range(B):
        n = N if lengths is None else int(lengths[b])
        sums = attn[b, :, :, :n].astype(np.float64).sum(-1)
        assert float(np.abs(sums - 1.0).max()) <= n * 2.0 ** -23, (b, n)
        assert np.all(attn[b, :, :, n:] == 0.0) and np.all(key[b, n:] == 0.0)
    assert np.array_equal(key.view(np.uint32), attn_ref.key_of(attn).view(np.uint32))


@pytest.mark.parametrize("tag", ["fst", "tst"])
def test_engine_attention_f32(dev, tag):
    from pca_hip import _lib
    from pca_hip.trainer import STEngine
    g = np.load(os.path.join(GOLDEN, f"golden_attn_{tag}.npz"))
    net = _shipped_net(tag, dev)
    X = T(ga.shipped_input(tag), dev)
    B, N, _ = X.shape
    eng = STEngine(net, B, N, _lib.MODE_F32, training=False)
    plain = eng.forward(X).clone()
    logits, attn, key = eng.attention(X)
    torch.cuda.synchronize()
    assert np.array_equal(logits.cpu().numpy().view(np.uint32), plain.cpu().numpy().view(np.uint32))
    assert eng.forward(X).equal(plain)                        # the larger workspace changes nothing
    a, kk = attn.cpu().numpy(), key.cpu().numpy()
    _structure(a, kk)
    bar = 8.0 * float(g["err_ref"]) + float(g["err_enc"])
    err = attn_ref.row_err(a, g["A64"])
    print(f"\n{tag}: engine map row error {err:.3e}, bar {bar:.3e} (8 x {float(g['err_ref']):.3e} + "
          f"{float(g['err_enc']):.3e})")
    # the module route: enc, PMA.attention, dec
    lm, am = net.attention(X)
    am = am.cpu().numpy()
    assert am.shape == a.shape
    both = attn_ref.row_err(am, a.astype(np.float64))
    print(f"{tag}: module route against the engine {both:.3e}, logits differ by "
          f"{float((lm - plain).abs().max()):.3e}")
    # the key alone and the logits alone
    l2, none_a, k2 = eng.attention(X, want_attn=False)
    assert none_a is None and k2.equal(key) and l2.equal(plain)
    l3, a3, none_k = eng.attention(X, want_key=False)
    assert none_k is None and a3.equal(attn)
    assert err <= bar, (tag, err, bar)
    assert both <= 2.0 * bar, (tag, both, bar)
    assert float((lm.reshape(plain.shape) - plain).abs().max()) <= 1e-3
    with pytest.raises(_lib.PcaHipError):
        STEngine(net, B, N, _lib.MODE_F32, training=True).attention(X)


@pytest.mark.parametrize("tag", ["fst", "tst"])
def test_engine_attention_bf16_structure(dev, tag):
    from pca_hip import _lib
    from pca_hip.trainer import STEngine
    net = _shipped_net(tag, dev)
    Xh = ga.shipped_input(tag)
    B, N, din = Xh.shape
    lens = np.array(([N, 1, N // 2 + 1, N - 1] * B)[:B], dtype=np.int32)
    rng = np.random.Generator(np.random.PCG64(5))
    for b, n in enumerate(lens):                               # padding rows: finite garbage
        Xh[b, n:] = rng.uniform(-20, 1, (N - n, din)).astype(np.float32)
    X, ld = T(Xh, dev), T(lens, dev)
    res = {}
    for mode in (_lib.MODE_BF16, _lib.MODE_F32):
        eng = STEngine(net, B, N, mode, training=False)
        plain = eng.forward(X, ld).clone()
        logits, attn, key = eng.attention(X, ld)
        a, kk = attn.cpu().numpy(), key.cpu().numpy()
        assert np.array_equal(logits.cpu().numpy().view(np.uint32), plain.cpu().numpy().view(np.uint32))
        _structure(a, kk, lens)
        _, attn2, key2 = eng.attention(X, ld)                  # the same call, the same bits
        assert np.array_equal(attn2.cpu().numpy().view(np.uint32), a.view(np.uint32))
        assert np.array_equal(key2.cpu().numpy().view(np.uint32), kk.view(np.uint32))
        res[mode] = a
    dist = attn_ref.row_err(res[_lib.MODE_BF16], res[_lib.MODE_F32].astype(np.float64))
    print(f"\n{tag}: bf16-mode map against the F32-mode map, row error {dist:.3e} (measured, not barred)")


def _corpus(tag):
    rng = np.random.Generator(np.random.PCG64(31 if tag == "fst" else 32))
    if tag == "fst":
        F, n = 1025, 64
        x = rng.normal(-9, 3, size=(F, n)).astype(np.float32)
        return x, rng.integers(0, 10, size=n), np.linspace(0, 44100 / 2, F) / 44100, None, \
            [1, 51, 501, 1025], 24
    F, Nt, n = 512, 10, 16
    x = rng.normal(-9, 3, size=(F, Nt, n)).astype(np.float32)
    return x, rng.integers(0, 10, size=n), np.linspace(0, 44100 / 2, F) / 44100, \
        np.linspace(0, (512 / 44100) * Nt, Nt), [1, 2551, 5120], 6


@pytest.mark.parametrize("tag", ["fst", "tst"])
def test_attention_sweep_is_the_composition(dev, tag, tmp_path):
    import evalsweep
    import pca_hip
    from pca_hip import _lib
    from pca_hip.trainer import STEngine
    net = _shipped_net(tag, dev)
    x, y, farr, tarr, list_K, cap = _corpus(tag)
    path = str(tmp_path / "attn.json")
    out = evalsweep.attention_sweep(net, x, y, farr, tarr, list_K=list_K, sets_per_call=cap,
                                    json_file=path)
    n = x.shape[-1]
    assert out["list_K"] == list_K and sorted(out["data"]) == sorted(list_K)
    back = json.load(open(path))                               # the reference's max-K dictionary shape
    assert back["list_K"] == list_K
    assert {int(k): v for k, v in back["data"].items()} == {k: list(v) for k, v in out["data"].items()}
    assert all(len(v) == 2 and v[1] == 0 for v in out["data"].values())
    # the same composition by hand, with the same sets per call
    xs, lab, f32, t32 = evalsweep._resident_sets(x, y, farr, tarr, dev)
    N = x.shape[0] if tarr is None else x.shape[0] * x.shape[1]
    din = 2 if tarr is None else 3
    full = (n // 8) * 8
    keys, sets = [], []
    for p0 in range(0, full, cap):
        b = min(cap, full - p0)
        pos = torch.arange(p0, p0 + b, device=dev)
        X = torch.empty((b, N, din), dtype=torch.float32, device=dev)
        evalsweep._pack_sets(xs, f32, t32, pos, X)
        _, _, key = STEngine(net, b, N, _lib.MODE_F32, training=False).attention(X, want_attn=False)
        keys.append(key.clone())
        sets.append(X)
    for K in list_K:
        correct = 0
        for i, p0 in enumerate(range(0, full, cap)):
            b = min(cap, full - p0)
            sub, _ = pca_hip.select_points(sets[i], keys[i], K)
            logits = STEngine(net, b, K, _lib.MODE_F32, training=False).forward(sub)
            correct += int((logits.argmax(1) == lab[p0:p0 + b]).sum())
        assert out["data"][K] == [correct / full, 0], (tag, K, out["data"][K], correct)
    # K = N keeps every point: the accuracy of the full sets, whatever the order
    assert np.isfinite(out["data"][list_K[-1]][0])
