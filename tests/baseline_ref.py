"""Float64 numpy restatement of the two baselines' eval-mode forwards (Code/models.py:47-119) and
loaders of their golden parameters (golden_base.npz, golden_baselines*.npz)."""
import os

import numpy as np

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


def _leaky(x):
    return np.where(x > 0, x, 0.01 * x)


def _mlp(h, lins):
    for i, (w, b) in enumerate(lins):
        h = h @ w.astype(np.float64).T + b.astype(np.float64)
        if i + 1 < len(lins):
            h = _leaky(h)
    return h


def _pairs(params):
    v = list(params.values())
    return [(v[i], v[i + 1]) for i in range(0, len(v), 2)]


def fb_forward64(x, params):
    """x [B, F] -> softmax probabilities [B, C]; params: FB state_dict (ordered)."""
    z = _mlp(np.asarray(x, np.float64), _pairs(params))
    e = np.exp(z - z.max(1, keepdims=True))
    return e / e.sum(1, keepdims=True)


def cnn_forward64(x, params):
    """x [B, Nt, Nf] -> logits [B, C]; params: CNN_classifier state_dict (ordered)."""
    v = list(params.values())
    w = v[0].astype(np.float64)[0, 0]                     # [Nt, kw]
    Nt, kw = w.shape
    x = np.asarray(x, np.float64)
    L0 = x.shape[2] - kw + 1
    y = np.full((x.shape[0], L0), float(v[1][0]))
    for k in range(kw):
        y += np.einsum("btl,t->bl", x[:, :, k:k + L0], w[:, k])
    return _mlp(y, _pairs(dict(enumerate(v[2:]))))


def _unflatten(flat, keys, shapes):
    out, off = {}, 0
    for k, s in zip(keys, shapes):
        shape = tuple(int(a) for a in str(s).split(","))
        n = int(np.prod(shape))
        out[str(k)] = flat[off:off + n].reshape(shape)
        off += n
    assert off == flat.size
    return out


def shipped_params(tag):
    """The shipped checkpoint's state_dict (ordered dict of float32 arrays): tag 'fb' or 'cnntemp'."""
    base = np.load(os.path.join(GOLDEN, "golden_base.npz"))
    if tag == "fb":
        flat = np.concatenate([np.load(os.path.join(GOLDEN, f"golden_baselines_fb{i}.npz"))["flat"]
                               for i in range(3)])
    else:
        flat = np.load(os.path.join(GOLDEN, "golden_baselines.npz"))["cnn/flat"]
    return _unflatten(flat, base[f"shipped/{tag}/keys"], base[f"shipped/{tag}/shapes"])


def small_params(tag):
    """The small reference models of golden_base.npz: tag 'ff' or 'cnn'."""
    z = np.load(os.path.join(GOLDEN, "golden_base.npz"))
    pre = f"{tag}/p/"
    return {k[len(pre):]: z[k] for k in z.files if k.startswith(pre)}


def maxK_replace64(x, K):
    """Zero-filled max-K rows: x [S, n] -> [S, n] keeping each row's K largest values (stable
    descending order: equal values keep ascending position; Code/utils.py:86-96 and
    Code/dataset.py:101-135 on tie-free rows)."""
    x = np.asarray(x)
    out = np.zeros_like(x)
    for s in range(x.shape[0]):
        keep = np.argsort(-x[s], kind="stable")[:K]
        out[s, keep] = x[s, keep]
    return out
