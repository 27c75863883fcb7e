"""numpy restatement of the pooling attention and of the selection order (test infrastructure).

``pma_attention`` follows set_transformer-master/modules.py:20-28 as PMA reaches it, in the reference's own
order of operations (project the keys, split the heads, scores, softmax) and in float64 unless told
otherwise; tests/test_pool_attn_host.py pins it against golden_attn*.npz, the GPU tests lean on it for
shapes the fixtures do not hold.  The layout is the library's: A[B, k, h, N]; the reference's own
[h * B, k, N] row (j * B + b, s) is A[b, s, j, :] (``from_reference_layout``)."""
import numpy as np


def _softmax(x):
    x = x - x.max(axis=-1, keepdims=True)
    e = np.exp(x)
    return e / e.sum(axis=-1, keepdims=True)


def from_reference_layout(A_ref, B, h):
    """[h * B, k, N] (torch.cat of the head split along dim 0) -> [B, k, h, N]."""
    hB, k, N = A_ref.shape
    assert hB == h * B
    return np.ascontiguousarray(A_ref.reshape(h, B, k, N).transpose(1, 2, 0, 3))


def pma_attention(S, X, wq, bq, wk, bk, h, lengths=None, dtype=np.float64):
    """A[B, k, h, N] = softmax(Q_j K_j^T / sqrt(d)) with Q = fc_q(S), K = fc_k(X); with ``lengths`` the
    keys at and beyond lengths[b] take no part and their entries are zero."""
    S, X, wq, bq, wk, bk = (np.asarray(a, dtype=dtype) for a in (S, X, wq, bq, wk, bk))
    B, N, d = X.shape
    k = S.shape[0]
    dh = d // h
    Q = (S @ wq.T + bq).reshape(k, h, dh)
    A = np.zeros((B, k, h, N), dtype=dtype)
    for b in range(B):
        n = N if lengths is None else int(lengths[b])
        K = (X[b, :n] @ wk.T + bk).reshape(n, h, dh)
        sc = np.einsum("shf,nhf->shn", Q, K) / dtype(np.sqrt(d))
        A[b, :, :, :n] = _softmax(sc)
    return A


def key_of(attn):
    """key[B, N]: the float32 sum of attn over rows r = s * h + j in ascending r, divided by k * h - the
    order the kernel adds in, so the comparison is bitwise."""
    B, k, h, N = attn.shape
    a = np.asarray(attn, dtype=np.float32).reshape(B, k * h, N)
    acc = np.zeros((B, N), dtype=np.float32)
    for r in range(k * h):
        acc = acc + a[:, r, :]
    return acc / np.float32(k * h)


def row_err(A, A64):
    """max over rows of max_n |A - A64| / max_n A64 (rows: everything but the last axis)."""
    A = np.asarray(A, dtype=np.float64)
    A64 = np.asarray(A64, dtype=np.float64)
    num = np.abs(A - A64).max(axis=-1)
    den = A64.max(axis=-1)
    return float((num / den).max())


def desc_order(key, length=None):
    """Point order of pca_select_points for one set: keys descending, -0 == +0, equal keys in ascending
    point order, NaN last, the points at and beyond ``length`` after every valid one in index order."""
    key = np.asarray(key, dtype=np.float32)
    N = key.shape[0]
    length = N if length is None else int(length)
    v = key.astype(np.float64) + 0.0
    cls = np.where(np.isnan(v), 1, 0)
    cls[length:] = 1                       # padding ties with NaN: a valid NaN has the lower index
    neg = np.where(cls == 1, 0.0, -v)
    neg = neg + 0.0                        # -0.0 -> +0.0
    # stable: ties keep ascending index; primary class, then descending key
    return np.lexsort((np.arange(N), neg, cls)).astype(np.int32)


# ---- float64 encoder of the ST (the block input of the shipped-weight cases) ---------------------------
def _mab(Q, K, p, pre, h):
    wq, bq = p[pre + "fc_q.weight"], p[pre + "fc_q.bias"]
    wk, bk = p[pre + "fc_k.weight"], p[pre + "fc_k.bias"]
    wv, bv = p[pre + "fc_v.weight"], p[pre + "fc_v.bias"]
    wo, bo = p[pre + "fc_o.weight"], p[pre + "fc_o.bias"]
    d = wq.shape[0]
    dh = d // h
    Qp, Kp, Vp = Q @ wq.T + bq, K @ wk.T + bk, K @ wv.T + bv
    B, nq, nk = Qp.shape[0], Qp.shape[1], Kp.shape[1]
    q4, k4, v4 = Qp.reshape(B, nq, h, dh), Kp.reshape(B, nk, h, dh), Vp.reshape(B, nk, h, dh)
    A = _softmax(np.einsum("bqhf,bkhf->bhqk", q4, k4) / np.sqrt(d))
    O = Qp + np.einsum("bhqk,bkhf->bqhf", A, v4).reshape(B, nq, d)
    return O + np.maximum(O @ wo.T + bo, 0.0)


def encoder64(X, params, h):
    """enc(X) of Code/models.py:34-37 (two ISABs, modules.py:51-53) in float64.  ``params``: state_dict
    arrays without the 'module.' prefix."""
    p = {k: np.asarray(v, dtype=np.float64) for k, v in params.items()}
    Y = np.asarray(X, dtype=np.float64)
    for li in range(2):
        pre = f"enc.{li}."
        I = np.broadcast_to(p[pre + "I"], (Y.shape[0],) + p[pre + "I"].shape[1:])
        H = _mab(I, Y, p, pre + "mab0.", h)
        Y = _mab(Y, H, p, pre + "mab1.", h)
    return Y


def shipped_block_input(X, params, h):
    """The block input of the shipped-weight cases: float32(encoder64(X)).  The generator rounds the
    reference's own float64 encoder output the same way; the two float64 results differ in the last bits, so
    an element may round the other way once in ~1e8 - one float32 ulp of one input, far inside the bar."""
    return encoder64(X, params, h).astype(np.float32)
