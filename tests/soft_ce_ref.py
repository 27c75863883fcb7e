"""float64 numpy restatement of the soft-target cross-entropy (include/pca_hip.h, PcaSoftTargets):

    t_c   = (1 - eps) (w [c == y1] + (1 - w) [c == y2]) + eps / C
    loss  = logsumexp(x) - sum_c t_c x_c
    dx_c  = (softmax(x)_c - t_c) grad_scale / B
    corr  = [argmax(x) == (w >= 0.5 ? y1 : y2)]

tests/test_soft_targets_host.py checks it against torch.nn.functional.cross_entropy with probability
targets; the GPU tests check the library against it."""
import numpy as np


def _rows(logits, labels, labels2, weight):
    x = np.asarray(logits, dtype=np.float64)
    B = x.shape[0]
    y1 = np.asarray(labels, dtype=np.int64).reshape(B)
    y2 = y1 if labels2 is None else np.asarray(labels2, dtype=np.int64).reshape(B)
    w = np.ones(B) if weight is None else np.asarray(weight, dtype=np.float64).reshape(B)
    return x, y1, y2, w


def targets(labels, labels2, weight, eps, C):
    """t [B, C] float64."""
    y1 = np.asarray(labels, dtype=np.int64).reshape(-1)
    _, y1, y2, w = _rows(np.zeros((len(y1), C)), y1, labels2, weight)
    cls = np.arange(C)[None, :]
    hot1 = (cls == y1[:, None]).astype(np.float64)
    hot2 = (cls == y2[:, None]).astype(np.float64)
    return (1.0 - eps) * (w[:, None] * hot1 + (1.0 - w[:, None]) * hot2) + eps / C


def dominant(labels, labels2=None, weight=None):
    """The label accuracy is counted against: y1 where w >= 0.5 (a tie goes to y1), else y2."""
    y1 = np.asarray(labels, dtype=np.int64).reshape(-1)
    _, y1, y2, w = _rows(np.zeros((len(y1), 1)), y1, labels2, weight)
    return np.where(w >= 0.5, y1, y2)


def soft_ce(logits, labels, labels2=None, weight=None, eps=0.0, grad_scale=1.0):
    """-> dict(per float64 [B] per-sample losses, loss their mean, dlogits float64 [B, C],
    correct int: argmax (first maximum) == dominant label, t the targets)."""
    x, y1, y2, w = _rows(logits, labels, labels2, weight)
    B, C = x.shape
    t = targets(y1, y2, w, eps, C)
    m = x.max(axis=1, keepdims=True)
    e = np.exp(x - m)
    s = e.sum(axis=1, keepdims=True)
    lse = (m + np.log(s))[:, 0]
    per = lse - (t * x).sum(axis=1)
    dlog = (e / s - t) * (grad_scale / B)
    correct = int((x.argmax(axis=1) == dominant(y1, y2, w)).sum())
    return dict(per=per, loss=float(per.mean()), dlogits=dlog, correct=correct, t=t)
