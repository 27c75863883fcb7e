"""torch.autograd glue over the C ABI: device pointers and the current HIP stream are the
only things that cross the boundary (no torch types in the library).

PyTorch is plumbing here -- it owns device memory and streams; all arithmetic of the hot
path runs in libpca_hip.so.
"""
from __future__ import annotations

import ctypes as C
from typing import NamedTuple, Optional, Sequence, Tuple

import math

import numpy as np
import torch

from . import _lib
from ._lib import MabGrads, MabParams, MabShape, check, lib

_MODE = "f32"           # "f32" | "bf16" | "fp8" | "auto"


def set_mode(mode: str) -> None:
    """Arithmetic mode of MAB blocks: 'f32' = exact fp32 kernels (parity mode),
    'bf16' = bf16 MFMA operands with fp32 accumulate/softmax (fails for shapes the fused
    kernels do not cover), 'fp8' = as bf16 with fp8 (e4m3) operands in fc_o of the many-queries
    blocks and fc_k / fc_v of the d = 256 few-queries block (fc_q stays bf16:
    include/pca_hip.h), 'auto' = bf16 where covered, else f32.  Self-attention blocks (modules.SAB:
    per-set queries, Q = K) are covered at every set size for head dims 8 / 16 / 32 (fp8 runs them as
    bf16), so 'auto' resolves them to bf16."""
    global _MODE
    if mode not in ("f32", "bf16", "fp8", "auto"):
        raise ValueError(mode)
    _MODE = mode


def get_mode() -> str:
    return _MODE


def _stream(t: torch.Tensor) -> C.c_void_p:
    return C.c_void_p(torch.cuda.current_stream(t.device).cuda_stream)


def _ptr(t: Optional[torch.Tensor]) -> C.c_void_p:
    return C.c_void_p(0 if t is None else t.data_ptr())


def _need_cuda(*ts: torch.Tensor) -> None:
    for t in ts:
        if t is not None and not t.is_cuda:
            raise _lib.PcaHipError(
                "point-cloud-audio_amd runs on MI355X only: got a CPU tensor "
                "(move the module and its inputs to 'cuda'; there is no CPU fallback)")


def _f32c(t: torch.Tensor) -> torch.Tensor:
    if t.dtype != torch.float32:
        t = t.float()
    return t.contiguous()


# tests: with CANARY set, every scratch / saved block handed to the library is followed by a
# guard region that check_canaries() verifies (a kernel writing past its workspace)
CANARY = False
_GUARD = 1 << 16
_guards: list = []


def _bytes(n: int, like: torch.Tensor) -> torch.Tensor:
    n = max(int(n), 256)
    if not CANARY:
        return torch.empty(n, dtype=torch.uint8, device=like.device)
    n = (n + 255) // 256 * 256
    full = torch.empty(n + _GUARD, dtype=torch.uint8, device=like.device)
    full[n:] = 0xA5
    _guards.append(full[n:])
    return full[:n]


def check_canaries() -> int:
    """Number of guard regions checked; raises if a library call wrote past a block it was given."""
    torch.cuda.synchronize()
    k = len(_guards)
    for g in _guards:
        if not bool((g == 0xA5).all()):
            _guards.clear()
            raise _lib.PcaHipError("a kernel wrote past the end of its workspace")
    _guards.clear()
    return k


def _shape(B, nq, nk, dq, dk, d, h, q_shared, mode=_lib.MODE_F32, k_lengths=None,
           ln: bool = False) -> MabShape:
    return MabShape(B, nq, nk, dq, dk, d, h, int(q_shared), mode, _lib.PCA_F32,
                    _lib.PCA_F32, _lib.PCA_F32, 0 if k_lengths is None else k_lengths.data_ptr(),
                    int(ln))


def _lengths(key_lengths, B: int, like: torch.Tensor):
    """int32[B] on the device of ``like`` (the library reads it there), or None."""
    if key_lengths is None:
        return None
    kl = torch.as_tensor(key_lengths).to(like.device, torch.int32).contiguous()
    if kl.shape != (B,):
        raise RuntimeError(f"key_lengths must have shape ({B},), got {tuple(kl.shape)}")
    return kl


def _unbuilt_input_grad(s: MabShape, need_dq: bool, need_dk: bool) -> Optional[str]:
    """The input gradient a fused block of this shape cannot return, or None.  The layer-1 fused
    kernels take the point set itself: the many-queries block (per-set queries, keys of width d) has
    no dQ at dq <= 4, the few-queries block (shared queries) no dK at dk <= 4 - pca_mab_bwd returns
    PCA_EUNSUPPORTED for them (csrc/mab1_bwd_bf16.hip, csrc/mab0_bwd_bf16.hip, csrc/d256_host.hip).
    A self-attention block (dq = dk) runs the chain, which has both."""
    if need_dq and not s.q_shared and s.dq <= 4 and s.dk == s.d:
        return "dQ"
    if need_dk and s.q_shared and s.dk <= 4:
        return "dK"
    return None


def _pick_mode(s: MabShape, inference: bool = False, need_dq: bool = False,
               need_dk: bool = False) -> MabShape:
    """Resolve the arithmetic mode of one block: 'bf16' demands the fused kernel, 'auto' takes
    it where the library has one for this shape (pca_mab_saved_bytes() > 0; forward-only calls
    ask pca_mab_fwd_ws_bytes(), which also covers the kernels that have no backward yet) else
    exact fp32.  A training block whose backward must return an input gradient the fused kernel
    does not build (``_unbuilt_input_grad``) resolves to exact fp32 under 'auto' and raises here,
    at the forward, under 'bf16' / 'fp8'."""
    if _MODE == "f32":
        return s
    s.mode = _lib.MODE_FP8 if _MODE == "fp8" else _lib.MODE_BF16
    probe = lib().pca_mab_fwd_ws_bytes if inference else lib().pca_mab_saved_bytes
    if _MODE == "auto" and probe(C.byref(s)) == 0:
        s.mode = _lib.MODE_F32
        return s
    if not inference and probe(C.byref(s)) > 0:
        bad = _unbuilt_input_grad(s, need_dq, need_dk)
        if bad is not None and _MODE == "auto":
            s.mode = _lib.MODE_F32
        elif bad is not None:
            raise _lib.PcaHipError(
                f"mab: mode '{_MODE}' has no fused backward that returns {bad} for B={s.B} nq={s.nq} "
                f"nk={s.nk} dq={s.dq} dk={s.dk} d={s.d} h={s.h} q_shared={s.q_shared} (the layer-1 "
                f"kernels do not build the input gradient at width <= 4); use mode 'auto' or 'f32', "
                f"or do not require the gradient of the {'query' if bad == 'dQ' else 'keys'}")
    return s


class _MabFn(torch.autograd.Function):
    """set_transformer-master/modules.py:19-33 MAB.forward + its adjoint."""

    @staticmethod
    def forward(ctx, Q, K, wq, bq, wk, bk, wv, bv, wo, bo, num_heads: int, q_shared: bool,
                key_lengths=None, ln0w=None, ln0b=None, ln1w=None, ln1b=None):
        _need_cuda(Q, K, wq)
        Q, K = _f32c(Q), _f32c(K)
        params = [_f32c(p) for p in (wq, bq, wk, bk, wv, bv, wo, bo)]
        ln = ln0w is not None
        if ln:
            params += [_f32c(p) for p in (ln0w, ln0b, ln1w, ln1b)]
        B, nk, dk = K.shape
        if q_shared:
            nq, dq = Q.shape[-2], Q.shape[-1]
        else:
            if Q.shape[0] != B:
                raise RuntimeError(f"MAB: batch mismatch Q {tuple(Q.shape)} K {tuple(K.shape)}")
            nq, dq = Q.shape[1], Q.shape[2]
        d = params[0].shape[0]
        if params[0].shape[1] != dq or params[2].shape[1] != dk:
            raise RuntimeError("MAB: input width does not match fc_q / fc_k")
        kl = _lengths(key_lengths, B, K)
        s = _pick_mode(_shape(B, nq, nk, dq, dk, d, num_heads, q_shared, k_lengths=kl, ln=ln),
                       need_dq=ctx.needs_input_grad[0], need_dk=ctx.needs_input_grad[1])
        ctx.kl = kl                       # keeps the device array alive for the backward
        ctx.ln = ln
        L = lib()
        with torch.cuda.device(K.device):
            Y = torch.empty((B, nq, d), dtype=torch.float32, device=K.device)
            nsaved = L.pca_mab_saved_bytes(C.byref(s))
            if nsaved == 0:
                raise _lib.PcaHipError("pca_mab_saved_bytes: " + L.pca_last_error().decode())
            saved = _bytes(nsaved, K)
            ws = _bytes(L.pca_mab_fwd_ws_bytes(C.byref(s)), K)
            pp = MabParams(*[_ptr(p) for p in params])      # (ln pointers stay NULL without ln)
            check(L.pca_mab_fwd(C.byref(s), _ptr(Q), _ptr(K), C.byref(pp), _ptr(Y),
                                _ptr(saved), _ptr(ws), _stream(K)), "pca_mab_fwd")
        ctx.s = s
        ctx.save_for_backward(Q, K, saved, *params)
        return Y

    @staticmethod
    def backward(ctx, dY):
        Q, K, saved, *params = ctx.saved_tensors
        s = ctx.s
        L = lib()
        dY = _f32c(dY)
        need_dq, need_dk = ctx.needs_input_grad[0], ctx.needs_input_grad[1]
        with torch.cuda.device(K.device):
            sizes = [p.numel() for p in params]
            flat = torch.zeros(sum(sizes), dtype=torch.float32, device=K.device)
            gviews = list(torch.split(flat, sizes))
            gg = MabGrads(*[_ptr(g) for g in gviews])
            pp = MabParams(*[_ptr(p) for p in params])
            dQ = dK = None
            if need_dq:
                dQ = (torch.zeros_like(Q) if s.q_shared else torch.empty_like(Q))
            if need_dk:
                dK = torch.empty_like(K)
            ws = _bytes(L.pca_mab_bwd_ws_bytes(C.byref(s)), K)
            check(L.pca_mab_bwd(C.byref(s), _ptr(Q), _ptr(K), C.byref(pp), _ptr(saved),
                                _ptr(dY), _ptr(dQ), _ptr(dK), 0, C.byref(gg), _ptr(ws),
                                _stream(K)), "pca_mab_bwd")
        grads = [g.view_as(p) for g, p in zip(gviews, params)]
        if ctx.ln:
            return (dQ, dK, *grads[:8], None, None, None, *grads[8:])
        return (dQ, dK, *grads, None, None, None, None, None, None, None)


def mab(Q, K, wq, bq, wk, bk, wv, bv, wo, bo, num_heads: int, q_shared: bool = False,
        key_lengths=None, ln_params=None):
    """key_lengths (optional, int[B]): valid keys per set of a padded batch.
    ln_params (optional): (ln0.weight, ln0.bias, ln1.weight, ln1.bias) of MAB(ln=True)."""
    extra = tuple(ln_params) if ln_params is not None else (None, None, None, None)
    return _MabFn.apply(Q, K, wq, bq, wk, bk, wv, bv, wo, bo, num_heads, q_shared, key_lengths,
                        *extra)


def mab_infer(Q, K, params, num_heads: int, q_shared: bool = False,
              key_lengths=None, ln_params=None) -> torch.Tensor:
    """Forward only, nothing saved (used under torch.no_grad())."""
    _need_cuda(Q, K)
    Q, K = _f32c(Q), _f32c(K)
    params = [_f32c(p) for p in params]
    ln = ln_params is not None
    if ln:
        params += [_f32c(p) for p in ln_params]
    B, nk, dk = K.shape
    nq, dq = Q.shape[-2], Q.shape[-1]
    d = params[0].shape[0]
    kl = _lengths(key_lengths, B, K)
    s = _pick_mode(_shape(B, nq, nk, dq, dk, d, num_heads, q_shared, k_lengths=kl, ln=ln),
                   inference=True)
    L = lib()
    with torch.cuda.device(K.device):
        Y = torch.empty((B, nq, d), dtype=torch.float32, device=K.device)
        ws = _bytes(L.pca_mab_fwd_ws_bytes(C.byref(s)), K)
        pp = MabParams(*[_ptr(p) for p in params])
        check(L.pca_mab_fwd(C.byref(s), _ptr(Q), _ptr(K), C.byref(pp), _ptr(Y), None,
                            _ptr(ws), _stream(K)), "pca_mab_fwd")
    return Y


def pma_attention(S, X, params, num_heads: int, key_lengths=None, want_key: bool = False):
    """The pooling attention of a PMA block (pca_pma_attention): the `A` of
    set_transformer-master/modules.py:21-27 that MAB.forward builds and drops.
    S [k, d] or [1, k, d] the seeds, X [B, N, d] float32, ``params`` = (fc_q.weight, fc_q.bias, fc_k.weight,
    fc_k.bias[, ...]): only the first four are read.  Returns attn [B, k, h, N] float32 - the reference's
    own [h * B, k, N] row (j * B + b, s) is attn[b, s, j, :] - and, with ``want_key``, (attn, key): key
    [B, N], the mean over seeds and heads that select_points sorts by.  ``key_lengths`` int[B]: keys at and
    beyond it take no part and come out as exact zeros.  fp32 whatever the mode (set_mode is not consulted).
    Not differentiable: a diagnostic, computed outside autograd."""
    _need_cuda(S, X)
    S, X = _f32c(S.detach()), _f32c(X.detach())
    params = [_f32c(p.detach()) for p in list(params)[:4]]
    _need_cuda(*params)
    if X.dim() != 3:
        raise RuntimeError(f"pma_attention: X must be [B, N, d], got {tuple(X.shape)}")
    B, N, d = X.shape
    S = S.reshape(-1, S.shape[-1])
    k = S.shape[0]
    if S.shape[1] != d or tuple(params[0].shape) != (d, d) or tuple(params[2].shape) != (d, d):
        raise RuntimeError("pma_attention: the widths of S, X, fc_q and fc_k do not match")
    kl = _lengths(key_lengths, B, X)
    s = _shape(B, k, N, d, d, d, num_heads, True, k_lengths=kl)
    L = lib()
    with torch.cuda.device(X.device):
        n = L.pca_pma_attention_ws_bytes(C.byref(s))
        if n == 0:
            raise _lib.PcaHipError("pca_pma_attention_ws_bytes: " + L.pca_last_error().decode())
        ws = _bytes(n, X)
        attn = torch.empty((B, k, num_heads, N), dtype=torch.float32, device=X.device)
        key = torch.empty((B, N), dtype=torch.float32, device=X.device) if want_key else None
        pp = MabParams(*([_ptr(p) for p in params] + [None] * 8))
        check(L.pca_pma_attention(C.byref(s), _ptr(S), _ptr(X), C.byref(pp), _ptr(attn), _ptr(key),
                                  _ptr(ws), _stream(X)), "pca_pma_attention")
    return (attn, key) if want_key else attn


class _LinearFn(torch.autograd.Function):
    """nn.Linear (Code/models.py:40) on the library's GEMM."""

    @staticmethod
    def forward(ctx, X, W, b):
        _need_cuda(X, W, b)
        X, W, b = _f32c(X), _f32c(W), _f32c(b)
        lead = X.shape[:-1]
        M = X.numel() // X.shape[-1]
        with torch.cuda.device(X.device):
            Y = torch.empty((*lead, W.shape[0]), dtype=torch.float32, device=X.device)
            check(lib().pca_linear_fwd(_ptr(X), _ptr(W), _ptr(b), _ptr(Y), M, W.shape[1],
                                       W.shape[0], _stream(X)), "pca_linear_fwd")
        ctx.save_for_backward(X, W)
        return Y

    @staticmethod
    def backward(ctx, dY):
        X, W = ctx.saved_tensors
        dY = _f32c(dY)
        M = X.numel() // X.shape[-1]
        with torch.cuda.device(X.device):
            dX = torch.empty_like(X) if ctx.needs_input_grad[0] else None
            dW = torch.zeros_like(W)
            db = torch.zeros(W.shape[0], dtype=torch.float32, device=X.device)
            check(lib().pca_linear_bwd(_ptr(X), _ptr(W), _ptr(dY), _ptr(dX), _ptr(dW),
                                       _ptr(db), M, W.shape[1], W.shape[0], None,
                                       _stream(X)), "pca_linear_bwd")
        return dX, dW, db


def linear(X, W, b):
    return _LinearFn.apply(X, W, b)


class _CrossEntropyFn(torch.autograd.Function):
    """nn.CrossEntropyLoss() (mean), Code/settransformer.py:88,104; with ``labels2`` / ``weight`` /
    ``label_smoothing`` the soft-target form (pca_cross_entropy_soft)."""

    @staticmethod
    def forward(ctx, logits, labels, labels2=None, weight=None, label_smoothing=0.0):
        _need_cuda(logits, labels, labels2, weight)
        logits = _f32c(logits)
        labels = labels.to(torch.int64).contiguous()
        B, Cc = logits.shape
        soft = labels2 is not None or weight is not None or label_smoothing != 0.0
        with torch.cuda.device(logits.device):
            loss = torch.empty(1, dtype=torch.float32, device=logits.device)
            dlog = torch.empty_like(logits)
            if soft:
                if labels2 is not None:
                    labels2 = labels2.to(torch.int64).contiguous()
                    assert labels2.numel() == B
                if weight is not None:
                    weight = _f32c(weight)
                    assert weight.numel() == B
                tg = _lib.PcaSoftTargets(_ptr(labels2).value, _ptr(weight).value, float(label_smoothing))
                check(lib().pca_cross_entropy_soft(_ptr(logits), _ptr(labels), C.byref(tg), B, Cc, 1.0,
                                                   _ptr(loss), _ptr(dlog), None, _stream(logits)),
                      "pca_cross_entropy_soft")
            else:
                check(lib().pca_cross_entropy(_ptr(logits), _ptr(labels), B, Cc, 1.0, _ptr(loss),
                                              _ptr(dlog), None, _stream(logits)),
                      "pca_cross_entropy")
        ctx.save_for_backward(dlog)
        return loss.squeeze(0)

    @staticmethod
    def backward(ctx, g):
        (dlog,) = ctx.saved_tensors
        return dlog * g, None, None, None, None


def cross_entropy(logits, labels, labels2=None, weight=None, label_smoothing=0.0):
    """Mean cross-entropy of ``logits`` [B, C] against ``labels`` int64 [B].  With ``labels2`` int64 [B],
    ``weight`` float32 [B] in [0, 1] (the share of ``labels``) and / or ``label_smoothing`` in [0, 1) the
    target of sample b is (1 - eps)(w onehot(labels) + (1 - w) onehot(labels2)) + eps / C, as
    ``torch.nn.functional.cross_entropy`` with probability targets; ``labels2=None`` means labels,
    ``weight=None`` means 1.  No gradient flows to the targets.  The two-argument call runs
    pca_cross_entropy as before."""
    if labels2 is None and weight is None and label_smoothing == 0.0:
        return _CrossEntropyFn.apply(logits, labels)
    return _CrossEntropyFn.apply(logits, labels, labels2, weight, float(label_smoothing))


def eval_tally(logits: torch.Tensor, labels: torch.Tensor, counts: torch.Tensor,
               slot: int = 0) -> torch.Tensor:
    """counts[slot] += #(logits.argmax(1) == labels) on the device (pca_eval_tally): no host
    sync; argmax as torch.argmax (first maximum, NaN is the maximum).  logits [B, C] float32,
    labels int64[B], counts int64 (contiguous).  Returns ``counts``."""
    _need_cuda(logits, labels, counts)
    assert logits.dim() == 2 and logits.dtype == torch.float32 and logits.is_contiguous()
    assert labels.dtype == torch.int64 and labels.is_contiguous()
    assert labels.numel() == logits.shape[0]
    assert counts.dtype == torch.int64 and counts.is_contiguous() and 0 <= slot < counts.numel()
    with torch.cuda.device(logits.device):
        check(lib().pca_eval_tally(_ptr(logits), _ptr(labels), logits.shape[0], logits.shape[1],
                                   _ptr(counts), int(slot), _stream(logits)), "pca_eval_tally")
    return counts


def clip_aggregate(logits: torch.Tensor, offsets: torch.Tensor,
                   labels: Optional[torch.Tensor] = None, counts: Optional[torch.Tensor] = None,
                   slot: int = 0):
    """Per-clip aggregation of frame (or chunk) logits on the device (pca_clip_aggregate): no host
    sync.  logits [n_sets, C] float32; offsets int64[n_clips + 1], non-decreasing: clip c owns rows
    offsets[c] : offsets[c + 1].  Returns (pred, mean_logprob, votes):
    mean_logprob [n_clips, C] float32, the mean of log_softmax over the clip's rows; votes
    [n_clips, C] int32, the rows whose argmax (as torch.argmax) is the class; pred int64
    [n_clips, 2], column 0 by votes (ties to the higher mean log-prob, then the lower class),
    column 1 by mean log-prob.  A clip without rows gets zeros and pred -1.
    With ``labels`` int64[n_clips] and ``counts`` int64 (both or neither):
    counts[2 * slot] += clips the vote rule gets right, counts[2 * slot + 1] += the mean rule's."""
    _need_cuda(logits, offsets, labels, counts)
    assert logits.dim() == 2 and logits.dtype == torch.float32 and logits.is_contiguous()
    assert offsets.dim() == 1 and offsets.dtype == torch.int64 and offsets.is_contiguous()
    assert offsets.numel() >= 1 and logits.shape[1] >= 1
    n_sets, Cc = logits.shape
    n_clips = offsets.numel() - 1
    assert (labels is None) == (counts is None), "labels and counts go together"
    if labels is not None:
        assert labels.dtype == torch.int64 and labels.is_contiguous() and labels.numel() == n_clips
        assert counts.dtype == torch.int64 and counts.is_contiguous()
        assert 0 <= slot and 2 * slot + 1 < counts.numel()
    with torch.cuda.device(logits.device):
        mean = torch.empty((n_clips, Cc), dtype=torch.float32, device=logits.device)
        votes = torch.empty((n_clips, Cc), dtype=torch.int32, device=logits.device)
        pred = torch.empty((n_clips, 2), dtype=torch.int64, device=logits.device)
        check(lib().pca_clip_aggregate(_ptr(logits), n_sets, Cc, _ptr(offsets), n_clips,
                                       _ptr(labels), _ptr(mean), _ptr(votes), _ptr(pred),
                                       _ptr(counts), int(slot), _stream(logits)),
              "pca_clip_aggregate")
    return pred, mean, votes


def eval_metrics(logits: torch.Tensor, labels: torch.Tensor, topk: int = 5,
                 counts: Optional[torch.Tensor] = None, slot: int = 0,
                 confusion: Optional[torch.Tensor] = None,
                 loss_sum: Optional[torch.Tensor] = None, rows: bool = False):
    """Held-out metrics of a whole logit buffer on the device (pca_eval_metrics): no host sync.
    logits [n_rows, C] float32, labels int64[n_rows].  Per row: loss = logsumexp - logit of the label,
    pred = argmax as torch.argmax, rank = classes ordered before the label's (top-k correct when
    rank < topk); a row whose label is outside [0, C) is skipped and counted as skipped.
    Accumulated into the caller's device tensors, each optional:
    counts int64: counts[4 * slot + {0, 1, 2, 3}] += {scored, top-1 correct, top-k correct, skipped};
    confusion int64 [C, C]: confusion[label, pred] += 1; loss_sum float64[1] += sum of the losses
    (fp64, fixed order: bit-reproducible).
    Returns (row_loss float32, row_pred int64, row_rank int32) with ``rows``, else None."""
    _need_cuda(logits, labels, counts, confusion, loss_sum)
    assert logits.dim() == 2 and logits.dtype == torch.float32 and logits.is_contiguous()
    assert labels.dtype == torch.int64 and labels.is_contiguous()
    n, Cc = logits.shape
    assert labels.numel() == n and Cc >= 1 and topk >= 1
    if counts is not None:
        assert counts.dtype == torch.int64 and counts.is_contiguous()
        assert 0 <= slot and 4 * slot + 3 < counts.numel()
    if confusion is not None:
        assert confusion.dtype == torch.int64 and confusion.is_contiguous()
        assert tuple(confusion.shape) == (Cc, Cc)
    if loss_sum is not None:
        assert loss_sum.dtype == torch.float64 and loss_sum.numel() >= 1
    L = lib()
    dev = logits.device
    with torch.cuda.device(dev):
        out = (None, None, None)
        if rows:
            out = (torch.empty(n, dtype=torch.float32, device=dev),
                   torch.empty(n, dtype=torch.int64, device=dev),
                   torch.empty(n, dtype=torch.int32, device=dev))
        ws = None
        if counts is not None or loss_sum is not None:
            ws = _bytes(L.pca_eval_metrics_ws_bytes(n), logits)
        check(L.pca_eval_metrics(_ptr(logits), _ptr(labels), n, Cc, int(topk), _ptr(out[0]),
                                 _ptr(out[1]), _ptr(out[2]), _ptr(counts), int(slot),
                                 _ptr(confusion), _ptr(loss_sum), _ptr(ws), _stream(logits)),
              "pca_eval_metrics")
    return out if rows else None


# --------------------------------------------------------------------------- #
# feature extraction                                                           #
# --------------------------------------------------------------------------- #
def stft_logmag(wave: torch.Tensor, n_fft: int, win_length: Optional[int] = None,
                hop: Optional[int] = None, drop_nyquist: bool = False,
                frame_major: bool = False) -> torch.Tensor:
    """log(1e-8 + |stft|/n_fft) of a 1-D float32 device waveform.
    Returns [F, T] (reference layout) or, with frame_major, [T, F] (each frame -- one
    2-D point set -- contiguous, the layout the packers read coalesced)."""
    _need_cuda(wave)
    wave = _f32c(wave)
    win_length = n_fft if win_length is None else win_length
    hop = n_fft // 2 if hop is None else hop
    L = lib()
    T = L.pca_stft_num_frames(wave.numel(), hop)
    F = n_fft // 2 if drop_nyquist else n_fft // 2 + 1
    with torch.cuda.device(wave.device):
        if frame_major:
            out = torch.empty((T, F), dtype=torch.float32, device=wave.device)
            sf, st = 1, F
        else:
            out = torch.empty((F, T), dtype=torch.float32, device=wave.device)
            sf, st = T, 1
        check(L.pca_stft_logmag(_ptr(wave), wave.numel(), n_fft, win_length, hop, F,
                                _ptr(out), sf, st, _stream(wave)), "pca_stft_logmag")
    return out


# ---- resampling (the sampling-rate axis of the evaluation sweep, Code/pceval.py:74) ----------------
# librosa.resample(.., res_type='kaiser_fast', scale=True) = resampy's band-limited interpolation; the
# filter design below is resampy's documented kaiser_fast (16 zero crossings, 512 table entries per
# zero crossing, roll-off 0.85, Kaiser beta 8.5555): "parity unpinned" (neither package is available).
KAISER_FAST = dict(num_zeros=16, precision=9, rolloff=0.85, beta=8.555504641634386)
_resample_tables = {}


def _resample_filter(ratio: float, device, design):
    import numpy as np
    key = (round(ratio, 12), str(device), tuple(sorted(design.items())))
    if key not in _resample_tables:
        num_table = 2 ** design["precision"]
        n = num_table * design["num_zeros"]
        win = design["rolloff"] * np.sinc(design["rolloff"] * np.linspace(0, design["num_zeros"], n + 1))
        win = win * np.kaiser(2 * n + 1, design["beta"])[n:]
        if ratio < 1:
            win = win * ratio
        delta = np.zeros_like(win)
        delta[:-1] = np.diff(win)
        _resample_tables[key] = (torch.from_numpy(win).to(device), torch.from_numpy(delta).to(device),
                                 num_table)
    return _resample_tables[key]


def resample(wave: torch.Tensor, fs_old: float, fs_new: float, scale: bool = True,
             **design) -> torch.Tensor:
    """1-D float32 device waveform at fs_old -> ceil(n * fs_new / fs_old) samples at fs_new
    (librosa.resample(x, fs_old, fs_new, res_type='kaiser_fast', fix=True, scale=scale))."""
    _need_cuda(wave)
    wave = _f32c(wave)
    ratio = float(fs_new) / float(fs_old)
    if ratio == 1.0:
        return wave.clone()
    d = dict(KAISER_FAST)
    d.update(design)
    win, delta, num_table = _resample_filter(ratio, wave.device, d)
    n_in = wave.numel()
    n_res = int(n_in * ratio)
    n_out = int(math.ceil(n_in * ratio))
    with torch.cuda.device(wave.device):
        out = torch.zeros(n_out, dtype=torch.float32, device=wave.device)
        if n_res > 0:
            check(lib().pca_resample(_ptr(wave), n_in, ratio, _ptr(win), _ptr(delta), win.numel(),
                                     num_table, (1.0 / math.sqrt(ratio)) if scale else 1.0, _ptr(out),
                                     min(n_res, n_out), _stream(wave)), "pca_resample")
    return out


# ---- silence trimming (librosa.effects.trim, the step before resampling / STFT in every script) ------
def trim_batch(waves, top_db: float = 60, frame_length: int = 2048, hop_length: int = 512):
    """Leading / trailing silence of a list of 1-D float32 device waveforms, as
    ``librosa.effects.trim(x, top_db, frame_length=, hop_length=)`` (Code/pceval.py:74; librosa 0.8
    semantics restated, "parity unpinned": librosa is not available and the reference holds no trimmed
    fixture).  One pca_trim_bounds call and one host read of the bounds for the whole list.
    Returns (clips, bounds): clips[c] = waves[c][start:end], a view of the input (no copy), and
    bounds the int64 ndarray [n, 2] of (start, end)."""
    waves = list(waves)
    assert len(waves) > 0
    _need_cuda(*waves)
    for w in waves:
        if w.dim() != 1 or w.dtype != torch.float32:
            raise _lib.PcaHipError(f"trim: 1-D float32 waveforms, got {tuple(w.shape)} {w.dtype}")
    dev = waves[0].device
    lens = [int(w.numel()) for w in waves]
    woff = [0]
    for n in lens:
        woff.append(woff[-1] + n)
    L = lib()
    with torch.cuda.device(dev):
        cat = waves[0].contiguous() if len(waves) == 1 else torch.cat(waves)
        woff_d = torch.tensor(woff, dtype=torch.int64, device=dev)
        bounds = torch.empty((len(waves), 2), dtype=torch.int64, device=dev)
        ws = _bytes(L.pca_trim_ws_bytes(woff[-1], len(waves), frame_length, hop_length), cat)
        check(L.pca_trim_bounds(_ptr(cat), _ptr(woff_d), len(waves), max(lens), min(lens),
                                frame_length, hop_length, float(top_db), _ptr(bounds), _ptr(ws),
                                _stream(cat)), "pca_trim_bounds")
        b = bounds.cpu().numpy()                               # the one host read
    return [w[int(s):int(e)] for w, (s, e) in zip(waves, b)], b


def trim(wave: torch.Tensor, top_db: float = 60, frame_length: int = 2048,
         hop_length: int = 512):
    """``librosa.effects.trim`` of one 1-D float32 device waveform: (wave[start:end] as a view,
    (start, end)).  See trim_batch."""
    clips, b = trim_batch([wave], top_db, frame_length, hop_length)
    return clips[0], (int(b[0, 0]), int(b[0, 1]))


def stft_logmag_batch(waves, n_fft: int, win_length: Optional[int] = None,
                      hop: Optional[int] = None, drop_nyquist: bool = False,
                      frame_major: bool = False, norm: Optional[float] = None,
                      frame_align: int = 1):
    """log(1e-8 + |stft|/n_fft) of a list of 1-D float32 device waveforms in ONE launch.
    Returns (spec, frame_off): spec is [F, T_total] (or [T_total, F] with frame_major), clip c
    occupies columns (rows) frame_off[c] : frame_off[c + 1]; each clip's block is bit-identical
    to stft_logmag(clip).

    ``norm``: divide the magnitude by ``norm`` instead of n_fft (pca_stft_logmag_batch_norm; the
    re-framing loops of Code/pc_temp3d_eval.py:75 divide by the window length N); None keeps
    the n_fft divisor and the plain entry point.
    ``frame_align`` > 1: every clip's first frame lands on a multiple of ``frame_align`` (and
    T_total is one too), so that chunks of ``frame_align`` frames never straddle two clips; clip
    c then holds the first 1 + len_c // hop frames of frame_off[c] : frame_off[c + 1] and the
    frames after them are zeros."""
    assert len(waves) > 0
    assert frame_align >= 1
    _need_cuda(*waves)
    dev = waves[0].device
    win_length = n_fft if win_length is None else win_length
    hop = n_fft // 2 if hop is None else hop
    lens = [int(w.numel()) for w in waves]
    frames = [1 + n // hop for n in lens]
    woff = [0]
    foff = [0]
    for n, t in zip(lens, frames):
        woff.append(woff[-1] + n)
        foff.append(-(-(foff[-1] + t) // frame_align) * frame_align)
    T = foff[-1]
    F = n_fft // 2 if drop_nyquist else n_fft // 2 + 1
    L = lib()
    alloc = torch.empty if frame_align == 1 else torch.zeros
    with torch.cuda.device(dev):
        cat = torch.cat([_f32c(w).reshape(-1) for w in waves])
        woff_d = torch.tensor(woff, dtype=torch.int64, device=dev)
        foff_d = torch.tensor(foff, dtype=torch.int64, device=dev)
        if frame_major:
            out = alloc((T, F), dtype=torch.float32, device=dev)
            sf, st = 1, F
        else:
            out = alloc((F, T), dtype=torch.float32, device=dev)
            sf, st = T, 1
        if norm is None:
            check(L.pca_stft_logmag_batch(_ptr(cat), _ptr(woff_d), _ptr(foff_d), len(waves),
                                          max(lens), min(lens), n_fft, win_length, hop, F,
                                          _ptr(out), sf, st, _stream(cat)), "pca_stft_logmag_batch")
        else:
            check(L.pca_stft_logmag_batch_norm(_ptr(cat), _ptr(woff_d), _ptr(foff_d), len(waves),
                                               max(lens), min(lens), n_fft, win_length, hop, F,
                                               _ptr(out), sf, st, float(norm), _stream(cat)),
                  "pca_stft_logmag_batch_norm")
    return out, foff


def pack_points_2d(spec: torch.Tensor, farr: torch.Tensor, idx: torch.Tensor,
                   labels: Optional[torch.Tensor] = None, frame_major: bool = False,
                   out: Optional[torch.Tensor] = None, labels_out: Optional[torch.Tensor] = None
                   ) -> Tuple[torch.Tensor, Optional[torch.Tensor]]:
    """Batch of ESC_pc items: spec [F,T] (or [T,F] frame_major), idx int64[B] ->
    ([B,F,2] float32, labels[idx])."""
    _need_cuda(spec, farr, idx)
    assert spec.dtype == torch.float32 and farr.dtype == torch.float32
    assert idx.dtype == torch.int64
    if frame_major:
        T, F = spec.shape
        sf, st = spec.stride(1), spec.stride(0)
    else:
        F, T = spec.shape
        sf, st = spec.stride(0), spec.stride(1)
    B = idx.numel()
    with torch.cuda.device(spec.device):
        if out is None:
            out = torch.empty((B, F, 2), dtype=torch.float32, device=spec.device)
        if labels is not None and labels_out is None:
            labels_out = torch.empty(B, dtype=torch.int64, device=spec.device)
        check(lib().pca_pack_points_2d(_ptr(spec), sf, st, _ptr(farr), _ptr(idx), B, F,
                                       _ptr(out), _ptr(labels), _ptr(labels_out),
                                       _stream(spec)), "pca_pack_points_2d")
    return out, labels_out


def pack_points_3d(spec: torch.Tensor, farr: torch.Tensor, tarr: torch.Tensor,
                   idx: torch.Tensor, labels: Optional[torch.Tensor] = None,
                   out: Optional[torch.Tensor] = None,
                   labels_out: Optional[torch.Tensor] = None,
                   nt_valid: Optional[torch.Tensor] = None,
                   lengths_out: Optional[torch.Tensor] = None):
    """Batch of ESC_pc_temp items: spec indexed [f, t, s] through its strides (any
    layout), idx int64[B] -> ([B, Nt*F, 3] float32, labels[idx]).
    With ``nt_valid`` (device int32[S], frames held by each chunk) the batch is padded:
    returns (points, labels[idx], lengths int32[B]) (pca_pack_points_3d_var)."""
    _need_cuda(spec, farr, tarr, idx)
    assert spec.dtype == torch.float32 and idx.dtype == torch.int64
    F, Nt, S = spec.shape
    B = idx.numel()
    with torch.cuda.device(spec.device):
        if out is None:
            out = torch.empty((B, F * Nt, 3), dtype=torch.float32, device=spec.device)
        if labels is not None and labels_out is None:
            labels_out = torch.empty(B, dtype=torch.int64, device=spec.device)
        if nt_valid is not None:
            _need_cuda(nt_valid)
            assert nt_valid.dtype == torch.int32 and nt_valid.numel() == S
            if lengths_out is None:
                lengths_out = torch.empty(B, dtype=torch.int32, device=spec.device)
            check(lib().pca_pack_points_3d_var(
                _ptr(spec), spec.stride(0), spec.stride(1), spec.stride(2), _ptr(farr),
                _ptr(tarr), _ptr(nt_valid), _ptr(idx), B, F, Nt, _ptr(out), _ptr(lengths_out),
                _ptr(labels), _ptr(labels_out), _stream(spec)), "pca_pack_points_3d_var")
            return out, labels_out, lengths_out
        check(lib().pca_pack_points_3d(_ptr(spec), spec.stride(0), spec.stride(1),
                                       spec.stride(2), _ptr(farr), _ptr(tarr), _ptr(idx), B,
                                       F, Nt, _ptr(out), _ptr(labels), _ptr(labels_out),
                                       _stream(spec)), "pca_pack_points_3d")
    return out, labels_out


MAXK, RANDK = 0, 1


def _draw_ptr(draw_dev):
    if draw_dev is None:
        return None
    assert draw_dev.is_cuda and draw_dev.dtype == torch.int32 and draw_dev.numel() >= 1
    return draw_dev.data_ptr()


def subsample_points(spec: torch.Tensor, farr: torch.Tensor, tarr: Optional[torch.Tensor],
                     idx: torch.Tensor, K: int, mode: int = MAXK, seed: int = 0,
                     draw: int = 0, labels: Optional[torch.Tensor] = None,
                     out: Optional[torch.Tensor] = None,
                     labels_out: Optional[torch.Tensor] = None, want_sel: bool = False,
                     draw_dev: Optional[torch.Tensor] = None):
    """Batch of sub-sampled point sets selected on the device (pca_subsample_points).
    ``draw_dev`` (device int32, optional): its first element is added to ``draw`` on the device,
    so a launch captured into a hipGraph draws a fresh selection on every replay.

    spec indexed [f, t, s] through its strides ([F, T] with tarr=None for the framewise
    2-D case); idx int64[B].  mode MAXK: the K largest values per set, descending
    (Code/dataset.py:196, Code/utils.py:42); RANDK: K points of a random permutation
    (Code/dataset.py:236, Code/utils.py:70) from the stream (seed, draw).
    Returns (points [B, K, din] float32, labels[idx] or None[, sel int32 [B, K]])."""
    _need_cuda(spec, farr, idx)
    assert spec.dtype == torch.float32 and idx.dtype == torch.int64
    if tarr is None:
        assert spec.dim() == 2
        F, Nt = spec.shape[0], 1
        sf, st, ss = spec.stride(0), 0, spec.stride(1)
        din = 2
    else:
        _need_cuda(tarr)
        F, Nt, _ = spec.shape
        sf, st, ss = spec.stride(0), spec.stride(1), spec.stride(2)
        din = 3
    B = idx.numel()
    with torch.cuda.device(spec.device):
        if out is None:
            out = torch.empty((B, K, din), dtype=torch.float32, device=spec.device)
        if labels is not None and labels_out is None:
            labels_out = torch.empty(B, dtype=torch.int64, device=spec.device)
        sel = torch.empty((B, K), dtype=torch.int32, device=spec.device) if want_sel else None
        check(lib().pca_subsample_points(_ptr(spec), sf, st, ss, _ptr(farr), _ptr(tarr),
                                         _ptr(idx), B, F, Nt, int(K), int(mode),
                                         int(seed) & (2 ** 64 - 1), int(draw) & (2 ** 64 - 1),
                                         _draw_ptr(draw_dev), _ptr(out), _ptr(sel),
                                         _ptr(labels), _ptr(labels_out), _stream(spec)),
              "pca_subsample_points")
    return (out, labels_out, sel) if want_sel else (out, labels_out)


NORM_NFFT, NORM_WIN = 0, 1


def frame_points(waves: torch.Tensor, wave_off: torch.Tensor, set_off: torch.Tensor,
                 idx: torch.Tensor, n_fft: int, hop: int, n_bins: int, farr: torch.Tensor,
                 tarr: Optional[torch.Tensor] = None, Nt: int = 1, *, max_len: int, min_len: int,
                 clip_labels: Optional[torch.Tensor] = None, jitter: int = 0,
                 gain_db: float = 0.0, win_lengths: Optional[torch.Tensor] = None,
                 norm_mode: int = NORM_NFFT, seed: int = 0, draw: int = 0,
                 out: Optional[torch.Tensor] = None, labels_out: Optional[torch.Tensor] = None,
                 draw_dev: Optional[torch.Tensor] = None, want_meta: bool = False):
    """Batch of point sets framed from resident waveforms and augmented on the device
    (pca_frame_points): no spectrogram is kept, every call cuts its frames anew.

    waves float32: the clips back to back; wave_off int64[n_clips + 1] their sample offsets;
    set_off int64[n_clips + 1] the prefix sum of the sets per clip (1 + len // hop frames with
    Nt = 1, frames // Nt whole chunks otherwise); idx int64[B] set ids; max_len / min_len the
    longest / shortest clip (host values).  All tensors on the device.
    Per batch slot one time shift in [-jitter, jitter] samples, one gain of up to +-gain_db dB and
    one window length out of ``win_lengths`` (device int32; None: n_fft) from the stream (seed,
    draw); a field left at its default is off and exact.  ``norm_mode`` NORM_NFFT divides the
    magnitude by n_fft, NORM_WIN by the slot's window length.  ``draw_dev`` (device int32,
    optional): its first element is added to ``draw`` on the device, so a launch captured into a
    hipGraph draws afresh on every replay.
    Returns (points [B, Nt * n_bins, 2 or 3] float32, clip_labels of each slot's clip or None
    [, meta int32 [B, 4] = (clip, centre sample of frame 0, window length, bits of the fp32 gain)])."""
    _need_cuda(waves, wave_off, set_off, idx, farr)
    assert waves.dtype == torch.float32 and waves.is_contiguous() and farr.dtype == torch.float32
    assert wave_off.dtype == set_off.dtype == idx.dtype == torch.int64
    assert wave_off.numel() == set_off.numel() >= 2 and farr.numel() >= n_bins
    din = 2
    if tarr is not None:
        _need_cuda(tarr)
        assert tarr.dtype == torch.float32 and tarr.numel() >= Nt
        din = 3
    B = idx.numel()
    with torch.cuda.device(waves.device):
        if win_lengths is None:
            win_lengths = torch.tensor([n_fft], dtype=torch.int32, device=waves.device)
        assert win_lengths.is_cuda and win_lengths.dtype == torch.int32
        if out is None:
            out = torch.empty((B, Nt * n_bins, din), dtype=torch.float32, device=waves.device)
        if clip_labels is not None and labels_out is None:
            labels_out = torch.empty(B, dtype=torch.int64, device=waves.device)
        meta = torch.empty((B, 4), dtype=torch.int32, device=waves.device) if want_meta else None
        aug = _lib.PcaFrameAug(int(jitter), float(gain_db), win_lengths.data_ptr(),
                               win_lengths.numel(), int(norm_mode), int(seed) & (2 ** 64 - 1),
                               int(draw) & (2 ** 64 - 1), _draw_ptr(draw_dev))
        check(lib().pca_frame_points(_ptr(waves), _ptr(wave_off), _ptr(set_off),
                                     wave_off.numel() - 1, int(max_len), int(min_len),
                                     _ptr(clip_labels), _ptr(idx), B, int(n_fft), int(hop),
                                     int(n_bins), int(Nt), _ptr(farr), _ptr(tarr), C.byref(aug),
                                     _ptr(out), _ptr(labels_out), _ptr(meta), _stream(waves)),
              "pca_frame_points")
    return (out, labels_out, meta) if want_meta else (out, labels_out)


class FrameLevel(NamedTuple):
    """One resolution of a multi-resolution point set (``frame_points_multires``): ``Nt`` frames of
    ``n_fft`` samples, ``hop`` apart, the first centred ``offset`` samples from the set's anchor, ``n_bins``
    bins each; ``farr`` float32 [n_bins] and ``tarr`` float32 [Nt] (None in every level: 2-D rows) on the
    device; ``win_lengths`` device int32, this level's window for each window index (None: [n_fft])."""
    n_fft: int
    hop: int
    n_bins: int
    Nt: int
    farr: torch.Tensor
    tarr: Optional[torch.Tensor] = None
    win_lengths: Optional[torch.Tensor] = None
    offset: int = 0


def frame_points_multires(waves: torch.Tensor, wave_off: torch.Tensor, set_off: torch.Tensor,
                          idx: torch.Tensor, levels: Sequence[FrameLevel], span: int, *, max_len: int,
                          min_len: int, clip_labels: Optional[torch.Tensor] = None, jitter: int = 0,
                          gain_db: float = 0.0, norm_mode: int = NORM_NFFT, seed: int = 0, draw: int = 0,
                          out: Optional[torch.Tensor] = None, labels_out: Optional[torch.Tensor] = None,
                          draw_dev: Optional[torch.Tensor] = None, want_meta: bool = False):
    """Batch of point sets that hold several STFT resolutions at once, framed from resident waveforms in
    ONE launch (pca_frame_points_multires): what one ``frame_points`` per level plus ``torch.cat`` gives,
    without the batch's second trip through memory and with one set of draws.

    waves / wave_off / idx / max_len / min_len / clip_labels / jitter / gain_db / norm_mode / seed / draw /
    draw_dev as ``frame_points``; set_off int64[n_clips + 1] the prefix sum of the sets per clip at ``span``
    samples a set.  Set s of a clip has its anchor at s * span + the slot's shift; frame j of a level is
    centred at anchor + level.offset + j * level.hop, clamped into the clip.  A slot draws one shift, one
    gain and one window INDEX for all its levels; every level's ``win_lengths`` has the same number of
    entries (``ValueError`` otherwise).  At most 4 levels, at most 16384 points a set.
    Returns (points [B, N, 2 or 3] float32 - the levels' rows back to back in the order given, point
    j * n_bins + f inside a level -, clip_labels of each slot's clip or None [, meta int32 [B, 8] = (clip,
    centre sample of level 0's frame 0, level 0's window length, bits of the fp32 gain, shift, window index,
    0, 0)])."""
    levels = [lv if isinstance(lv, FrameLevel) else FrameLevel(*lv) for lv in levels]
    if not 1 <= len(levels) <= _lib.FRAME_MAX_LEVELS:
        raise ValueError(f"frame_points_multires: {len(levels)} levels (1 .. {_lib.FRAME_MAX_LEVELS})")
    _need_cuda(waves, wave_off, set_off, idx)
    assert waves.dtype == torch.float32 and waves.is_contiguous()
    assert wave_off.dtype == set_off.dtype == idx.dtype == torch.int64
    assert wave_off.numel() == set_off.numel() >= 2
    three = [lv.tarr is not None for lv in levels]
    if any(three) != all(three):
        raise ValueError("frame_points_multires: tarr is given in every level or in none")
    din = 3 if three[0] else 2
    B = idx.numel()
    with torch.cuda.device(waves.device):
        wins = [torch.tensor([lv.n_fft], dtype=torch.int32, device=waves.device)
                if lv.win_lengths is None else lv.win_lengths for lv in levels]
        n_win = wins[0].numel()
        if any(w.numel() != n_win for w in wins) or n_win < 1:
            raise ValueError(f"frame_points_multires: every level needs the same number of window lengths, "
                             f"got {[w.numel() for w in wins]}")
        arr = (_lib.PcaFrameLevel * len(levels))()
        N = 0
        for lv, w, a in zip(levels, wins, arr):
            _need_cuda(lv.farr, w)
            assert lv.farr.dtype == torch.float32 and lv.farr.numel() >= lv.n_bins
            assert w.dtype == torch.int32 and w.is_contiguous()
            if lv.tarr is not None:
                _need_cuda(lv.tarr)
                assert lv.tarr.dtype == torch.float32 and lv.tarr.numel() >= lv.Nt
            a.n_fft, a.hop, a.n_bins, a.Nt, a.offset = (int(lv.n_fft), int(lv.hop), int(lv.n_bins),
                                                        int(lv.Nt), int(lv.offset))
            a.farr, a.tarr, a.win_lengths = lv.farr.data_ptr(), _ptr(lv.tarr), w.data_ptr()
            N += int(lv.Nt) * int(lv.n_bins)
        if out is None:
            out = torch.empty((B, N, din), dtype=torch.float32, device=waves.device)
        assert out.is_contiguous() and out.numel() == B * N * din
        if clip_labels is not None and labels_out is None:
            labels_out = torch.empty(B, dtype=torch.int64, device=waves.device)
        meta = torch.empty((B, 8), dtype=torch.int32, device=waves.device) if want_meta else None
        aug = _lib.PcaFrameAug(int(jitter), float(gain_db), None, n_win, int(norm_mode),
                               int(seed) & (2 ** 64 - 1), int(draw) & (2 ** 64 - 1), _draw_ptr(draw_dev))
        check(lib().pca_frame_points_multires(_ptr(waves), _ptr(wave_off), _ptr(set_off),
                                              wave_off.numel() - 1, int(max_len), int(min_len),
                                              _ptr(clip_labels), _ptr(idx), B, arr, len(levels), int(span),
                                              C.byref(aug), _ptr(out), _ptr(labels_out), _ptr(meta),
                                              _stream(waves)), "pca_frame_points_multires")
    return (out, labels_out, meta) if want_meta else (out, labels_out)


class FilterBank:
    """A bank of non-negative band filters over the ``n_fft/2 + 1`` bins of a frame, for
    ``frame_points_bands``: value of band m = log(amin + sum_k W[m, k] * |X[k]|^power).

    ``W`` float64 [n_bands, n_fft/2 + 1] on the host (anything ``numpy.asarray`` takes), ``centres`` the
    bands' centre frequencies in Hz [n_bands] (the datasets' frequency axis), ``power`` 1 (magnitude) or 2
    (power), ``amin`` > 0.  Packed once to the banded form of ``PcaFrameBands``: per band the span from its
    first to its last non-zero weight (as the device sees them: rounded to fp32), zeros inside the span
    kept; uploaded once per device.  ``ValueError`` for a wrong shape, a negative or non-finite weight and a
    band without a non-zero weight (the message names the band)."""

    def __init__(self, W, centres, power: int = 2, amin: float = 1e-8):
        W = np.asarray(W, dtype=np.float64)
        centres = np.asarray(centres, dtype=np.float64)
        if W.ndim != 2 or W.shape[0] < 1 or W.shape[1] < 2:
            raise ValueError(f"FilterBank: W of shape {W.shape}, expected [n_bands, n_fft/2 + 1]")
        n_fft = 2 * (W.shape[1] - 1)
        if n_fft & (n_fft - 1):
            raise ValueError(f"FilterBank: W has {W.shape[1]} columns, expected n_fft/2 + 1 for a power of "
                             "two n_fft")
        if centres.shape != (W.shape[0],):
            raise ValueError(f"FilterBank: centres of shape {centres.shape} for {W.shape[0]} bands")
        if not np.isfinite(W).all() or (W < 0).any():
            raise ValueError("FilterBank: a negative or non-finite weight")
        if not np.isfinite(centres).all():
            raise ValueError("FilterBank: a non-finite centre")
        w32 = W.astype(np.float32)
        if not np.isfinite(w32).all():
            raise ValueError("FilterBank: a weight beyond the fp32 range")
        lo, off, parts = [], [0], []
        for m in range(W.shape[0]):
            nz = np.flatnonzero(w32[m])
            if nz.size == 0:
                raise ValueError(f"FilterBank: band {m} has no non-zero weight (too many bands for "
                                 f"{W.shape[1]} bins?)")
            lo.append(int(nz[0]))
            parts.append(w32[m, nz[0]:nz[-1] + 1])
            off.append(off[-1] + parts[-1].size)
        self._init(np.asarray(lo, np.int32), np.asarray(off, np.int32), np.concatenate(parts), W.shape[1],
                   centres, power, amin)
        self.W = W                        # as given, in fp64; dense() is what the device applies

    def _init(self, band_lo, band_off, weights, n_src, centres, power, amin):
        power, amin = int(power), float(amin)
        if power not in (1, 2):
            raise ValueError(f"FilterBank: power {power} (1: magnitude, 2: power)")
        if not (0.0 < amin < float("inf")) or not float(np.float32(amin)) > 0.0:
            raise ValueError(f"FilterBank: amin {amin} must be finite and > 0 (in fp32)")
        self.band_lo, self.band_off, self.weights = band_lo, band_off, weights
        self.n_src, self.n_fft = int(n_src), 2 * (int(n_src) - 1)
        self.n_bands, self.nnz = int(band_lo.size), int(weights.size)
        self.centres, self.power, self.amin = centres, power, amin
        self._dev = {}

    @classmethod
    def from_packed(cls, band_lo, band_off, weights, n_src: int, centres=None, power: int = 2,
                    amin: float = 1e-8) -> "FilterBank":
        """A bank from its banded arrays, values unchecked (the launch clips every band's range into the
        frame's bins on the device): band_lo int32 [n_bands], band_off int32 [n_bands + 1], weights float32
        [nnz >= n_bands].  ``centres`` defaults to the band index."""
        band_lo = np.ascontiguousarray(band_lo, dtype=np.int32).reshape(-1)
        band_off = np.ascontiguousarray(band_off, dtype=np.int32).reshape(-1)
        weights = np.ascontiguousarray(weights, dtype=np.float32).reshape(-1)
        if band_lo.size < 1 or band_off.size != band_lo.size + 1 or weights.size < band_lo.size:
            raise ValueError(f"FilterBank.from_packed: {band_lo.size} bands, {band_off.size} offsets, "
                             f"{weights.size} weights")
        centres = (np.arange(band_lo.size, dtype=np.float64) if centres is None
                   else np.asarray(centres, dtype=np.float64))
        if centres.shape != (band_lo.size,):
            raise ValueError(f"FilterBank.from_packed: centres of shape {centres.shape}")
        self = cls.__new__(cls)
        self._init(band_lo, band_off, weights, n_src, centres, power, amin)
        self.W = self.dense()
        return self

    def dense(self) -> "np.ndarray":
        """The bank as the device applies it: float64 [n_bands, n_src] from the packed fp32 weights, every
        band clipped into the bins as the launch clips it."""
        W = np.zeros((self.n_bands, self.n_src), dtype=np.float64)
        for m in range(self.n_bands):
            o0 = min(max(int(self.band_off[m]), 0), self.nnz)
            o1 = min(max(int(self.band_off[m + 1]), o0), self.nnz)
            lo = int(self.band_lo[m])
            for i in range(max(-lo, 0), min(o1 - o0, self.n_src - lo)):
                W[m, lo + i] = float(self.weights[o0 + i])
        return W

    def summary(self) -> dict:
        return {"n_bands": self.n_bands, "power": self.power, "amin": self.amin, "nnz": self.nnz}

    def on(self, device) -> "_lib.PcaFrameBands":
        """The C struct with the arrays on ``device`` (uploaded on first use, kept for the bank's life)."""
        device = torch.device(device)
        if device.type == "cuda" and device.index is None:
            device = torch.device("cuda", torch.cuda.current_device())
        if device not in self._dev:
            if device.type != "cuda":
                raise _lib.PcaHipError("FilterBank.on: a bank is applied on the device (no CPU fallback)")
            self._dev[device] = tuple(torch.from_numpy(a).to(device)
                                      for a in (self.band_lo, self.band_off, self.weights))
        lo, off, w = self._dev[device]
        return _lib.PcaFrameBands(self.n_bands, self.nnz, lo.data_ptr(), off.data_ptr(), w.data_ptr(),
                                  self.power, self.amin)


def _hz_to_mel(f, htk: bool):
    f = np.asarray(f, dtype=np.float64)
    if htk:
        return 2595.0 * np.log10(1.0 + f / 700.0)
    lin = f / (200.0 / 3.0)
    with np.errstate(divide="ignore"):
        log = 15.0 + np.log(np.maximum(f, 1e-300) / 1000.0) / (math.log(6.4) / 27.0)
    return np.where(f >= 1000.0, log, lin)


def _mel_to_hz(m, htk: bool):
    m = np.asarray(m, dtype=np.float64)
    if htk:
        return 700.0 * (10.0 ** (m / 2595.0) - 1.0)
    return np.where(m >= 15.0, 1000.0 * np.exp((math.log(6.4) / 27.0) * (m - 15.0)), m * (200.0 / 3.0))


def mel_bank(fs: float, n_fft: int, n_mels: int, fmin: float = 0.0, fmax: Optional[float] = None,
             htk: bool = False, norm: Optional[str] = "slaney", power: int = 2,
             amin: float = 1e-8) -> FilterBank:
    """Triangular mel filters as a ``FilterBank``, in the form of ``librosa.filters.mel`` (written from the
    published formulae; parity with librosa itself is not pinned by a test: it is not a dependency).

    Slaney scale (default): mel = f / (200/3) below 1000 Hz, 15 + ln(f / 1000) / (ln(6.4) / 27) from there;
    ``htk``: 2595 log10(1 + f / 700).  ``n_mels + 2`` points p equally spaced in mel between ``fmin`` and
    ``fmax`` (None: fs / 2), mapped back to Hz; band i is the triangle
    max(0, min((f_k - p_i) / (p_i+1 - p_i), (p_i+2 - f_k) / (p_i+2 - p_i+1))) over f_k = k fs / n_fft,
    times 2 / (p_i+2 - p_i) with ``norm="slaney"`` (None: peaks of up to 1).  ``centres`` = p_i+1.
    ``ValueError`` when a band falls between two bins (no non-zero weight): fewer bands or a longer frame."""
    n_fft, n_mels = int(n_fft), int(n_mels)
    if n_mels < 1:
        raise ValueError(f"mel_bank: n_mels {n_mels}")
    if norm not in (None, "slaney"):
        raise ValueError(f"mel_bank: norm {norm!r} (None or 'slaney')")
    fmax = float(fs) / 2.0 if fmax is None else float(fmax)
    if not 0.0 <= float(fmin) < fmax <= float(fs) / 2.0 + 1e-9:
        raise ValueError(f"mel_bank: fmin {fmin}, fmax {fmax} outside 0 <= fmin < fmax <= fs/2")
    pts = _mel_to_hz(np.linspace(float(_hz_to_mel(fmin, htk)), float(_hz_to_mel(fmax, htk)), n_mels + 2), htk)
    fk = np.arange(n_fft // 2 + 1, dtype=np.float64) * (float(fs) / n_fft)
    d = np.diff(pts)
    lower = (fk[None, :] - pts[:-2, None]) / d[:-1, None]
    upper = (pts[2:, None] - fk[None, :]) / d[1:, None]
    W = np.maximum(0.0, np.minimum(lower, upper))
    if norm == "slaney":
        W = W * (2.0 / (pts[2:] - pts[:-2]))[:, None]
    return FilterBank(W, pts[1:-1], power=power, amin=amin)


def frame_points_bands(waves: torch.Tensor, wave_off: torch.Tensor, set_off: torch.Tensor,
                       idx: torch.Tensor, n_fft: int, hop: int, bank: FilterBank, farr: torch.Tensor,
                       tarr: Optional[torch.Tensor] = None, Nt: int = 1, *, max_len: int, min_len: int,
                       clip_labels: Optional[torch.Tensor] = None, jitter: int = 0,
                       gain_db: float = 0.0, win_lengths: Optional[torch.Tensor] = None,
                       norm_mode: int = NORM_NFFT, seed: int = 0, draw: int = 0,
                       out: Optional[torch.Tensor] = None, labels_out: Optional[torch.Tensor] = None,
                       draw_dev: Optional[torch.Tensor] = None, want_meta: bool = False):
    """``frame_points`` with the bins of every frame summed into the bands of ``bank`` inside the launch
    (pca_frame_points_bands): log-mel and other filter-bank point sets, one point per band.

    Every argument of ``frame_points`` with the same meaning (``n_bins`` is ``bank.n_bands``); ``farr``
    float32 [n_bands] on the device is the band axis.  Slot b's clip, shift, gain and window are
    ``frame_points``' for the same arguments, and so are the labels and meta; the value of band m is
    logf(amin + sum_k W[m, k] * |X[k]|^power), the sum in fp64 in an order the bank alone fixes.
    Returns (points [B, Nt * n_bands, 2 or 3] float32, labels or None [, meta int32 [B, 4]])."""
    if not isinstance(bank, FilterBank):
        raise TypeError(f"frame_points_bands: bank is a {type(bank).__name__}, expected a FilterBank")
    if bank.n_src != int(n_fft) // 2 + 1:
        raise ValueError(f"frame_points_bands: the bank covers {bank.n_src} bins, n_fft {n_fft} has "
                         f"{int(n_fft) // 2 + 1}")
    _need_cuda(waves, wave_off, set_off, idx, farr)
    assert waves.dtype == torch.float32 and waves.is_contiguous() and farr.dtype == torch.float32
    assert wave_off.dtype == set_off.dtype == idx.dtype == torch.int64
    assert wave_off.numel() == set_off.numel() >= 2 and farr.numel() >= bank.n_bands
    din = 2
    if tarr is not None:
        _need_cuda(tarr)
        assert tarr.dtype == torch.float32 and tarr.numel() >= Nt
        din = 3
    B = idx.numel()
    with torch.cuda.device(waves.device):
        if win_lengths is None:
            win_lengths = torch.tensor([n_fft], dtype=torch.int32, device=waves.device)
        assert win_lengths.is_cuda and win_lengths.dtype == torch.int32
        if out is None:
            out = torch.empty((B, Nt * bank.n_bands, din), dtype=torch.float32, device=waves.device)
        assert out.is_contiguous() and out.numel() == B * Nt * bank.n_bands * din
        if clip_labels is not None and labels_out is None:
            labels_out = torch.empty(B, dtype=torch.int64, device=waves.device)
        meta = torch.empty((B, 4), dtype=torch.int32, device=waves.device) if want_meta else None
        aug = _lib.PcaFrameAug(int(jitter), float(gain_db), win_lengths.data_ptr(),
                               win_lengths.numel(), int(norm_mode), int(seed) & (2 ** 64 - 1),
                               int(draw) & (2 ** 64 - 1), _draw_ptr(draw_dev))
        bands = bank.on(waves.device)
        check(lib().pca_frame_points_bands(_ptr(waves), _ptr(wave_off), _ptr(set_off),
                                           wave_off.numel() - 1, int(max_len), int(min_len),
                                           _ptr(clip_labels), _ptr(idx), B, int(n_fft), int(hop), int(Nt),
                                           _ptr(farr), _ptr(tarr), C.byref(aug), C.byref(bands),
                                           _ptr(out), _ptr(labels_out), _ptr(meta), _stream(waves)),
              "pca_frame_points_bands")
    return (out, labels_out, meta) if want_meta else (out, labels_out)


class Pcen:
    """Per-channel energy normalisation of band energies, for ``frame_points_pcen`` and the datasets'
    ``pcen=``: ``librosa.pcen``'s parameters (Wang et al. 2017; Lostanlen et al. 2019) as an immutable spec.

        M[0] = x[0];  M[u] = (1 - s) M[u-1] + s x[u];   y = (bias + x / (eps + M)^gain)^power - bias^power

    with x = ``scale`` * the band energy.  ``context`` frames of history before each set feed the smoother
    (its truncation error falls as (1 - s)^context; every frame of context is one more frame transform per
    set).  ``s`` is given, or follows from ``time_constant`` (seconds) by ``coefficient(fs, hop)``.  Parity
    with librosa is by formula and not pinned by a test: it is not a dependency.  ``ValueError`` outside
    context [0, 255], s (0, 1], gain [0, 4], bias [0, 1e6], power (0, 1], eps > 0, scale > 0,
    time_constant > 0 (the launch's rules)."""

    __slots__ = ("context", "time_constant", "gain", "bias", "power", "eps", "scale", "s")

    def __init__(self, context: int = 32, time_constant: float = 0.4, gain: float = 0.98, bias: float = 2.0,
                 power: float = 0.5, eps: float = 1e-6, scale: float = 1.0, s: Optional[float] = None):
        v = dict(context=int(context), time_constant=float(time_constant), gain=float(gain), bias=float(bias),
                 power=float(power), eps=float(eps), scale=float(scale), s=None if s is None else float(s))

        def fin(a):                       # finite and > 0 as the fp32 the launch gets
            with np.errstate(over="ignore"):
                return 0.0 < float(np.float32(a)) < float("inf")

        if not 0 <= v["context"] <= 255:
            raise ValueError(f"Pcen: context {context} outside [0, 255]")
        if v["s"] is None and not 0.0 < v["time_constant"] < float("inf"):
            raise ValueError(f"Pcen: time_constant {time_constant} must be finite and > 0")
        if v["s"] is not None and not 0.0 < float(np.float32(v["s"])) <= 1.0:
            raise ValueError(f"Pcen: s {s} outside (0, 1]")
        if not 0.0 <= v["gain"] <= 4.0:
            raise ValueError(f"Pcen: gain {gain} outside [0, 4]")
        if not 0.0 <= v["bias"] <= 1e6:
            raise ValueError(f"Pcen: bias {bias} outside [0, 1e6]")
        if not 0.0 < float(np.float32(v["power"])) <= 1.0:
            raise ValueError(f"Pcen: power {power} outside (0, 1]")
        if not fin(v["eps"]):
            raise ValueError(f"Pcen: eps {eps} must be finite and > 0 (in fp32)")
        if not fin(v["scale"]):
            raise ValueError(f"Pcen: scale {scale} must be finite and > 0 (in fp32)")
        for k, x in v.items():
            object.__setattr__(self, k, x)

    def __setattr__(self, k, x):
        raise AttributeError("Pcen is immutable")

    def __repr__(self):
        return "Pcen(" + ", ".join(f"{k}={getattr(self, k)!r}" for k in self.__slots__) + ")"

    def _key(self):
        return tuple(getattr(self, k) for k in self.__slots__)

    def __eq__(self, other):
        return isinstance(other, Pcen) and self._key() == other._key()

    def __hash__(self):
        return hash(self._key())

    def coefficient(self, fs: float, hop: int) -> float:
        """The smoother's coefficient: ``s`` when given, else librosa's (sqrt(1 + 4 t^2) - 1) / (2 t^2) with
        t = time_constant * fs / hop frames."""
        if self.s is not None:
            return self.s
        t = self.time_constant * float(fs) / float(hop)
        return (math.sqrt(1.0 + 4.0 * t * t) - 1.0) / (2.0 * t * t)

    def summary(self) -> dict:
        return {k: getattr(self, k) for k in self.__slots__}

    def struct(self, fs: float, hop: int) -> "_lib.PcaPcen":
        return _lib.PcaPcen(self.context, self.coefficient(fs, hop), self.gain, self.bias, self.power, self.eps,
                            self.scale)


_PCEN_WS = {}     # (device, B, T, n_bands) -> (energy float64 [B, T, n_bands], tickets int32 [B], all zero)


def pcen_workspace(device, B: int, T: int, n_bands: int):
    """The launch's workspace, kept per (device, B, T, n_bands): the tickets are zeroed once, here - every
    launch leaves them zero.  Launches that share it run one after the other (one stream); callers that
    overlap launches pass workspaces of their own.  Under stream capture nothing is kept: a first use
    inside a capture gets tensors of the graph's own pool, zeroed by a node of that graph."""
    device = torch.device(device)
    if device.index is None:
        device = torch.device("cuda", torch.cuda.current_device())
    key = (device, int(B), int(T), int(n_bands))
    held = _PCEN_WS.get(key)
    if held is None:
        held = (torch.empty((B, T, n_bands), dtype=torch.float64, device=device),
                torch.zeros(B, dtype=torch.int32, device=device))
        if not torch.cuda.is_current_stream_capturing():
            _PCEN_WS[key] = held
    return held


def frame_points_pcen(waves: torch.Tensor, wave_off: torch.Tensor, set_off: torch.Tensor,
                      idx: torch.Tensor, n_fft: int, hop: int, bank: FilterBank, farr: torch.Tensor,
                      tarr: Optional[torch.Tensor] = None, Nt: int = 1, *, pcen: Pcen, fs: float,
                      max_len: int, min_len: int, clip_labels: Optional[torch.Tensor] = None,
                      jitter: int = 0, gain_db: float = 0.0, win_lengths: Optional[torch.Tensor] = None,
                      norm_mode: int = NORM_NFFT, seed: int = 0, draw: int = 0,
                      out: Optional[torch.Tensor] = None, labels_out: Optional[torch.Tensor] = None,
                      draw_dev: Optional[torch.Tensor] = None, want_meta: bool = False,
                      workspace: Optional[Tuple[torch.Tensor, torch.Tensor]] = None):
    """``frame_points_bands`` with per-channel energy normalisation in place of the log
    (pca_frame_points_pcen): every argument of ``frame_points_bands`` with the same meaning - the clip,
    shift, gain, window, labels and meta of slot b are that launch's bits - plus ``pcen``, a ``Pcen``, and
    ``fs`` (``Pcen.coefficient(fs, hop)`` turns its time constant into the smoother's coefficient).  The
    value of band m in frame j is (bias + x / (eps + M)^gain)^power - bias^power with x = scale * the band
    launch's fp64 band sum and M its smoothed history over ``pcen.context`` frames before the set and the
    set's own; ``bank.amin`` is not used.  One launch over context + Nt frames per slot.

    ``workspace``: (energy float64 with >= B * (context + Nt) * n_bands elements, tickets int32 [>= B], ZERO)
    on the device, for callers that overlap launches; None: ``pcen_workspace``'s, kept per shape.
    Returns (points [B, Nt * n_bands, 2 or 3] float32, labels or None [, meta int32 [B, 4]])."""
    if not isinstance(bank, FilterBank):
        raise TypeError(f"frame_points_pcen: bank is a {type(bank).__name__}, expected a FilterBank")
    if not isinstance(pcen, Pcen):
        raise TypeError(f"frame_points_pcen: pcen is a {type(pcen).__name__}, expected a Pcen")
    if bank.n_src != int(n_fft) // 2 + 1:
        raise ValueError(f"frame_points_pcen: the bank covers {bank.n_src} bins, n_fft {n_fft} has "
                         f"{int(n_fft) // 2 + 1}")
    _need_cuda(waves, wave_off, set_off, idx, farr)
    assert waves.dtype == torch.float32 and waves.is_contiguous() and farr.dtype == torch.float32
    assert wave_off.dtype == set_off.dtype == idx.dtype == torch.int64
    assert wave_off.numel() == set_off.numel() >= 2 and farr.numel() >= bank.n_bands
    din = 2
    if tarr is not None:
        _need_cuda(tarr)
        assert tarr.dtype == torch.float32 and tarr.numel() >= Nt
        din = 3
    B = idx.numel()
    T = pcen.context + int(Nt)
    with torch.cuda.device(waves.device):
        if win_lengths is None:
            win_lengths = torch.tensor([n_fft], dtype=torch.int32, device=waves.device)
        assert win_lengths.is_cuda and win_lengths.dtype == torch.int32
        if out is None:
            out = torch.empty((B, Nt * bank.n_bands, din), dtype=torch.float32, device=waves.device)
        assert out.is_contiguous() and out.numel() == B * Nt * bank.n_bands * din
        if clip_labels is not None and labels_out is None:
            labels_out = torch.empty(B, dtype=torch.int64, device=waves.device)
        meta = torch.empty((B, 4), dtype=torch.int32, device=waves.device) if want_meta else None
        energy, tickets = pcen_workspace(waves.device, B, T, bank.n_bands) if workspace is None else workspace
        _need_cuda(energy, tickets)
        assert energy.dtype == torch.float64 and energy.is_contiguous()
        assert tickets.dtype == torch.int32 and tickets.is_contiguous() and tickets.numel() >= B
        aug = _lib.PcaFrameAug(int(jitter), float(gain_db), win_lengths.data_ptr(),
                               win_lengths.numel(), int(norm_mode), int(seed) & (2 ** 64 - 1),
                               int(draw) & (2 ** 64 - 1), _draw_ptr(draw_dev))
        bands = bank.on(waves.device)
        spec = pcen.struct(fs, hop)
        check(lib().pca_frame_points_pcen(_ptr(waves), _ptr(wave_off), _ptr(set_off),
                                          wave_off.numel() - 1, int(max_len), int(min_len),
                                          _ptr(clip_labels), _ptr(idx), B, int(n_fft), int(hop), int(Nt),
                                          _ptr(farr), _ptr(tarr), C.byref(aug), C.byref(bands),
                                          C.byref(spec), _ptr(energy), energy.numel(), _ptr(tickets),
                                          _ptr(out), _ptr(labels_out), _ptr(meta), _stream(waves)),
              "pca_frame_points_pcen")
    return (out, labels_out, meta) if want_meta else (out, labels_out)


DELTA_AXES = {"t": 1, "f": 2, "tf": 3}


class Deltas:
    """Regression deltas of a point set's value column as further point columns, for ``frame_points_delta``
    and the datasets' ``deltas=``: an immutable spec.

        dt[j][m] = sum_{n=1..W} n (v[j+n][m] - v[j-n][m]) / (2 sum n^2)      along the frames
        df[j][m] = sum_{n=1..W} n (v[j][m+n] - v[j][m-n]) / (2 sum n^2)      along the rows, edges replicated

    ``axes``: "t", "f" or "tf" (dt, then df); ``width``: W in 1..4.  A time delta reads ``width`` context frames
    before and after each set (frames outside the clip repeat its end frames): ``2 * width`` more frame
    transforms per set.  ``ValueError`` for anything else (the launch's rules)."""

    __slots__ = ("axes", "width")

    def __init__(self, axes: str = "t", width: int = 2):
        if not isinstance(axes, str) or axes not in DELTA_AXES:
            raise ValueError(f"Deltas: axes {axes!r} is not one of {sorted(DELTA_AXES)}")
        if isinstance(width, bool) or width not in (1, 2, 3, 4):
            raise ValueError(f"Deltas: width {width!r} outside 1..4")
        object.__setattr__(self, "axes", axes)
        object.__setattr__(self, "width", int(width))

    def __setattr__(self, k, x):
        raise AttributeError("Deltas is immutable")

    def __repr__(self):
        return f"Deltas(axes={self.axes!r}, width={self.width})"

    def _key(self):
        return (self.axes, self.width)

    def __eq__(self, other):
        return isinstance(other, Deltas) and self._key() == other._key()

    def __hash__(self):
        return hash(self._key())

    @property
    def count(self) -> int:
        """How many columns the spec adds to a point."""
        return len(self.axes)

    @property
    def context(self) -> int:
        """Context frames before, and after, each set: ``width`` with a time delta, else 0."""
        return self.width if "t" in self.axes else 0

    def summary(self) -> dict:
        return {"axes": self.axes, "width": self.width}

    def struct(self) -> "_lib.PcaDelta":
        return _lib.PcaDelta(DELTA_AXES[self.axes], self.width)


_DELTA_WS = {}    # (device, B, T, F) -> (values float32 [B, T, F], tickets int32 [B], all zero)


def delta_workspace(device, B: int, T: int, F: int):
    """The launch's workspace, kept per (device, B, T, F), as ``pcen_workspace``: the tickets are zeroed once,
    here - every launch leaves them zero.  Launches that share it run one after the other (one stream);
    callers that overlap launches pass workspaces of their own.  Under stream capture nothing is kept."""
    device = torch.device(device)
    if device.index is None:
        device = torch.device("cuda", torch.cuda.current_device())
    key = (device, int(B), int(T), int(F))
    held = _DELTA_WS.get(key)
    if held is None:
        held = (torch.empty((B, T, F), dtype=torch.float32, device=device),
                torch.zeros(B, dtype=torch.int32, device=device))
        if not torch.cuda.is_current_stream_capturing():
            _DELTA_WS[key] = held
    return held


def frame_points_delta(waves: torch.Tensor, wave_off: torch.Tensor, set_off: torch.Tensor,
                       idx: torch.Tensor, n_fft: int, hop: int, n_bins: int, farr: torch.Tensor,
                       tarr: Optional[torch.Tensor] = None, Nt: int = 1, *, deltas: Deltas,
                       bank: Optional[FilterBank] = None, max_len: int, min_len: int,
                       clip_labels: Optional[torch.Tensor] = None, jitter: int = 0, gain_db: float = 0.0,
                       win_lengths: Optional[torch.Tensor] = None, norm_mode: int = NORM_NFFT, seed: int = 0,
                       draw: int = 0, out: Optional[torch.Tensor] = None,
                       labels_out: Optional[torch.Tensor] = None, draw_dev: Optional[torch.Tensor] = None,
                       want_meta: bool = False,
                       workspace: Optional[Tuple[torch.Tensor, torch.Tensor]] = None):
    """``frame_points`` (``bank`` None) or ``frame_points_bands`` (a ``FilterBank``) with regression deltas of
    the value column as further columns (pca_frame_points_delta): every argument of those with the same
    meaning - the coordinates, the value column, labels and meta of slot b are that launch's bits - plus
    ``deltas``, a ``Deltas``.  A frame has F rows: ``n_bins``, or ``bank.n_bands`` (``n_bins`` is then not
    used).  Rows are (f, [t,] value, dt and / or df in the order of ``deltas.axes``); din = 2 or 3 plus
    ``deltas.count`` is at most 4, so a set with ``tarr`` takes one axis.  One launch over
    Nt + 2 * ``deltas.context`` frames per slot.

    ``workspace``: (values float32 with >= B * (Nt + 2 * context) * F elements, tickets int32 [>= B], ZERO) on
    the device, for callers that overlap launches or read the values back; None: ``delta_workspace``'s, kept
    per shape.
    Returns (points [B, Nt * F, din] float32, labels or None [, meta int32 [B, 4]])."""
    if not isinstance(deltas, Deltas):
        raise TypeError(f"frame_points_delta: deltas is a {type(deltas).__name__}, expected a Deltas")
    if bank is not None:
        if not isinstance(bank, FilterBank):
            raise TypeError(f"frame_points_delta: bank is a {type(bank).__name__}, expected a FilterBank or None")
        if bank.n_src != int(n_fft) // 2 + 1:
            raise ValueError(f"frame_points_delta: the bank covers {bank.n_src} bins, n_fft {n_fft} has "
                             f"{int(n_fft) // 2 + 1}")
    F = int(n_bins) if bank is None else bank.n_bands
    _need_cuda(waves, wave_off, set_off, idx, farr)
    assert waves.dtype == torch.float32 and waves.is_contiguous() and farr.dtype == torch.float32
    assert wave_off.dtype == set_off.dtype == idx.dtype == torch.int64
    assert wave_off.numel() == set_off.numel() >= 2 and farr.numel() >= F
    din = 2
    if tarr is not None:
        _need_cuda(tarr)
        assert tarr.dtype == torch.float32 and tarr.numel() >= Nt
        din = 3
    din += deltas.count
    if din > 4:
        raise ValueError(f"frame_points_delta: Deltas {deltas.axes!r} on 3-D sets gives din {din} (max 4: one "
                         f"axis)")
    B = idx.numel()
    T = int(Nt) + 2 * deltas.context
    with torch.cuda.device(waves.device):
        if win_lengths is None:
            win_lengths = torch.tensor([n_fft], dtype=torch.int32, device=waves.device)
        assert win_lengths.is_cuda and win_lengths.dtype == torch.int32
        if out is None:
            out = torch.empty((B, Nt * F, din), dtype=torch.float32, device=waves.device)
        assert out.is_contiguous() and out.numel() == B * Nt * F * din
        if clip_labels is not None and labels_out is None:
            labels_out = torch.empty(B, dtype=torch.int64, device=waves.device)
        meta = torch.empty((B, 4), dtype=torch.int32, device=waves.device) if want_meta else None
        values, tickets = delta_workspace(waves.device, B, T, F) if workspace is None else workspace
        _need_cuda(values, tickets)
        assert values.dtype == torch.float32 and values.is_contiguous()
        assert tickets.dtype == torch.int32 and tickets.is_contiguous() and tickets.numel() >= B
        aug = _lib.PcaFrameAug(int(jitter), float(gain_db), win_lengths.data_ptr(),
                               win_lengths.numel(), int(norm_mode), int(seed) & (2 ** 64 - 1),
                               int(draw) & (2 ** 64 - 1), _draw_ptr(draw_dev))
        bands = None if bank is None else C.byref(bank.on(waves.device))
        spec = deltas.struct()
        check(lib().pca_frame_points_delta(_ptr(waves), _ptr(wave_off), _ptr(set_off),
                                           wave_off.numel() - 1, int(max_len), int(min_len),
                                           _ptr(clip_labels), _ptr(idx), B, int(n_fft), int(hop),
                                           int(n_bins) if bank is None else int(n_fft) // 2 + 1, int(Nt),
                                           _ptr(farr), _ptr(tarr), C.byref(aug), bands, C.byref(spec),
                                           _ptr(values), values.numel(), _ptr(tickets), _ptr(out),
                                           _ptr(labels_out), _ptr(meta), _stream(waves)),
              "pca_frame_points_delta")
    return (out, labels_out, meta) if want_meta else (out, labels_out)


REASSIGN_AXES = {"f": 1, "t": 2, "ft": 3, "tf": 3}


def reassign_spec(axes: str = "f", rel_floor: float = math.log(1e3), abs_floor: float = float("-inf"),
                  max_df: float = 2.0, max_dt: float = 1.0, strength: float = 1.0) -> "_lib.PcaReassignSpec":
    """``PcaReassignSpec`` checked on the host by the rules of pca_frame_points_reassigned
    (``ValueError``)."""
    if axes not in REASSIGN_AXES:
        raise ValueError(f"axes {axes!r}: one of 'f', 't', 'ft'")
    rel_floor, abs_floor = float(rel_floor), float(abs_floor)
    max_df, max_dt, strength = float(max_df), float(max_dt), float(strength)
    if not rel_floor >= 0.0:
        raise ValueError(f"rel_floor {rel_floor}: >= 0 (inf switches it off)")
    if abs_floor != abs_floor:
        raise ValueError("abs_floor is NaN (-inf switches it off)")
    if not 0.0 < max_df <= 64.0:
        raise ValueError(f"max_df {max_df} outside (0, 64] bins")
    if not 0.0 < max_dt <= 4.0:
        raise ValueError(f"max_dt {max_dt} outside (0, 4] frames")
    if not 0.0 <= strength <= 1.0:
        raise ValueError(f"strength {strength} outside [0, 1]")
    return _lib.PcaReassignSpec(REASSIGN_AXES[axes], rel_floor, abs_floor, max_df, max_dt, strength)


def frame_points_reassigned(waves: torch.Tensor, wave_off: torch.Tensor, set_off: torch.Tensor,
                            idx: torch.Tensor, n_fft: int, hop: int, n_bins: int, farr: torch.Tensor,
                            tarr: Optional[torch.Tensor] = None, Nt: int = 1, *, max_len: int,
                            min_len: int, clip_labels: Optional[torch.Tensor] = None, jitter: int = 0,
                            gain_db: float = 0.0, win_lengths: Optional[torch.Tensor] = None,
                            norm_mode: int = NORM_NFFT, seed: int = 0, draw: int = 0,
                            axes: str = "f", rel_floor: float = math.log(1e3),
                            abs_floor: float = float("-inf"), max_df: float = 2.0, max_dt: float = 1.0,
                            strength: float = 1.0, out: Optional[torch.Tensor] = None,
                            labels_out: Optional[torch.Tensor] = None,
                            draw_dev: Optional[torch.Tensor] = None, want_meta: bool = False):
    """``frame_points`` with every point written where its energy lies (pca_frame_points_reassigned):
    time-frequency reassignment in the form of ``librosa.reassigned_spectrogram``.  The value column,
    the labels and meta are ``frame_points``' bits for the same arguments; the coordinates become
    real-valued.

    Every argument of ``frame_points`` with the same meaning, plus: ``axes`` "f" (frequency), "t" (time;
    needs tarr and Nt >= 2) or "ft"; a bin moves iff its value is at least the frame's maximum minus
    ``rel_floor`` (inf: off) and at least ``abs_floor`` (-inf: off); the frequency shift is clamped to
    +-``max_df`` bins (0 < . <= 64), the time shift to +-``max_dt`` frames (0 < . <= 4), and both are
    then multiplied by ``strength`` in [0, 1] (0: the grid rows, bit for bit).  The moved frequency is
    piecewise-linear on ``farr``, the moved time on ``tarr`` (extrapolated with the edge spacing).
    n_bins >= 2.  Argument errors raise ``ValueError`` before any launch.
    Returns what ``frame_points`` returns."""
    spec = reassign_spec(axes, rel_floor, abs_floor, max_df, max_dt, strength)
    if int(n_bins) < 2:
        raise ValueError(f"n_bins {n_bins}: the frequency axis is interpolated, at least 2 bins")
    if spec.axes & 2 and (tarr is None or int(Nt) < 2):
        raise ValueError(f"axes {axes!r}: the time axis needs tarr and Nt >= 2 (Nt = {Nt})")
    _need_cuda(waves, wave_off, set_off, idx, farr)
    assert waves.dtype == torch.float32 and waves.is_contiguous() and farr.dtype == torch.float32
    assert wave_off.dtype == set_off.dtype == idx.dtype == torch.int64
    assert wave_off.numel() == set_off.numel() >= 2 and farr.numel() >= n_bins
    din = 2
    if tarr is not None:
        _need_cuda(tarr)
        assert tarr.dtype == torch.float32 and tarr.numel() >= Nt
        din = 3
    B = idx.numel()
    with torch.cuda.device(waves.device):
        if win_lengths is None:
            win_lengths = torch.tensor([n_fft], dtype=torch.int32, device=waves.device)
        assert win_lengths.is_cuda and win_lengths.dtype == torch.int32
        if out is None:
            out = torch.empty((B, Nt * n_bins, din), dtype=torch.float32, device=waves.device)
        if clip_labels is not None and labels_out is None:
            labels_out = torch.empty(B, dtype=torch.int64, device=waves.device)
        meta = torch.empty((B, 4), dtype=torch.int32, device=waves.device) if want_meta else None
        aug = _lib.PcaFrameAug(int(jitter), float(gain_db), win_lengths.data_ptr(),
                               win_lengths.numel(), int(norm_mode), int(seed) & (2 ** 64 - 1),
                               int(draw) & (2 ** 64 - 1), _draw_ptr(draw_dev))
        check(lib().pca_frame_points_reassigned(
            _ptr(waves), _ptr(wave_off), _ptr(set_off), wave_off.numel() - 1, int(max_len),
            int(min_len), _ptr(clip_labels), _ptr(idx), B, int(n_fft), int(hop), int(n_bins), int(Nt),
            _ptr(farr), _ptr(tarr), C.byref(aug), C.byref(spec), _ptr(out), _ptr(labels_out),
            _ptr(meta), _stream(waves)), "pca_frame_points_reassigned")
    return (out, labels_out, meta) if want_meta else (out, labels_out)


def clip_rms(waves: torch.Tensor, wave_off: torch.Tensor, max_len: int) -> torch.Tensor:
    """Root mean square of every clip of a corpus on the device (pca_clip_rms): waves float32, the
    clips back to back, wave_off int64[n_clips + 1] their offsets, max_len the longest one.  Returns
    float64[n_clips], fp64 sums in a fixed order (bit-reproducible); an empty clip gives 0."""
    _need_cuda(waves, wave_off)
    assert waves.dtype == torch.float32 and waves.is_contiguous()
    assert wave_off.dtype == torch.int64 and wave_off.is_contiguous() and wave_off.numel() >= 2
    n = wave_off.numel() - 1
    with torch.cuda.device(waves.device):
        out = torch.empty(n, dtype=torch.float64, device=waves.device)
        check(lib().pca_clip_rms(_ptr(waves), _ptr(wave_off), n, int(max_len), _ptr(out),
                                 _stream(waves)), "pca_clip_rms")
    return out


_speed_tables = {}


def _speed_filter(ratios, device):
    """The filter tables of pca_frame_points_ex: float64 [n_speed, 2, nwin] (win, delta) of
    ``_resample_filter``, one pair per ratio (zeros for a ratio of 1.0: never read), cached per
    (ratios, device).  Returns (tables or None when every ratio is 1.0, nwin, num_table)."""
    key = (tuple(ratios), str(device))
    if key not in _speed_tables:
        if all(r == 1.0 for r in ratios):
            _speed_tables[key] = (None, 0, 0)
        else:
            pairs, num_table = {}, 0
            for r in ratios:
                if r != 1.0:
                    win, delta, num_table = _resample_filter(r, device, dict(KAISER_FAST))
                    pairs[r] = torch.stack([win, delta])
            nwin = next(iter(pairs.values())).shape[1]
            zero = torch.zeros((2, nwin), dtype=torch.float64, device=device)
            tables = torch.stack([pairs.get(r, zero) for r in ratios]).contiguous()
            _speed_tables[key] = (tables, nwin, num_table)
    return _speed_tables[key]


def frame_points_ex(waves: torch.Tensor, wave_off: torch.Tensor, set_off: torch.Tensor,
                    idx: torch.Tensor, n_fft: int, hop: int, n_bins: int, farr: torch.Tensor,
                    tarr: Optional[torch.Tensor] = None, Nt: int = 1, *, max_len: int, min_len: int,
                    clip_labels: Optional[torch.Tensor] = None, jitter: int = 0,
                    gain_db: float = 0.0, win_lengths: Optional[torch.Tensor] = None,
                    norm_mode: int = NORM_NFFT, seed: int = 0, draw: int = 0,
                    ratios=(1.0,), clip_rms: Optional[torch.Tensor] = None,
                    bg_waves: Optional[torch.Tensor] = None, bg_off: Optional[torch.Tensor] = None,
                    bg_rms: Optional[torch.Tensor] = None, bg_max_len: int = 0,
                    mix_prob: float = 0.0, mix_snr_db=(0.0, 0.0),
                    out: Optional[torch.Tensor] = None, labels_out: Optional[torch.Tensor] = None,
                    draw_dev: Optional[torch.Tensor] = None, want_meta: bool = False,
                    want_samples: bool = False, bg_labels: Optional[torch.Tensor] = None,
                    labels2_out: Optional[torch.Tensor] = None,
                    weight_out: Optional[torch.Tensor] = None, _mask=None):
    """``frame_points`` with a speed change and a background mix applied while the frame is loaded
    (pca_frame_points_ex); the arguments they share mean the same, and with ``ratios == (1.0,)`` and
    ``mix_prob == 0`` (or no ``bg_waves``) the points, labels and meta[:, :4] are ``frame_points``' bits.

    ratios      up to 8 resampling ratios (new length / old length = 1 / playback speed), each in
                [0.5, 2.0]; one per batch slot, uniformly.  The resampler is ``pca_hip.resample``'s
                (kaiser_fast), evaluated for the samples the frame needs.
    bg_waves / bg_off int64[n_bg + 1] / bg_rms float64[n_bg] / bg_max_len   the background corpus, laid
                out as waves / wave_off, with ``clip_rms`` of it; ``clip_rms`` float64[n_clips] that of
                the main corpus.  A slot mixes with probability ``mix_prob``: one background clip, read
                circularly from a random start, at an SNR uniform in ``mix_snr_db`` = (lo, hi) dB.
    Returns (points, labels or None [, meta int32 [B, 8] = (clip, centre of frame 0 in the resampled
    clip, window length, bits of the gain, speed index, background clip or -1, its start, bits of the
    fp32 background scale)] [, samples float32 [B, Nt, n_fft]: the frames before window and gain]
    [, labels2 int64 [B], weight float32 [B]]).

    bg_labels   int64[n_bg], the classes of the background clips (needs ``clip_labels``): the call
                (pca_frame_points_ex_targets) also returns, after everything else, the soft target of each
                slot for ``cross_entropy`` / ``STEngine.fwd_bwd``: ``labels2`` = the background clip's class
                and ``weight`` = 1 / (1 + 10^(-snr/20)), the primary clip's share of the amplitude after
                RMS matching (between-class learning's rule with the RMS for its A-weighted level;
                ``mix_snr_db=(-20, 20)`` spans weights of about 0.09 .. 0.91), in a slot that mixes;
                ``labels2`` = the slot's own label and ``weight`` = 1 in every other slot.  Everything
                else is bit for bit what the call without ``bg_labels`` returns.
    (``_mask``: ``frame_points_masked``'s way in - its checked options and ``lengths_out``.)"""
    _need_cuda(waves, wave_off, set_off, idx, farr, clip_rms, bg_waves, bg_off, bg_rms, bg_labels)
    assert waves.dtype == torch.float32 and waves.is_contiguous() and farr.dtype == torch.float32
    assert wave_off.dtype == set_off.dtype == idx.dtype == torch.int64
    assert wave_off.numel() == set_off.numel() >= 2 and farr.numel() >= n_bins
    din = 2
    if tarr is not None:
        _need_cuda(tarr)
        assert tarr.dtype == torch.float32 and tarr.numel() >= Nt
        din = 3
    B = idx.numel()
    n_clips = wave_off.numel() - 1
    ratios = tuple(float(r) for r in ratios)
    if not 1 <= len(ratios) <= _lib.FRAME_MAX_SPEEDS:
        raise _lib.PcaHipError(f"frame_points_ex: {len(ratios)} ratios (1 .. {_lib.FRAME_MAX_SPEEDS})")
    n_bg = 0
    if bg_waves is not None:
        assert bg_waves.dtype == torch.float32 and bg_waves.is_contiguous()
        assert bg_off is not None and bg_off.dtype == torch.int64 and bg_off.is_contiguous()
        n_bg = bg_off.numel() - 1
        assert bg_rms is None or (bg_rms.dtype == torch.float64 and bg_rms.numel() == n_bg)
        assert clip_rms is None or (clip_rms.dtype == torch.float64 and clip_rms.numel() == n_clips)
    with torch.cuda.device(waves.device):
        tables, nwin, num_table = _speed_filter(ratios, waves.device)
        if win_lengths is None:
            win_lengths = torch.tensor([n_fft], dtype=torch.int32, device=waves.device)
        assert win_lengths.is_cuda and win_lengths.dtype == torch.int32
        if out is None:
            out = torch.empty((B, Nt * n_bins, din), dtype=torch.float32, device=waves.device)
        if clip_labels is not None and labels_out is None:
            labels_out = torch.empty(B, dtype=torch.int64, device=waves.device)
        meta = torch.empty((B, 8), dtype=torch.int32, device=waves.device) if want_meta else None
        samples = (torch.empty((B, Nt, n_fft), dtype=torch.float32, device=waves.device)
                   if want_samples else None)
        aug = _lib.PcaFrameAugEx(
            int(jitter), float(gain_db), win_lengths.data_ptr(), win_lengths.numel(), int(norm_mode),
            int(seed) & (2 ** 64 - 1), int(draw) & (2 ** 64 - 1), _draw_ptr(draw_dev),
            len(ratios), int(nwin), int(num_table), int(n_bg),
            (C.c_double * _lib.FRAME_MAX_SPEEDS)(*ratios), _ptr(tables),
            _ptr(bg_waves), _ptr(bg_off), _ptr(bg_rms), _ptr(clip_rms), int(bg_max_len),
            float(mix_prob), float(mix_snr_db[0]), float(mix_snr_db[1]))
        args = (_ptr(waves), _ptr(wave_off), _ptr(set_off), n_clips, int(max_len), int(min_len),
                _ptr(clip_labels), _ptr(idx), B, int(n_fft), int(hop), int(n_bins), int(Nt), _ptr(farr),
                _ptr(tarr), C.byref(aug), _ptr(out), _ptr(labels_out), _ptr(meta), _ptr(samples))
        lengths_out = mask_meta = None
        if _mask is not None:
            mask, lengths_out = _mask
            if mask.mode == _lib.MASK_DROP and lengths_out is None:
                lengths_out = torch.empty(B, dtype=torch.int32, device=waves.device)
            if lengths_out is not None:
                _need_cuda(lengths_out)
                assert lengths_out.dtype == torch.int32 and lengths_out.is_contiguous()
                assert lengths_out.numel() == B
            if want_meta:
                mask_meta = torch.empty((B, 4 * _lib.POINT_MASK_MAX), dtype=torch.int32,
                                        device=waves.device)
        if bg_labels is not None:
            assert bg_labels.dtype == torch.int64 and bg_labels.is_contiguous()
            assert bg_labels.numel() == n_bg, "one background label per background clip"
            if labels2_out is None:
                labels2_out = torch.empty(B, dtype=torch.int64, device=waves.device)
            if weight_out is None:
                weight_out = torch.empty(B, dtype=torch.float32, device=waves.device)
            assert labels2_out.dtype == torch.int64 and labels2_out.numel() == B
            assert weight_out.dtype == torch.float32 and weight_out.numel() == B
        if _mask is not None:
            check(lib().pca_frame_points_masked(*args, _ptr(bg_labels), _ptr(labels2_out),
                                                _ptr(weight_out), C.byref(mask), _ptr(lengths_out),
                                                _ptr(mask_meta), _stream(waves)),
                  "pca_frame_points_masked")
        elif bg_labels is not None:
            check(lib().pca_frame_points_ex_targets(*args, _ptr(bg_labels), _ptr(labels2_out),
                                                    _ptr(weight_out), _stream(waves)),
                  "pca_frame_points_ex_targets")
        else:
            check(lib().pca_frame_points_ex(*args, _stream(waves)), "pca_frame_points_ex")
    ret = (out, labels_out)
    if want_meta:
        ret += (meta if mask_meta is None else torch.cat([meta, mask_meta], dim=1),)
    if want_samples:
        ret += (samples,)
    if bg_labels is not None:
        ret += (labels2_out, weight_out)
    if _mask is not None and mask.mode == _lib.MASK_DROP:
        ret += (lengths_out,)
    return ret


MASK_MODES = {"drop": _lib.MASK_DROP, "floor": _lib.MASK_FLOOR}


def point_mask(n_bins: int, Nt: int, freq_masks: int = 0, freq_mask_width: int = 0, time_masks: int = 0,
               time_mask_width: int = 0, mask_mode="drop") -> "_lib.PcaPointMask":
    """The checked mask options of ``frame_points_masked`` as the C struct; ``ValueError`` for what
    pca_frame_points_masked would refuse (the same rules, on the host)."""
    nf, wf, nt, wt = int(freq_masks), int(freq_mask_width), int(time_masks), int(time_mask_width)
    if mask_mode not in MASK_MODES:
        raise ValueError(f"mask_mode is 'drop' or 'floor', got {mask_mode!r}")
    for name, n in (("freq_masks", nf), ("time_masks", nt)):
        if not 0 <= n <= _lib.POINT_MASK_MAX:
            raise ValueError(f"{name} {n} outside [0, {_lib.POINT_MASK_MAX}]")
    if wf < 0 or wt < 0:
        raise ValueError(f"mask widths must be >= 0, got freq_mask_width {wf}, time_mask_width {wt}")
    if nf > 0 and wf > 0 and nf * wf >= n_bins:
        raise ValueError(f"{nf} bands of up to {wf} bins could mask all {n_bins} bins: one must survive")
    if nt > 0 and wt > 0 and nt * wt >= Nt:
        raise ValueError(f"{nt} stripes of up to {wt} frames could mask all {Nt} frames: one must survive")
    return _lib.PcaPointMask(nf, wf, nt, wt, MASK_MODES[mask_mode])


def frame_points_masked(*args, freq_masks: int = 0, freq_mask_width: int = 0, time_masks: int = 0,
                        time_mask_width: int = 0, mask_mode="drop",
                        lengths_out: Optional[torch.Tensor] = None, **kw):
    """``frame_points_ex`` (every argument of it, with the same meaning) that also removes random
    frequency bands and time stripes of points from every set, in the same launch
    (pca_frame_points_masked): SpecAugment for point sets - a masked point is absent, not overwritten.

    freq_masks / freq_mask_width   per batch slot ``freq_masks`` (0 .. 4) bands, each 0 .. ``freq_mask_width``
                bins wide at a uniform position, removed from all Nt frames of the slot
    time_masks / time_mask_width   likewise stripes of whole frames (needs Nt > 1)
    mask_mode   "drop": the kept points of every set are compacted to its front in their order, the rows
                behind them are zeros, and the call returns, after everything else, ``lengths`` int32 [B]
                (``lengths_out`` when given): the point count of every set, for ``STEngine.fwd_bwd`` /
                ``ST.forward``.  "floor": rows stay in place, a masked point keeps its coordinates and
                carries the value of a silent bin, log(1e-8); no ``lengths``.
    A kind whose count or width is 0 is off and draws nothing; overlapping masks form their union;
    ``freq_masks * freq_mask_width < n_bins`` and ``time_masks * time_mask_width < Nt`` (``ValueError``),
    so a set never becomes empty.  The masks use draws of their own: everything else the call returns is
    bit for bit ``frame_points_ex``'s.  ``want_meta``: meta is int32 [B, 24], ``frame_points_ex``'s 8 columns,
    then (start, width) of the 4 bands and of the 4 stripes as drawn (unused ones 0)."""
    n_bins = kw["n_bins"] if "n_bins" in kw else args[6]
    Nt = kw["Nt"] if "Nt" in kw else (args[9] if len(args) > 9 else 1)
    mask = point_mask(int(n_bins), int(Nt), freq_masks, freq_mask_width, time_masks, time_mask_width,
                      mask_mode)
    if mask.mode == _lib.MASK_FLOOR and lengths_out is not None:
        raise ValueError("mask_mode 'floor' keeps every row: no lengths_out")
    return frame_points_ex(*args, _mask=(mask, lengths_out), **kw)


def select_points(X: torch.Tensor, key: torch.Tensor, K: int,
                  lengths: Optional[torch.Tensor] = None, out: Optional[torch.Tensor] = None,
                  sel: Optional[torch.Tensor] = None):
    """The K points of largest ``key`` of every packed set (pca_select_points): X [B, N, din] float32, din
    2 or 3, key [B, N] float32, 1 <= K <= N <= 16384.  Order: keys descending, equal keys in ascending
    point order, NaN last (subsample_points' MAXK rule); with ``lengths`` (device int32[B]) the points at
    and beyond lengths[b] come after every valid one.  Returns (out [B, K, din], sel int32 [B, K]); both
    may be passed in (contiguous)."""
    _need_cuda(X, key, lengths, out, sel)
    assert X.dim() == 3 and X.dtype == torch.float32 and X.is_contiguous()
    B, N, din = X.shape
    assert key.dtype == torch.float32 and key.is_contiguous() and tuple(key.shape) == (B, N)
    if lengths is not None:
        assert lengths.dtype == torch.int32 and lengths.is_contiguous() and tuple(lengths.shape) == (B,)
    K = int(K)
    with torch.cuda.device(X.device):
        if out is None:
            out = torch.empty((B, K, din), dtype=torch.float32, device=X.device)
        if sel is None:
            sel = torch.empty((B, K), dtype=torch.int32, device=X.device)
        assert out.dtype == torch.float32 and out.is_contiguous() and tuple(out.shape) == (B, K, din)
        assert sel.dtype == torch.int32 and sel.is_contiguous() and tuple(sel.shape) == (B, K)
        check(lib().pca_select_points(_ptr(X), _ptr(key), _ptr(lengths), B, N, din, K, _ptr(out),
                                      _ptr(sel), _stream(X)), "pca_select_points")
    return out, sel


def peak_spec(radius_f: int = 1, radius_t: int = 0, rel_floor: float = float("inf"),
              abs_floor: float = float("-inf"), refine: bool = True) -> "_lib.PcaPeakSpec":
    """``PcaPeakSpec`` checked on the host by the rules of pca_peak_points (``ValueError``)."""
    radius_f, radius_t, rel_floor, abs_floor = int(radius_f), int(radius_t), float(rel_floor), float(abs_floor)
    if not 1 <= radius_f <= 16:
        raise ValueError(f"radius_f {radius_f} outside [1, 16] bins")
    if not 0 <= radius_t <= 4:
        raise ValueError(f"radius_t {radius_t} outside [0, 4] frames")
    if not rel_floor >= 0.0:
        raise ValueError(f"rel_floor {rel_floor}: >= 0 (inf switches it off)")
    if abs_floor != abs_floor:
        raise ValueError("abs_floor is NaN (-inf switches it off)")
    return _lib.PcaPeakSpec(radius_f, radius_t, rel_floor, abs_floor, int(bool(refine)))


def peak_points(X: torch.Tensor, F: int, Nt: int, K: int, radius_f: int = 1, radius_t: int = 0,
                rel_floor: float = float("inf"), abs_floor: float = float("-inf"), refine: bool = True,
                lengths: Optional[torch.Tensor] = None, out: Optional[torch.Tensor] = None,
                lengths_out: Optional[torch.Tensor] = None, want_sel: bool = False,
                want_count: bool = False):
    """The K strongest spectral peaks of every packed set (pca_peak_points): X [B, F * Nt, din] float32 as
    the pack and frame launches write it (point p = t * F + f, value in the last column, frequency in
    column 0; din 2 needs Nt = 1), F >= 3, 1 <= K <= N <= 16384.

    A peak is a point with 1 <= f <= F - 2 whose (value, -p) is greater than that of every other point within
    ``radius_f`` bins and ``radius_t`` frames (a tie goes to the lower index; NaN never wins) and whose value
    is at least ``abs_floor`` and at least the set's maximum minus ``rel_floor``.  Peaks are ranked by raw
    value, descending, equal values in ascending point order (subsample_points' MAXK rule).  ``refine``:
    frequency and value come from the parabola through the values at f - 1, f, f + 1 (fp64, rounded once);
    off: the bin's own row.  ``lengths`` (device int32[B], whole frames): the points at and beyond
    lengths[b] take no part.

    Returns (out [B, K, din] - rows behind a set's last peak are zeros -, lengths int32 [B] =
    clamp(number of peaks, 1, K): a set without peaks yields its largest point) [, sel int32 [B, K], the
    point indices, -1 behind the last][, count int32 [B], the peaks before truncation]; ``out`` and
    ``lengths_out`` may be passed in (contiguous)."""
    _need_cuda(X, lengths, out, lengths_out)
    assert X.dim() == 3 and X.dtype == torch.float32 and X.is_contiguous()
    B, N, din = X.shape
    F, Nt, K = int(F), int(Nt), int(K)
    assert N == F * Nt, (N, F, Nt)
    if lengths is not None:
        assert lengths.dtype == torch.int32 and lengths.is_contiguous() and tuple(lengths.shape) == (B,)
    spec = peak_spec(radius_f, radius_t, rel_floor, abs_floor, refine)
    with torch.cuda.device(X.device):
        if out is None:
            out = torch.empty((B, K, din), dtype=torch.float32, device=X.device)
        if lengths_out is None:
            lengths_out = torch.empty(B, dtype=torch.int32, device=X.device)
        assert out.dtype == torch.float32 and out.is_contiguous() and tuple(out.shape) == (B, K, din)
        assert lengths_out.dtype == torch.int32 and lengths_out.is_contiguous() \
            and tuple(lengths_out.shape) == (B,)
        sel = torch.empty((B, K), dtype=torch.int32, device=X.device) if want_sel else None
        count = torch.empty(B, dtype=torch.int32, device=X.device) if want_count else None
        check(lib().pca_peak_points(_ptr(X), _ptr(lengths), B, F, Nt, din, C.byref(spec), K, _ptr(out),
                                    _ptr(lengths_out), _ptr(count), _ptr(sel), _stream(X)),
              "pca_peak_points")
    res = (out, lengths_out)
    if want_sel:
        res += (sel,)
    if want_count:
        res += (count,)
    return res


def pack_points_2d_ss(x_tk: torch.Tensor, f_tk: torch.Tensor, idx: torch.Tensor,
                      labels: Optional[torch.Tensor] = None,
                      out: Optional[torch.Tensor] = None,
                      labels_out: Optional[torch.Tensor] = None
                      ) -> Tuple[torch.Tensor, Optional[torch.Tensor]]:
    """Batch of ESC_pc_ss items from frame-major tables x_tk, f_tk [T, K] (contiguous):
    ([B, K, 2] float32, labels[idx])."""
    _need_cuda(x_tk, f_tk, idx)
    assert x_tk.dtype == torch.float32 and f_tk.dtype == torch.float32
    assert x_tk.is_contiguous() and f_tk.is_contiguous() and x_tk.shape == f_tk.shape
    K = x_tk.shape[1]
    B = idx.numel()
    with torch.cuda.device(x_tk.device):
        if out is None:
            out = torch.empty((B, K, 2), dtype=torch.float32, device=x_tk.device)
        if labels is not None and labels_out is None:
            labels_out = torch.empty(B, dtype=torch.int64, device=x_tk.device)
        check(lib().pca_pack_points_2d_ss(_ptr(x_tk), _ptr(f_tk), _ptr(idx), B, K, _ptr(out),
                                          _ptr(labels), _ptr(labels_out), _stream(x_tk)),
              "pca_pack_points_2d_ss")
    return out, labels_out


def importance_kernel(winF: int) -> torch.Tensor:
    """The [2, winF] smoothing kernel of Code/dataset.py:283: outer product of two periodic
    Kaiser windows (beta 5.09), built with the same torch calls so that the weights are
    bit-identical to the reference's."""
    return (torch.kaiser_window(window_length=2, periodic=True, beta=5.09)[:, None]
            @ torch.kaiser_window(window_length=int(winF), periodic=True, beta=5.09)[None, :]
            ).contiguous()


def importance_points(spec: torch.Tensor, farr: torch.Tensor, tarr: torch.Tensor,
                      idx: torch.Tensor, K: int, choice: int, kern: torch.Tensor,
                      seed: int = 0, draw: int = 0, labels: Optional[torch.Tensor] = None,
                      out: Optional[torch.Tensor] = None,
                      labels_out: Optional[torch.Tensor] = None, want_sel: bool = False,
                      want_heat: bool = False, draw_dev: Optional[torch.Tensor] = None):
    """Batch of ESC_pc_temp_importancerandKSS items (pca_importance_points): spec [F, Nt, S]
    through its strides, kern [2, winF] float32 on the device.  Returns
    (points [B, K, 3], labels[idx] or None[, sel int32 [B, K]][, heat [B, F, Nt]])."""
    _need_cuda(spec, farr, tarr, idx, kern)
    assert spec.dtype == torch.float32 and idx.dtype == torch.int64
    assert kern.dtype == torch.float32 and kern.is_contiguous() and kern.shape[0] == 2
    F, Nt, _ = spec.shape
    B = idx.numel()
    with torch.cuda.device(spec.device):
        if out is None:
            out = torch.empty((B, K, 3), dtype=torch.float32, device=spec.device)
        if labels is not None and labels_out is None:
            labels_out = torch.empty(B, dtype=torch.int64, device=spec.device)
        sel = torch.empty((B, K), dtype=torch.int32, device=spec.device) if want_sel else None
        heat = torch.empty((B, F, Nt), dtype=torch.float32, device=spec.device) \
            if want_heat else None
        check(lib().pca_importance_points(
            _ptr(spec), spec.stride(0), spec.stride(1), spec.stride(2), _ptr(farr), _ptr(tarr),
            _ptr(idx), B, F, Nt, int(K), int(choice), _ptr(kern), int(kern.shape[1]),
            int(seed) & (2 ** 64 - 1), int(draw) & (2 ** 64 - 1), _draw_ptr(draw_dev), _ptr(out),
            _ptr(sel), _ptr(heat), _ptr(labels), _ptr(labels_out), _stream(spec)), "pca_importance_points")
    res = [out, labels_out]
    if want_sel:
        res.append(sel)
    if want_heat:
        res.append(heat)
    return tuple(res)


def pack_points_2d_seq(spec: torch.Tensor, farr: torch.Tensor, idx_seq: torch.Tensor,
                       step_dev: torch.Tensor, base_dev: torch.Tensor, B: int,
                       labels: Optional[torch.Tensor] = None, frame_major: bool = False,
                       out: Optional[torch.Tensor] = None,
                       labels_out: Optional[torch.Tensor] = None):
    """pack_points_2d for batch number ``step_dev[0] - base_dev[0]`` of the pre-staged index
    sequence ``idx_seq`` ([n_steps * B] int64 on the device): the cursor lives on the device, so
    a captured step replays without any per-step index upload (pca_pack_points_2d_seq)."""
    _need_cuda(spec, farr, idx_seq, step_dev, base_dev)
    assert spec.dtype == torch.float32 and idx_seq.dtype == torch.int64
    assert step_dev.dtype == torch.int32 and base_dev.dtype == torch.int32
    if frame_major:
        T_, F = spec.shape
        sf, st = spec.stride(1), spec.stride(0)
    else:
        F, T_ = spec.shape
        sf, st = spec.stride(0), spec.stride(1)
    with torch.cuda.device(spec.device):
        if out is None:
            out = torch.empty((B, F, 2), dtype=torch.float32, device=spec.device)
        if labels is not None and labels_out is None:
            labels_out = torch.empty(B, dtype=torch.int64, device=spec.device)
        check(lib().pca_pack_points_2d_seq(_ptr(spec), sf, st, _ptr(farr), _ptr(idx_seq),
                                           _ptr(step_dev), _ptr(base_dev), B, F, _ptr(out),
                                           _ptr(labels), _ptr(labels_out), _stream(spec)),
              "pca_pack_points_2d_seq")
    return out, labels_out


def pack_points_3d_seq(spec: torch.Tensor, farr: torch.Tensor, tarr: torch.Tensor,
                       idx_seq: torch.Tensor, step_dev: torch.Tensor, base_dev: torch.Tensor,
                       B: int, labels: Optional[torch.Tensor] = None,
                       out: Optional[torch.Tensor] = None,
                       labels_out: Optional[torch.Tensor] = None,
                       nt_valid: Optional[torch.Tensor] = None,
                       lengths_out: Optional[torch.Tensor] = None):
    """3-D counterpart of pack_points_2d_seq (pca_pack_points_3d_seq); with ``nt_valid`` the
    batch is padded and the lengths are returned as a third value."""
    _need_cuda(spec, farr, tarr, idx_seq, step_dev, base_dev)
    assert spec.dtype == torch.float32 and idx_seq.dtype == torch.int64
    F, Nt, S = spec.shape
    with torch.cuda.device(spec.device):
        if out is None:
            out = torch.empty((B, F * Nt, 3), dtype=torch.float32, device=spec.device)
        if labels is not None and labels_out is None:
            labels_out = torch.empty(B, dtype=torch.int64, device=spec.device)
        if nt_valid is not None and lengths_out is None:
            lengths_out = torch.empty(B, dtype=torch.int32, device=spec.device)
        check(lib().pca_pack_points_3d_seq(
            _ptr(spec), spec.stride(0), spec.stride(1), spec.stride(2), _ptr(farr), _ptr(tarr),
            _ptr(nt_valid), _ptr(idx_seq), _ptr(step_dev), _ptr(base_dev), B, F, Nt, _ptr(out),
            _ptr(lengths_out if nt_valid is not None else None), _ptr(labels), _ptr(labels_out),
            _stream(spec)), "pca_pack_points_3d_seq")
    if nt_valid is not None:
        return out, labels_out, lengths_out
    return out, labels_out
