"""Eval-mode forward of the paper's two fixed-input baselines on MI355X: FB (``models.baseline_ff``,
Code/models.py:47-88) and CNN_temp (``models.CNN_classifier``, Code/models.py:91-119), through
pca_fb_forward / pca_cnn_temp_forward (csrc/baselines.hip).

The sets are read in place from a resident spectrogram (FB frames: [F, T]; CNN_temp chunks:
[F, Nt, S], addressed as pca_pack_points_3d) and may be sub-sampled inside the launch: all but K cells
zeroed, the kept ones chosen exactly as ``subsample_points`` chooses them (max-K / random-K), which is
the zero-filled input of Code/utils.py:86-108 (FB) / Code/dataset.py:101-135 (CNN_temp).  Training the
baselines stays stock PyTorch.
"""
from __future__ import annotations

import ctypes as C
from typing import List, Optional, Tuple

import torch

from . import _lib
from ._lib import check, lib
from .ops import MAXK, RANDK, _draw_ptr, _need_cuda, _ptr, _stream  # noqa: F401

SEL_ALL = 2        # PCA_SEL_ALL: no selection, the whole set

__all__ = ["BaselineEngine", "baseline_config", "SEL_ALL"]


def _linears(seq) -> List[torch.nn.Linear]:
    return [m for m in seq.children() if isinstance(m, torch.nn.Linear)]


def baseline_config(model) -> Tuple[bool, int, int, List[int], int]:
    """(is_cnn, Nt, Nf, layer_dims, nclasses) of a ``baseline_ff`` / ``CNN_classifier`` (bare or
    under nn.DataParallel), read off its sub-modules, so the reference's own classes work too."""
    model = getattr(model, "module", model)
    if hasattr(model, "ENC_NN"):
        lins = _linears(model.ENC_NN)
        cnn, Nt, Nf = False, 1, 0
    elif hasattr(model, "cnn") and hasattr(model, "linear"):
        w = model.cnn.weight
        if tuple(w.shape[:2]) != (1, 1) or model.cnn.bias is None or \
                tuple(model.cnn.stride) != (1, 1) or tuple(model.cnn.padding) != (0, 0):
            raise _lib.PcaHipError(f"CNN_temp: unexpected conv {model.cnn}")
        lins = _linears(model.linear)
        cnn, Nt = True, int(w.shape[2])
        Nf = int(w.shape[3]) - 1 + lins[0].in_features
    else:
        raise _lib.PcaHipError(f"{type(model).__name__} is neither baseline_ff nor CNN_classifier")
    dims = [int(lin.in_features) for lin in lins]
    for a, b in zip(lins[:-1], lins[1:]):
        assert a.out_features == b.in_features, "MLP widths do not chain"
    return cnn, Nt, Nf, dims, int(lins[-1].out_features)


class BaselineEngine:
    """Forward of a ``baseline_ff`` (FB) or ``CNN_classifier`` (CNN_temp) on the device.

    The parameters are copied ONCE into a flat fp32 vector in state_dict order (the model itself is
    left alone: build a new engine after changing its weights).  ``forward`` returns FB
    probabilities (the model ends in nn.Softmax) or CNN_temp logits, [B, nclasses]."""

    def __init__(self, model, device=None):
        self.cnn, self.Nt, self.Nf, self.layer_dims, self.nclasses = baseline_config(model)
        m = getattr(model, "module", model)
        sd = m.state_dict()
        dev = torch.device(device) if device is not None else next(m.parameters()).device
        _need_cuda(torch.empty(0, device=dev))
        self.dev = dev
        self.flat = torch.cat([v.detach().reshape(-1).float() for v in sd.values()]).to(dev)
        self._dims = (C.c_int * len(self.layer_dims))(*self.layer_dims)
        n = lib().pca_baseline_param_count(int(self.cnn), self.Nt, self.Nf, self._dims,
                                           len(self.layer_dims), self.nclasses)
        if n != self.flat.numel():
            msg = lib().pca_last_error()
            raise _lib.PcaHipError(f"parameter count mismatch: kernel {n}, model "
                                   f"{self.flat.numel()} {msg.decode() if msg else ''}")
        self.F = self.Nf if self.cnn else self.layer_dims[0]

    @property
    def num_cells(self) -> int:
        """Cells of one input set: F (FB) or F * Nt (CNN_temp)."""
        return self.F * self.Nt

    def forward(self, spec: torch.Tensor, idx: torch.Tensor, K: Optional[int] = None,
                mode: int = SEL_ALL, seed: int = 0, draw: int = 0,
                draw_dev: Optional[torch.Tensor] = None, labels: Optional[torch.Tensor] = None,
                out: Optional[torch.Tensor] = None, labels_out: Optional[torch.Tensor] = None,
                want_sel: bool = False):
        """Sets ``idx`` (int64 [B], device) of ``spec`` - FB: [F, T] float32 (frame t =
        spec[:, t]); CNN_temp: [F, Nt, S] (chunk s = spec[:, :, s]), any strides.  ``mode``
        SEL_ALL: the whole set; MAXK / RANDK: all but K cells zeroed, chosen as
        ``subsample_points(spec, .., idx, K, mode, seed, draw, draw_dev=draw_dev)`` chooses them.
        Returns (out [B, nclasses], labels[idx] or None[, sel int32 [B, K]]); enqueues only."""
        _need_cuda(spec, idx)
        assert spec.dtype == torch.float32 and idx.dtype == torch.int64 and idx.is_contiguous()
        B = idx.numel()
        if mode == SEL_ALL:
            K = 0
            assert not want_sel, "no selection to return"
        else:
            assert K is not None, "max-K / random-K need K"
        L = lib()
        with torch.cuda.device(spec.device):
            if out is None:
                out = torch.empty((B, self.nclasses), dtype=torch.float32, device=spec.device)
            assert out.shape == (B, self.nclasses) and out.is_contiguous()
            if labels is not None and labels_out is None:
                labels_out = torch.empty(B, dtype=torch.int64, device=spec.device)
            sel = torch.empty((B, int(K)), dtype=torch.int32, device=spec.device) \
                if want_sel else None
            common = (self._dims, len(self.layer_dims), self.nclasses, _ptr(self.flat),
                      self.flat.numel(), int(K), int(mode), int(seed) & (2 ** 64 - 1),
                      int(draw) & (2 ** 64 - 1), _draw_ptr(draw_dev), _ptr(out), _ptr(sel),
                      _ptr(labels), _ptr(labels_out), _stream(spec))
            if self.cnn:
                assert spec.dim() == 3, "CNN_temp: spec is [F, Nt, S]"
                F, Nt, _ = spec.shape
                assert Nt == self.Nt, f"chunks of {Nt} frames, the model takes {self.Nt}"
                check(L.pca_cnn_temp_forward(_ptr(spec), spec.stride(0), spec.stride(1),
                                             spec.stride(2), _ptr(idx), B, F, Nt, self.Nf, *common),
                      "pca_cnn_temp_forward")
            else:
                assert spec.dim() == 2, "FB: spec is [F, T]"
                check(L.pca_fb_forward(_ptr(spec), spec.stride(0), spec.stride(1), _ptr(idx), B,
                                       spec.shape[0], *common), "pca_fb_forward")
        return (out, labels_out, sel) if want_sel else (out, labels_out)
