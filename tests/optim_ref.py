"""One guarded optimiser step (pca_grad_sumsq + pca_adam_step_ex) restated in torch on the CPU.

``OptimRef.step``: the global norm from a float64 sum of squares, rounded to fp32 like the kernel's; the
fp32 clip factor of torch.nn.utils.clip_grad_norm_; the learning rate looked up in the host's table; the
skip of a step whose norm is not finite; and oracle.st_oracle.AdamState for the update itself, whose own
step count is the number of APPLIED steps, which is what the bias correction must use.

``TorchTruth``: the same step by stock parts, torch.nn.utils.clip_grad_norm_ and torch.optim.Adam (a
skipped step never calls ``step()``): the outer truth the restatement is itself held to
(tests/test_optim_host.py)."""
import math

import numpy as np
import torch

from oracle import st_oracle as orc


def f32(x):
    return float(np.float32(x))


def global_norm(grads, grad_scale=1.0):
    """grad_scale * sqrt(sum of squares), the sum in float64, the result rounded to fp32."""
    s = sum(float(g.double().pow(2).sum()) for g in grads.values())
    with np.errstate(over="ignore", invalid="ignore"):
        return f32(np.float64(grad_scale) * np.sqrt(np.float64(s)))


def clip_factor(norm, max_norm):
    """min(1, max_norm / (norm + 1e-6)) in fp32; 1 without max_norm."""
    if max_norm is None or not max_norm > 0:
        return 1.0
    with np.errstate(over="ignore", invalid="ignore"):
        c = np.float32(max_norm) / (np.float32(norm) + np.float32(1e-6))
    return float(c) if not c >= 1 else 1.0


def table_lr(table, t):
    """The table's entry for step t (1-based; the last entry holds from there on), as fp32."""
    return f32(table[min(t, len(table)) - 1])


class OptimRef:
    def __init__(self, params, lr=1e-3, wd=1e-3, b1=0.9, b2=0.999, eps=1e-8, max_norm=None,
                 skip_nonfinite=False, table=None, grad_scale=1.0):
        self.adam = orc.AdamState(params, lr=lr, wd=wd, b1=b1, b2=b2, eps=eps)
        self.lr, self.max_norm, self.skip_nonfinite = lr, max_norm, skip_nonfinite
        self.table, self.grad_scale = table, grad_scale
        self.t = self.skipped = self.clipped = 0
        self.last_norm = self.last_lr = 0.0

    @property
    def m(self):
        return self.adam.m

    @property
    def v(self):
        return self.adam.v

    def step(self, params, grads):
        """params: {name: fp32 tensor}, updated in place; grads: the same names."""
        self.t += 1
        self.last_lr = table_lr(self.table, self.t) if self.table is not None else f32(self.lr)
        self.last_norm = global_norm(grads, self.grad_scale)
        clip = clip_factor(self.last_norm, self.max_norm)
        if self.skip_nonfinite and not math.isfinite(self.last_norm):
            self.skipped += 1
            return
        self.clipped += clip < 1.0
        scale = f32(np.float32(self.grad_scale) * np.float32(clip))
        self.adam.lr = self.last_lr
        self.adam.step(params, {k: g * scale for k, g in grads.items()})


class TorchTruth:
    """torch.optim.Adam (coupled weight decay) behind torch.nn.utils.clip_grad_norm_ on leaf copies of
    ``params``; the learning rate is set per step from the same table."""

    def __init__(self, params, lr=1e-3, wd=1e-3, betas=(0.9, 0.999), eps=1e-8, max_norm=None,
                 skip_nonfinite=False, table=None):
        self.p = {k: v.detach().clone().requires_grad_(True) for k, v in params.items()}
        self.opt = torch.optim.Adam(list(self.p.values()), lr=lr, betas=betas, eps=eps, weight_decay=wd)
        self.lr, self.max_norm, self.skip_nonfinite, self.table = lr, max_norm, skip_nonfinite, table
        self.t = 0
        self.norms = []

    def step(self, grads):
        self.t += 1
        for k, w in self.p.items():
            w.grad = grads[k].detach().clone()
        leaves = list(self.p.values())
        if self.max_norm is not None:
            norm = float(torch.nn.utils.clip_grad_norm_(leaves, self.max_norm))
        else:
            norm = float(torch.linalg.vector_norm(torch.stack([w.grad.norm() for w in leaves])))
        self.norms.append(norm)
        if self.skip_nonfinite and not math.isfinite(norm):
            return
        for grp in self.opt.param_groups:
            grp["lr"] = table_lr(self.table, self.t) if self.table is not None else self.lr
        self.opt.step()

    def moments(self, name):
        st = self.opt.state[self.p[name]]
        return st["exp_avg"], st["exp_avg_sq"]
