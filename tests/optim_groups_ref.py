"""One pca_adam_step_groups step (csrc/optim.hip) restated in torch on the CPU, and the same step by
stock parts.

``GroupsRef.step``: tests/optim_ref.py's norm, clip factor and table lookup in front of the per-segment
Adam / AdamW update written out in fp32 torch, and the averaged copy behind it (a copy up to applied step
``avg_start``, ``avg += (1 - decay) * (w - avg)`` after it; a skipped step touches nothing and is not counted).

``StockTruth``: torch.optim.AdamW / torch.optim.Adam with one param_group per segment carrying
``lr * lr_scale`` and ``weight_decay * wd_scale``, torch.nn.utils.clip_grad_norm_ over all of them, and
torch.optim.swa_utils.AveragedModel(multi_avg_fn=get_ema_multi_avg_fn(decay)) updated from applied step
``avg_start`` on and never on a skipped step: the outer truth the restatement is itself held to
(tests/test_optim_groups_host.py).

``CASES``: the option sets both the host and the GPU tests run, on a flat vector of n = 10007."""
import math

import numpy as np
import torch
from torch.optim.swa_utils import AveragedModel, get_ema_multi_avg_fn

from optim_ref import clip_factor, f32, global_norm, table_lr

LR, WD = 1e-2, 0.1                       # large enough for every switch to show (see the GPU tests)
SEG_END = (4099, 4101, 7000, 10007)      # both inner boundaries inside a float4; one segment of two
LR_SCALE = (1.0, 0.0, 1.0, 0.5)
WD_SCALE = (1.0, 1.0, 0.0, 2.0)

GROUPS = dict(seg_end=SEG_END, lr_scale=LR_SCALE, wd_scale=WD_SCALE)
CASES = {
    "decoupled_grouped_averaged_clipped": dict(GROUPS, decoupled=True, max_norm=50.0, avg_decay=0.9,
                                               avg_start=2),
    "coupled_grouped": dict(GROUPS, decoupled=False, max_norm=50.0, avg_decay=0.9, avg_start=2),
    "decoupled_ungrouped": dict(decoupled=True, max_norm=50.0, avg_decay=0.9, avg_start=2),
    "unit_scales": dict(seg_end=SEG_END, lr_scale=(1.0,) * 4, wd_scale=(1.0,) * 4, decoupled=False),
    "skip": dict(GROUPS, decoupled=True, max_norm=50.0, skip_nonfinite=True, avg_decay=0.9, avg_start=1),
}


def segments(n, seg_end):
    """[(lo, hi)] of the table; without one the whole vector is one segment."""
    ends = [n] if not seg_end else list(seg_end)
    assert ends[-1] == n and all(b > a for a, b in zip([0] + ends[:-1], ends)), (n, ends)
    return list(zip([0] + ends[:-1], ends))


class GroupsRef:
    def __init__(self, p, seg_end=None, lr_scale=None, wd_scale=None, decoupled=False, lr=LR, wd=WD,
                 b1=0.9, b2=0.999, eps=1e-8, max_norm=None, skip_nonfinite=False, table=None,
                 grad_scale=1.0, avg_decay=None, avg_start=1):
        self.p = p.detach().clone().float()
        self.m, self.v = torch.zeros_like(self.p), torch.zeros_like(self.p)
        self.segs = segments(self.p.numel(), seg_end)
        self.lr_scale = [1.0] * len(self.segs) if lr_scale is None else list(lr_scale)
        self.wd_scale = [1.0] * len(self.segs) if wd_scale is None else list(wd_scale)
        self.decoupled, self.lr, self.wd, self.b1, self.b2, self.eps = decoupled, lr, wd, b1, b2, eps
        self.max_norm, self.skip_nonfinite, self.table = max_norm, skip_nonfinite, table
        self.grad_scale = grad_scale
        self.avg = None if avg_decay is None else torch.zeros_like(self.p)
        self.avg_weight = None if avg_decay is None else f32(1.0 - avg_decay)
        self.avg_start = avg_start
        self.t = self.skipped = self.clipped = 0
        self.last_norm = self.last_lr = 0.0

    def step(self, grad):
        self.t += 1
        self.last_lr = table_lr(self.table, self.t) if self.table is not None else f32(self.lr)
        self.last_norm = global_norm({"w": grad}, self.grad_scale)
        clip = clip_factor(self.last_norm, self.max_norm)
        if self.skip_nonfinite and not math.isfinite(self.last_norm):
            self.skipped += 1
            return
        self.clipped += clip < 1.0
        scale = f32(np.float32(self.grad_scale) * np.float32(clip))
        a = self.t - self.skipped                              # applied steps, this one included
        bc1, bc2 = 1 - self.b1 ** a, 1 - self.b2 ** a
        for (lo, hi), ls, ws in zip(self.segs, self.lr_scale, self.wd_scale):
            lr_e = f32(np.float32(self.last_lr) * np.float32(ls))
            wd_e = f32(np.float32(self.wd) * np.float32(ws))
            w, m, v = self.p[lo:hi], self.m[lo:hi], self.v[lo:hi]
            w_in = w.clone()
            g = grad[lo:hi].float() * scale
            if self.decoupled:
                w.mul_(f32(1.0 - np.float32(lr_e) * np.float32(wd_e)))
            else:
                g = g + wd_e * w
            m.mul_(self.b1).add_(g, alpha=1 - self.b1)
            v.mul_(self.b2).addcmul_(g, g, value=1 - self.b2)
            denom = (v.sqrt() / math.sqrt(bc2)).add_(self.eps)
            w.addcdiv_(m, denom, value=-lr_e / bc1)
            if ls == 0:
                w.copy_(w_in)                                  # a frozen segment keeps its bits
        if self.avg is not None:
            if a <= self.avg_start:
                self.avg.copy_(self.p)
            else:
                self.avg.add_(self.p - self.avg, alpha=self.avg_weight)


class _Leaves(torch.nn.Module):
    def __init__(self, pieces):
        super().__init__()
        self.w = torch.nn.ParameterList([torch.nn.Parameter(x.detach().clone()) for x in pieces])


class StockTruth:
    def __init__(self, p, seg_end=None, lr_scale=None, wd_scale=None, decoupled=False, lr=LR, wd=WD,
                 betas=(0.9, 0.999), eps=1e-8, max_norm=None, skip_nonfinite=False, table=None,
                 avg_decay=None, avg_start=1):
        self.segs = segments(p.numel(), seg_end)
        self.lr_scale = [1.0] * len(self.segs) if lr_scale is None else list(lr_scale)
        wd_scale = [1.0] * len(self.segs) if wd_scale is None else list(wd_scale)
        self.net = _Leaves([p[lo:hi].float() for lo, hi in self.segs])
        groups = [dict(params=[w], lr=lr * ls, weight_decay=wd * ws)
                  for w, ls, ws in zip(self.net.w, self.lr_scale, wd_scale)]
        cls = torch.optim.AdamW if decoupled else torch.optim.Adam
        self.opt = cls(groups, lr=lr, betas=betas, eps=eps, weight_decay=wd)
        self.ema = None if avg_decay is None else \
            AveragedModel(self.net, multi_avg_fn=get_ema_multi_avg_fn(avg_decay))
        self.lr, self.max_norm, self.skip_nonfinite, self.table = lr, max_norm, skip_nonfinite, table
        self.avg_start = avg_start
        self.t = self.applied = self.averaged = 0
        self.norms = []

    def step(self, grad):
        self.t += 1
        leaves = list(self.net.w)
        for w, (lo, hi) in zip(leaves, self.segs):
            w.grad = grad[lo:hi].detach().clone().float()
        if self.max_norm is not None:
            norm = float(torch.nn.utils.clip_grad_norm_(leaves, self.max_norm))
        else:
            norm = float(torch.linalg.vector_norm(torch.stack([w.grad.norm() for w in leaves])))
        self.norms.append(norm)
        if self.skip_nonfinite and not math.isfinite(norm):
            return
        lr = table_lr(self.table, self.t) if self.table is not None else self.lr
        for grp, ls in zip(self.opt.param_groups, self.lr_scale):
            grp["lr"] = lr * ls
        self.opt.step()
        self.applied += 1
        if self.ema is not None and self.applied >= self.avg_start:
            self.ema.update_parameters(self.net)
            self.averaged += 1

    def _cat(self, ts):
        return torch.cat([t.detach().reshape(-1) for t in ts])

    @property
    def p(self):
        return self._cat(self.net.w)

    @property
    def m(self):
        return self._cat([self.opt.state[w]["exp_avg"] for w in self.net.w])

    @property
    def v(self):
        return self._cat([self.opt.state[w]["exp_avg_sq"] for w in self.net.w])

    @property
    def avg(self):
        return self._cat(self.ema.module.w)


def adam_inputs():
    """p and five gradients, n = 10007: test_gpu_optim.py's _adam_inputs() draws."""
    g = torch.Generator().manual_seed(9)
    torch.randn(37, 50, generator=g)
    torch.randint(0, 50, (37,), generator=g)
    n = 10007
    p = torch.randn(n, generator=g)
    return n, p, [torch.randn(n, generator=g) for _ in range(5)]


def case_grads(name, grads):
    """The five gradients as the case uses them: step 3 scaled to 0.2 (so that one step does not clip), or
    for "skip" with a NaN at element 4321 instead, as test_gpu_optim.py's clip and skip tests have them."""
    grads = [x.clone() for x in grads]
    if name == "skip":
        grads[2][4321] = float("nan")
    else:
        grads[2] = grads[2] * 0.2
    return grads
