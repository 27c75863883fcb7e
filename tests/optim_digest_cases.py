"""The cases of tests/test_gpu_optim_digest.py and scripts/optim_digest_golden.py, and their runner: three
launches of one optimiser entry point on seeded vectors, then the SHA-256 of everything the launches wrote.

The grid is ceil(n / 2048) workgroups, at most 1024, so the sizes are the smallest that reach every code site:
0 (the step still advances), 3 (tail only), 7 (one quadruple and a tail), 2053 (two workgroups, a thread's
second quadruple), 292 530 (cfg2's parameter count, n % 4 == 2) and 2 200 003 (the grid-stride loop and a
tail).  Each runs 16-byte aligned and with every vector one float behind a 16-byte boundary, with zero_grad 0
and 1, through every VARIANT below.

Gradients: the first launch's has norm 4 (clip factor 0.25 under max_norm = 1), the third's norm 0.25 (factor
exactly 1); the guarded variants get an inf into the second launch's, which is then skipped.  grad_scale is
not 1 in the update (GSCALE) so that the product g * grad_scale rounds: with a scale of 1 both fusions of
`g * s + wd * w` give the same bits and a moved fusion would go unseen."""
import ctypes as C
import functools
import hashlib

import numpy as np
import torch

SIZES = (0, 3, 7, 2053, 292530, 2200003)
OFFSETS = (0, 1)
ZERO_GRAD = (0, 1)
LR, WD, GSCALE, MAX_NORM = 1e-2, 0.1, 0.37, 1.0
TABLE = (2e-2, 5e-3)                  # two entries: the third launch reads past the end, i.e. the last
AVG_DECAY = 0.9

# name -> (entry point, options).  guards: max_norm + skip_nonfinite + TABLE, and the inf in launch 2
VARIANTS = {
    "plain": ("plain", {}),
    "ex": ("ex", {}),
    "ex_guards": ("ex", dict(guards=True)),
    "groups": ("groups", {}),
    "groups_avg": ("groups", dict(avg_start=2)),
    "groups_table": ("groups", dict(table=True)),
    "groups_decoupled": ("groups", dict(decoupled=True)),      # the pass without a table, at every n
    "groups_all": ("groups", dict(decoupled=True, table=True, avg_start=1, guards=True)),
}
GUARDED = tuple(k for k, (_, o) in VARIANTS.items() if o.get("guards"))


def key(n, offset, zero_grad, variant):
    return f"n{n}-off{offset}-zg{zero_grad}-{variant}"


def segments(n):
    """(seg_end, lr_scale, wd_scale): the first boundary inside a float4 quadruple, the second on one, one
    frozen segment (lr_scale 0).  Fewer segments where n has no room; none at n == 0."""
    ends = sorted({e for e in ((n // 3 & ~3) + 2, 2 * n // 3 & ~3, n) if 0 < e <= n})
    return ends, [1.5, 0.0, 0.5][:len(ends)], [0.0, 1.0, 2.0][:len(ends)]


@functools.lru_cache(maxsize=2)
def inputs_of(n):
    """p and the three gradients (fp32 numpy), plus the second gradient with an inf in the middle."""
    rng = np.random.Generator(np.random.PCG64(4100 + n))
    p = (rng.standard_normal(n) * 0.5).astype(np.float32)
    gs = []
    for norm in (4.0, 1.0, 0.25):
        g = rng.standard_normal(n)
        if n:
            g *= norm / (GSCALE * np.sqrt((g * g).sum()))      # the norm the kernel forms includes GSCALE
        gs.append(g.astype(np.float32))
    g_inf = gs[1].copy()
    if n:
        g_inf[n // 2] = np.inf
    return p, gs, g_inf


def run_case(dev, n, offset, zero_grad, variant):
    """-> (sha256 hex of p, g, m, v[, avg], step words, state words after three launches, state words)."""
    from pca_hip import _lib
    L = _lib.lib()
    entry, opt = VARIANTS[variant]
    guards = bool(opt.get("guards"))
    p0, gs, g_inf = inputs_of(n)
    grads = [gs[0], g_inf if guards else gs[1], gs[2]]

    def vec(src=None, fill=0.0):
        base = torch.full((n + 4 + offset,), fill, dtype=torch.float32, device=dev)
        assert base.data_ptr() % 16 == 0
        view = base[offset:offset + n]
        if src is not None:
            view.copy_(torch.from_numpy(src))
        return view

    at = lambda view: view._base.data_ptr() + 4 * view.storage_offset()     # also for an empty vector
    ptr = lambda t: None if t is None else t.data_ptr()
    p, g, m, v = vec(p0), vec(), vec(), vec()
    avg = vec(fill=-7.0) if "avg_start" in opt else None
    step = torch.zeros(2, dtype=torch.int32, device=dev)
    state = torch.zeros(8, dtype=torch.int32, device=dev)
    part = torch.zeros(int(L.pca_grad_sumsq_partials(n)), dtype=torch.float64, device=dev)
    table = torch.tensor(TABLE, dtype=torch.float32, device=dev) if guards else None
    cfg = _lib.OptimCfg(LR, 0.9, 0.999, 1e-8, WD, GSCALE, MAX_NORM if guards else 0.0, int(guards))
    ends, ls, ws = segments(n) if opt.get("table") else ([], [], [])
    ends_host = (C.c_int64 * max(len(ends), 1))(*ends)
    ends_dev = torch.tensor(ends, dtype=torch.int64, device=dev) if ends else None
    ls_dev = torch.tensor(ls, dtype=torch.float32, device=dev) if ends else None
    ws_dev = torch.tensor(ws, dtype=torch.float32, device=dev) if ends else None
    gr = _lib.OptimGroups(int(bool(opt.get("decoupled"))), len(ends), ptr(ends_dev), ptr(ls_dev), ptr(ws_dev),
                          None if avg is None else at(avg), 1.0 - AVG_DECAY, opt.get("avg_start", 1))
    st = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    for grad in grads:
        g.copy_(torch.from_numpy(grad))
        if entry == "plain":
            _lib.check(L.pca_adam_step(at(p), at(g), at(m), at(v), n, LR, 0.9, 0.999, 1e-8, WD, GSCALE,
                                       step.data_ptr(), zero_grad, st), "pca_adam_step")
            continue
        npart = part.numel() if guards else 0
        if guards:
            _lib.check(L.pca_grad_sumsq(at(g), n, part.data_ptr(), npart, st), "pca_grad_sumsq")
        args = (at(p), at(g), at(m), at(v), n, C.byref(cfg), part.data_ptr() if guards else None, npart,
                ptr(table), len(TABLE) if guards else 0, step.data_ptr(), state.data_ptr(), zero_grad)
        if entry == "ex":
            _lib.check(L.pca_adam_step_ex(*args, st), "pca_adam_step_ex")
        else:
            _lib.check(L.pca_adam_step_groups(*args, C.byref(gr), ends_host, st), "pca_adam_step_groups")
    torch.cuda.synchronize()
    h = hashlib.sha256()
    for t in (p, g, m, v, avg, step, state):
        if t is not None:
            h.update(t.cpu().numpy().tobytes())
    return h.hexdigest(), state.cpu().tolist()
