"""Cases, runners and hashes shared by tests/test_gpu_prep_rebuild.py and scripts/prep_rebuild_golden.py (which
records the hashes of a given build of the library in tests/golden/prep_rebuild_sha256.json).

Whole calls of the engine and the Trainer whose first launch is the preparation plan (csrc/prep_plan.hpp):
k_prep_all in the engine's training steps, k_mab0_prep / k_prep_jobs in the per-block and forward-only paths."""
import contextlib
import hashlib
import os

C = 50

# key -> (kind, B, N, din, d, h, m, lengths, environment)
#   kind "step": one eager train step of the engine; "forward": one forward-only call; "trainer": three steps of the
#   cursor-mode Trainer replayed from a graph, the pack deferred into the preparation launch (pca_pack_defer)
CASES = {
    "set128-B5-N256-din2": ("step", 5, 256, 2, 128, 4, 16, None, {"PCA_SET128": "1"}),
    "launches-B3-N96-din3": ("step", 3, 96, 3, 128, 4, 16, None, {"PCA_SET128": "0"}),
    "launches-lengths-B3-N96-din3": ("step", 3, 96, 3, 128, 4, 16, (96, 50, 1), {"PCA_SET128": "0"}),
    "trainer-cursor-B4-N256-din2": ("trainer", 4, 256, 2, 128, 4, 16, None, {"PCA_PACK_DEFER": "1"}),
    "forward-B5-N256-din2": ("forward", 5, 256, 2, 128, 4, 16, None, {}),
    "d256-B2-N64-din2": ("step", 2, 64, 2, 256, 8, 32, None, {}),
}
# The outputs a case pins: everything it produces, but for d = 256 / m = 32 - logits and loss only: there the weight
# gradients are summed by fp32 atomics in the order the workgroups arrive, and no build repeats them from pass to pass.
LOGITS_AND_LOSS_ONLY = ("d256-B2-N64-din2",)
# Further outputs that the library sums by fp32 atomics (none of the cases above has one: fc_q's gradient at dq = 4
# would be; see tests/mab1_bwd_loads_cases.py).  key -> names.  A case always keeps logits and loss.
UNPINNED = {}
STEPS = 3


@contextlib.contextmanager
def env(**kv):
    old = {k: os.environ.get(k) for k in kv}
    os.environ.update(kv)
    try:
        yield
    finally:
        for k, v in old.items():
            if v is None:
                del os.environ[k]
            else:
                os.environ[k] = v


def net_of(dev, key):
    import models
    import torch
    _, B, N, din, d, h, m, _, _ = CASES[key]
    torch.manual_seed(2100 + N + din + m)
    return models.ST(dim_input=din, num_outputs=1, dim_output=C, num_inds=m, dim_hidden=d, num_heads=h).to(dev)


def inputs_of(key):
    import inputs as gi
    _, B, N, din, _, _, _, lengths, _ = CASES[key]
    X = gi.pc_input(9100 + N + B, B, N, din)
    if lengths is not None:
        for b, L in enumerate(lengths):            # padding rows: zeros, as the pack kernel writes
            X[b, L:] = 0.0
    return X, gi.labels(9101 + N + B, B, C)


def dataset_of(dev, key):
    """A 2-D point-set dataset of STEPS batches: column t of the spectrogram is one set."""
    import dataset
    import inputs as gi
    import numpy as np
    _, B, N, din, _, _, _, _, _ = CASES[key]
    x = np.concatenate([gi.pc_input(9200 + s, B, N, din)[:, :, 1].T for s in range(STEPS)], axis=1)
    y = np.concatenate([gi.labels(9300 + s, B, C) for s in range(STEPS)])
    return dataset.ESC_pc(x, y, np.linspace(0.0, 0.5, N), device=dev)


def _grads(net, g, out):
    off = 0
    for k, prm in net.named_parameters():
        out[k] = g[off:off + prm.numel()].view_as(prm).clone()
        off += prm.numel()
    assert off == g.numel(), (off, g.numel())


def run(dev, key):
    """-> {"logits", "loss" (but for the forward-only call), one entry per gradient (where the case pins them)}."""
    import torch
    from pca_hip import _lib, trainer
    kind, B, N, din, d, h, m, lengths, extra = CASES[key]
    net = net_of(dev, key)
    out = {}
    with env(**extra):
        if kind == "trainer":
            tr = trainer.Trainer(net, dataset_of(dev, key), B, mode=_lib.MODE_BF16, use_graph=True, seed=1,
                                 shuffle=False, keep_grads=True)
            assert tr._cursor_mode
            for _ in range(STEPS):
                tr.step()
            torch.cuda.synchronize()
            eng = tr.eng
            out["X"], out["labels"], out["params"] = tr.X.clone(), tr.labels.clone(), eng.flat.clone()
        else:
            Xn, yn = inputs_of(key)
            X, y = torch.from_numpy(Xn).to(dev), torch.from_numpy(yn).to(dev)
            ld = None if lengths is None else torch.tensor(lengths, dtype=torch.int32, device=dev)
            eng = trainer.STEngine(net, B, N, _lib.MODE_BF16, training=kind == "step")
            if kind == "forward":
                eng.forward(X, lengths=ld)
            else:
                eng.fwd_bwd(X, y, phase=-1, lengths=ld)
            torch.cuda.synchronize()
            eng.check_handoffs()
        out["logits"] = eng.logits.clone()
        if kind != "forward":
            out["loss"] = eng.loss.clone()
            if key not in LOGITS_AND_LOSS_ONLY:
                _grads(net, eng.grads, out)
                assert len(out) >= 47, len(out)                          # logits, loss, the 45 gradients
    return {k: v for k, v in out.items() if k not in UNPINNED.get(key, ())}


def _sha(t):
    return hashlib.sha256(t.detach().cpu().contiguous().numpy().tobytes()).hexdigest()


def hashes(out):
    return {k: _sha(v) for k, v in out.items()}
