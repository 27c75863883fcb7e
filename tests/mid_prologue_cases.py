"""Cases, runner and hashes shared by tests/test_gpu_mid_prologue.py and scripts/mid_prologue_golden.py (which
records the hashes of a given build of the library in tests/golden/mid_prologue_sha256.json)."""
import hashlib
import os

D, H, M, C = 128, 4, 16, 50
# B x N x din of the mid-prologue work.  The many-queries backward keeps one 128-point tile per workgroup below
# 256 workgroups, so with B <= 13 a set leaves 2, 3 or 4 partials in both layers: one group of the sum, full or not.
CASES = [(B, N, din) for B in (1, 5, 13) for N in (256, 384, 512) for din in (2, 3)]
# The other paths of the sum: a single partial (a batch that makes that kernel take a whole set per workgroup),
# several groups (16 partials) and a last group that is not full (6).
EXTRA = [(256, 256, 2), (4, 2048, 2), (3, 768, 3)]
# (layer 2, layer 1) partials per set, as the library reports them
_TILES = {256: 2, 384: 3, 512: 4}
NPARTS = {**{(B, N, din): (_TILES[N], _TILES[N]) for B, N, din in CASES},
          (256, 256, 2): (1, 2), (4, 2048, 2): (16, 16), (3, 768, 3): (6, 6)}
SWITCHES = ("PCA_SET128", "PCA_D128_MIDFUSE")


def paths(N):
    """The per-block path everywhere; the set-resident forward where it applies."""
    return (False, True) if N in (256, 512) else (False,)


def key(B, N, din, set128):
    return f"B{B}-N{N}-din{din}-{'set128' if set128 else 'launches'}"


def net_of(dev, din, seed):
    import models
    import torch
    torch.manual_seed(seed)
    return models.ST(dim_input=din, num_outputs=1, dim_output=C, num_inds=M, dim_hidden=D, num_heads=H).to(dev)


def inputs_of(B, N, din):
    import inputs as gi
    return gi.pc_input(8600 + N + B, B, N, din), gi.labels(8601 + N + B, B, C)


def run(net, X, y, B, N, fuse, set128):
    """One eager train step with the switches set: logits, loss, flat gradients."""
    import torch
    from pca_hip import _lib, trainer
    old = {k: os.environ.get(k) for k in SWITCHES}
    os.environ["PCA_SET128"] = "1" if set128 else "0"
    os.environ["PCA_D128_MIDFUSE"] = "1" if fuse else "0"
    try:
        eng = trainer.STEngine(net, B, N, _lib.MODE_BF16, training=True)
        eng.fwd_bwd(X, y, phase=-1)
        torch.cuda.synchronize()
        eng.check_handoffs()
        return eng.logits.clone(), eng.loss.clone(), eng.grads.clone()
    finally:
        for k, v in old.items():
            if v is None:
                del os.environ[k]
            else:
                os.environ[k] = v


def _sha(t):
    return hashlib.sha256(t.detach().cpu().contiguous().numpy().tobytes()).hexdigest()


def hashes(net, out):
    """SHA-256 of the bytes of the logits, the loss and each of the 45 gradients."""
    lg, loss, g = out
    res = {"logits": _sha(lg), "loss": _sha(loss), "grads": {}}
    off = 0
    for k, prm in net.named_parameters():
        res["grads"][k] = _sha(g[off:off + prm.numel()])
        off += prm.numel()
    assert len(res["grads"]) == 45 and off == g.numel(), (len(res["grads"]), off, g.numel())
    return res
