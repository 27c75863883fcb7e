"""Cases and the runner shared by tests/test_gpu_set128_prefetch.py and scripts/set128_prefetch_golden.py (which
records the hashes of a given build of the library in tests/golden/set128_prefetch_sha256.json).

Whole eager train steps, d = 128, h = 4, m = 16, bf16 mode, on the set-resident path, at the smallest shapes that
reach every request that moved ahead of a hand-off of k_set128_fwd (csrc/set128_fwd.hip: the fragments of layer 2's
mid-stage A and B in front of hand-off 2's flag wait, the partner's payload in two batches, the head stages'
weights in front of hand-off 3's) and the fp32 weight-gradient rows of k_wgrad128_step that request their whole
range at once (csrc/wgrad128.hip):

* one and two units per quad (N = 256, 512), B = 1 and B with an odd pair count;
* ``lengths`` with a set at len <= N / 2 (half 1 publishes the empty partial at both hand-offs) and one at len = 1;
* the head stages as a launch of their own (PCA_SET128_HEAD=0: k_pma_head1) and the PMA's attention backward as
  one (PCA_SET128_PMABWD=0), where half 1 leaves behind hand-off 3 and only half 0 takes the prefetched weights;
* C = 50 and C = 3 (the classifier rows beyond C are loaded from row 0: the clamped class index);
* B = 1 (16 fp32 rows: the guarded prologue of the weight-gradient rows) and B = 9 (144 rows at 128 per workgroup:
  one workgroup with its whole range of two full steps in flight, one with a ragged single step)."""
import mab1_bwd_loads_cases as lc
import set128_addr_cases as sc

D, H, M = lc.D, lc.H, 16

# key -> (B, N, din, lengths or None, C, extra environment).  The B = 1 case comes first.
CASES = {
    "dense-B1-N256-din2": (1, 256, 2, None, 50, {}),
    "dense-B5-N256-din3": (5, 256, 3, None, 50, {}),
    "dense-B3-N512-din2": (3, 512, 2, None, 50, {}),
    "dense-B9-N256-din2": (9, 256, 2, None, 50, {}),
    "lengths-B1-N256-din2": (1, 256, 2, [97], 50, {}),
    "lengths-B5-N256-din3": (5, 256, 3, [256, 1, 128, 129, 33], 50, {}),
    "lengths-B3-N512-din2": (3, 512, 2, [512, 256, 1], 50, {}),
    "head0-B5-N256-din3": (5, 256, 3, None, 50, {"PCA_SET128_HEAD": "0"}),
    "head0-lengths-B3-N512-din2": (3, 512, 2, [512, 256, 1], 50, {"PCA_SET128_HEAD": "0"}),
    "pmabwd0-B3-N512-din2": (3, 512, 2, None, 50, {"PCA_SET128_PMABWD": "0"}),
    "pmabwd0-lengths-B5-N256-din3": (5, 256, 3, [256, 1, 128, 129, 33], 50, {"PCA_SET128_PMABWD": "0"}),
    "C3-B5-N256-din3": (5, 256, 3, None, 3, {}),
    "C3-lengths-B3-N512-din2": (3, 512, 2, [512, 256, 1], 3, {}),
}
N_OUT = sc.N_OUT      # logits, loss, 45 gradients
# Gradients that the parent's own passes do not repeat would be left out here by name, as
# set128_addr_cases.UNPINNED leaves out layer 1's fc_q at din = 4 (summed by atomics).  No case has din = 4, and
# scripts/set128_prefetch_golden.py refuses a build whose three passes differ in anything not listed.
UNPINNED = {}


def engine_net(dev, key):
    import models
    import torch
    B, N, din, _, C, _ = CASES[key]
    torch.manual_seed(6100 + N + din + C)
    return models.ST(dim_input=din, num_outputs=1, dim_output=C, num_inds=M, dim_hidden=D, num_heads=H).to(dev)


def engine_inputs(key):
    import inputs as gi
    B, N, din, lengths, C, _ = CASES[key]
    X = gi.pc_input(9700 + N + B, B, N, din)
    if lengths is not None:
        for b, L in enumerate(lengths):        # padding rows: zeros, as the pack kernel writes
            X[b, L:] = 0.0
    return X, gi.labels(9701 + N + B, B, C)


def run(net, key, X, y, witness=False):
    """One eager train step -> ({"logits", "loss", one entry per gradient}, kernel names of one more step or None).
    The hand-off counter is checked to be zero behind the step."""
    import torch
    from pca_hip import _lib, trainer
    B, N, din, lengths, C, extra = CASES[key]
    ld = None if lengths is None else torch.tensor(lengths, dtype=torch.int32, device=X.device)
    with lc.env(PCA_SET128="1", **extra):
        eng = trainer.STEngine(net, B, N, _lib.MODE_BF16, training=True)
        eng.fwd_bwd(X, y, phase=-1, lengths=ld)
        torch.cuda.synchronize()
        eng.check_handoffs()
        assert eng._handoff_word is not None and int(eng._handoff_word.item()) == 0
        out = {"logits": eng.logits.clone(), "loss": eng.loss.clone()}
        g = eng.grads.clone()
        off = 0
        for k, prm in net.named_parameters():
            out[k] = g[off:off + prm.numel()].view_as(prm)
            off += prm.numel()
        assert off == g.numel() and len(out) == N_OUT, (off, g.numel(), len(out))
        names = lc.kernel_names(lambda: eng.fwd_bwd(X, y, phase=-1, lengths=ld)) if witness else None
        if witness:
            eng.check_handoffs()
    return out, names
