"""Cases and the runner shared by tests/test_gpu_set128_handoff2.py and scripts/set128_handoff2_golden.py (which
records the hashes of a given build of the library in tests/golden/set128_handoff2_sha256.json).

Whole eager train steps, d = 128, h = 4, m = 16, bf16 mode, on the set-resident path, at the smallest shapes that
reach every path of layer 2's quad merge and pair hand-off 2 of k_set128_fwd (csrc/set128_fwd.hip) once round B, the
publish, the fetch of the partner's partial and the cross-half merge run on all sixteen waves - wave (quad q, head j)
owns the feature tiles 2 q and 2 q + 1 of head j:

* one and two units per quad (N = 256, 512), din = 2 and 3, B = 1;
* B = 9: an odd count of pairs, one XCD's slot used twice; B = 16: both pair slots of every XCD;
* ``lengths`` that put the partial's edge everywhere a quad or a half can be empty - N = 256: 256, 129 (half 1 holds
  one point), 128 (half 1 empty), 65 (quad 1 of half 0 holds one point), 64 (quads 1 - 3 empty), 1; N = 512: 512, 257,
  256, 129, 1;
* the head stages as a launch of their own (PCA_SET128_HEAD=0) and the PMA's attention backward as one
  (PCA_SET128_PMABWD=0), once each; C = 3 once."""
import contextlib

import mab1_bwd_loads_cases as lc
import set128_addr_cases as sc
import set128_prefetch_cases as pc

D, H, M = lc.D, lc.H, 16

L256 = [256, 129, 128, 65, 64, 1]
L512 = [512, 257, 256, 129, 1]
# key -> (B, N, din, lengths or None, C, extra environment).  The B = 1 cases come first.
CASES = {
    "dense-B1-N256-din2": (1, 256, 2, None, 50, {}),
    "dense-B1-N256-din3": (1, 256, 3, None, 50, {}),
    "dense-B1-N512-din2": (1, 512, 2, None, 50, {}),
    "dense-B1-N512-din3": (1, 512, 3, None, 50, {}),
    "dense-B9-N256-din2": (9, 256, 2, None, 50, {}),
    "dense-B16-N512-din3": (16, 512, 3, None, 50, {}),
    "lengths-B6-N256-din2": (6, 256, 2, L256, 50, {}),
    "lengths-B5-N512-din3": (5, 512, 3, L512, 50, {}),
    "head0-lengths-B6-N256-din3": (6, 256, 3, L256, 50, {"PCA_SET128_HEAD": "0"}),
    "pmabwd0-lengths-B5-N512-din2": (5, 512, 2, L512, 50, {"PCA_SET128_PMABWD": "0"}),
    "C3-B9-N512-din2": (9, 512, 2, None, 3, {}),
}
N_OUT = sc.N_OUT      # logits, loss, 45 gradients
# Gradients that the parent's own passes do not repeat would be left out here by name (see
# set128_prefetch_cases.UNPINNED).  No case has din = 4, and scripts/set128_handoff2_golden.py refuses a build
# whose three passes differ in anything not listed.
UNPINNED = {}


def engine_net(dev, key):
    import models
    import torch
    B, N, din, _, C, _ = CASES[key]
    torch.manual_seed(6200 + N + din + C)
    return models.ST(dim_input=din, num_outputs=1, dim_output=C, num_inds=M, dim_hidden=D, num_heads=H).to(dev)


def engine_inputs(key):
    import inputs as gi
    B, N, din, lengths, C, _ = CASES[key]
    X = gi.pc_input(9800 + N + B, B, N, din)
    if lengths is not None:
        for b, L in enumerate(lengths):        # padding rows: zeros, as the pack kernel writes
            X[b, L:] = 0.0
    return X, gi.labels(9801 + N + B, B, C)


@contextlib.contextmanager
def _cases_of(module, cases):
    keep = module.CASES
    module.CASES = cases
    try:
        yield
    finally:
        module.CASES = keep


def run(net, key, X, y, witness=False):
    """set128_prefetch_cases.run() on a case of THIS module: one eager train step -> ({"logits", "loss", one entry
    per gradient}, kernel names of one more step or None); the hand-off counter is checked to be zero behind it."""
    with _cases_of(pc, CASES):
        return pc.run(net, key, X, y, witness=witness)
