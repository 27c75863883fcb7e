"""The PMA's attention backward in the tail of the set-resident d = 128 forward (csrc/set128_fwd.hip,
pma_bwd_tail: both workgroups of a pair run the head stages on the same merge, then each computes dY2 of
its resident rows of Y2 and its dG slab) against

* the launch it replaces (``PCA_SET128_PMABWD=0``: k_mab0_bwd<32, true> over Y2 from memory): the tail
  runs the same MFMAs on the same operands and sums dG in the same order, so logits, loss and all 45
  gradients are the same bits;
* the CPU oracle (``oracle/st_oracle.py:st_grads``) at the bf16 mode's tolerance;
* itself: two passes are bitwise equal (no atomics: the dG slabs are summed in a fixed order).

The launch witness (tests/dispatch.py) checks that the switch removes one k_mab0_bwd launch per eager
step, and that ``PCA_SET128_HEAD=0`` (head stages as a launch of their own) keeps it."""
import os

import pytest
import torch

from dispatch import launches
import grad_bars as gb
from util import T, close, close_robust

import inputs as gi

pytestmark = pytest.mark.gpu

SWITCHES = ("PCA_SET128", "PCA_SET128_HEAD", "PCA_SET128_PMABWD")


@pytest.fixture(scope="module")
def dev():
    import pca_hip
    pca_hip.lib()
    return torch.device("cuda", 0)


def _net(dev, din, C, seed):
    import models
    torch.manual_seed(seed)
    return models.ST(dim_input=din, num_outputs=1, dim_output=C, num_inds=16, dim_hidden=128,
                     num_heads=4).to(dev)


def _run(net, X, y, B, N, pmabwd, head=True, witness=False):
    """One eager train step with the switches set; witness: also the k_mab0_bwd launches of one more
    step."""
    from pca_hip import _lib, trainer
    old = {k: os.environ.get(k) for k in SWITCHES}
    os.environ["PCA_SET128"] = "1"
    os.environ["PCA_SET128_HEAD"] = "1" if head else "0"
    os.environ["PCA_SET128_PMABWD"] = "1" if pmabwd else "0"
    try:
        eng = trainer.STEngine(net, B, N, _lib.MODE_BF16, training=True)
        eng.fwd_bwd(X, y, phase=-1)
        torch.cuda.synchronize()
        eng.check_handoffs()
        out = eng.logits.clone(), eng.loss.clone(), eng.grads.clone()
        if witness:
            n = launches(lambda: eng.fwd_bwd(X, y, phase=-1), ("mab0_bwd", "set_fwd"))
            eng.check_handoffs()
            return (*out, n)
        return out
    finally:
        for k, v in old.items():
            if v is None:
                del os.environ[k]
            else:
                os.environ[k] = v


@pytest.mark.parametrize("B,N,din", [(5, 256, 2), (13, 256, 3), (7, 512, 3), (21, 512, 2), (128, 512, 2)])
def test_pma_bwd_in_tail_equals_launch(dev, B, N, din):
    C = 50
    net = _net(dev, din, C, 300 + N + din)
    X = T(gi.pc_input(7200 + N + B, B, N, din), dev)
    y = T(gi.labels(7201 + N + B, B, C), dev)
    lg0, loss0, g0, n0 = _run(net, X, y, B, N, pmabwd=False, witness=True)
    lg1, loss1, g1, n1 = _run(net, X, y, B, N, pmabwd=True, witness=True)
    assert n0["set_fwd"] == 1 and n1["set_fwd"] == 1, (n0, n1)
    assert n1["mab0_bwd"] == n0["mab0_bwd"] - 1, f"k_mab0_bwd launches per step: {n0} -> {n1}"
    assert torch.isfinite(g1).all()
    assert torch.equal(lg1, lg0), "logits moved"
    assert torch.equal(loss1, loss0), (float(loss1), float(loss0))
    off = 0
    for k, prm in net.named_parameters():
        a = g1[off:off + prm.numel()]
        bref = g0[off:off + prm.numel()]
        off += prm.numel()
        assert torch.equal(a, bref), f"{k}: max |diff| {float((a - bref).abs().max()):.3e}"


def test_pma_bwd_in_tail_is_bit_reproducible(dev):
    B, N, din, C = 19, 512, 2, 50
    net = _net(dev, din, C, 41)
    X = T(gi.pc_input(7300, B, N, din), dev)
    y = T(gi.labels(7301, B, C), dev)
    a = _run(net, X, y, B, N, pmabwd=True)
    b = _run(net, X, y, B, N, pmabwd=True)
    for u, v, what in zip(a, b, ("logits", "loss", "grads")):
        assert torch.equal(u, v), what


def test_head_launch_keeps_k_mab0_bwd(dev):
    """PCA_SET128_HEAD=0: dT / LSE / Delta come from the k_pma_head1 launch, so the PMA backward stays a
    launch of its own whatever PCA_SET128_PMABWD says."""
    B, N, din, C = 6, 512, 2, 50
    net = _net(dev, din, C, 43)
    X = T(gi.pc_input(7400, B, N, din), dev)
    y = T(gi.labels(7401, B, C), dev)
    lg0, loss0, g0, n0 = _run(net, X, y, B, N, pmabwd=False, head=False, witness=True)
    lg1, loss1, g1, n1 = _run(net, X, y, B, N, pmabwd=True, head=False, witness=True)
    assert n1["mab0_bwd"] == n0["mab0_bwd"] >= 1, (n0, n1)
    for u, v, what in zip((lg0, loss0, g0), (lg1, loss1, g1), ("logits", "loss", "grads")):
        assert torch.equal(u, v), what


@pytest.mark.parametrize("B,N,din", [(6, 256, 2), (11, 512, 3)])
def test_pma_bwd_in_tail_vs_oracle(dev, B, N, din):
    from oracle import st_oracle as orc
    C = 50
    net = _net(dev, din, C, 500 + N)
    p = {k: v.detach().cpu().clone() for k, v in net.state_dict().items()}
    Xn = gi.pc_input(7500 + N, B, N, din)
    yn = gi.labels(7501 + N, B, C)
    ref_loss, ref_lg, ref_g = orc.st_grads(torch.from_numpy(Xn), torch.from_numpy(yn), p, 4)
    lg, loss, g = _run(net, T(Xn, dev), T(yn, dev), B, N, pmabwd=True)
    close(lg, ref_lg.reshape(B, C), 3e-2, "logits")
    assert abs(float(loss) - ref_loss) < 3e-2 * max(1.0, abs(ref_loss))
    off = 0
    for k, prm in net.named_parameters():
        close_robust(g[off:off + prm.numel()].view_as(prm), ref_g[k], 5e-2, k, outlier_frac=5e-3)
        off += prm.numel()
    gb.judge(g, ref_g, gb.BF16_VS_ORACLE, gb.shapes_of(net), f"B={B} N={N} din={din} tail vs oracle")
