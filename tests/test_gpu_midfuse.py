"""The ISAB's per-set backward mid chain (csrc/mid_bwd_body.hpp) run in the prologue of the few-queries
backward (k_mab0_bwd<64, .> in layer 2, k_mab0_bwd_small in layer 1; every workgroup of a set for itself,
the images kept in LDS) against

* the two k_mid_bwd launches it replaces (``PCA_D128_MIDFUSE=0``): the same MFMAs on the same operands in
  the same summation order, so logits, loss and all 45 gradients are the same bits;
* itself: two passes are bitwise equal;
* the CPU oracle (``oracle/st_oracle.py:st_grads``) at the tolerance tests/test_gpu_set128_pmabwd.py uses
  for the same comparison.

Launch witness: the kernels of one eager step as the profiler of torch sees them.  With the switch on the
library launches exactly two kernels fewer, and no k_mid_bwd."""
import os

import pytest
import torch

import grad_bars as gb
from util import T, close, close_robust

import inputs as gi

pytestmark = pytest.mark.gpu

SWITCHES = ("PCA_SET128", "PCA_D128_MIDFUSE")


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


def _kernels(fn):
    """Names of the device kernels one call of fn() launches."""
    from torch.profiler import ProfilerActivity, profile
    torch.cuda.synchronize()
    with profile(activities=[ProfilerActivity.CPU, ProfilerActivity.CUDA]) as prof:
        fn()
        torch.cuda.synchronize()
    cuda = getattr(torch.autograd.DeviceType, "CUDA", None)
    names = [e.name for e in prof.events() if e.device_type == cuda]
    # library kernels only (namespace pca, mangled or not; torch's own fills and copies are not)
    return [n for n in names if "pca" in n]


def _run(net, X, y, B, N, fuse, set128, witness=False):
    """One eager train step with the switches set; witness: also the kernel names of one more step."""
    from pca_hip import _lib, trainer
    old = {k: os.environ.get(k) for k in SWITCHES}
    os.environ["PCA_SET128"] = "1" if set128 else "0"
    os.environ["PCA_D128_MIDFUSE"] = "1" if fuse else "0"
    try:
        eng = trainer.STEngine(net, B, N, _lib.MODE_BF16, training=True)
        eng.fwd_bwd(X, y, phase=-1)
        torch.cuda.synchronize()
        eng.check_handoffs()
        out = eng.logits.clone(), eng.loss.clone(), eng.grads.clone()
        if witness:
            names = _kernels(lambda: eng.fwd_bwd(X, y, phase=-1))
            eng.check_handoffs()
            return (*out, names)
        return out
    finally:
        for k, v in old.items():
            if v is None:
                del os.environ[k]
            else:
                os.environ[k] = v


def _same_bits(net, a, b, what):
    lg1, loss1, g1 = a[:3]
    lg0, loss0, g0 = b[:3]
    assert torch.isfinite(g1).all()
    assert torch.equal(lg1, lg0), f"{what}: logits moved"
    assert torch.equal(loss1, loss0), (what, float(loss1), float(loss0))
    off = 0
    n = 0
    for k, prm in net.named_parameters():
        u = g1[off:off + prm.numel()]
        v = g0[off:off + prm.numel()]
        off += prm.numel()
        n += 1
        assert torch.equal(u, v), f"{what}: {k}: max |diff| {float((u - v).abs().max()):.3e}"
    assert n == 45 and off == g1.numel(), (n, off, g1.numel())


CASES = [(B, N, din) for N in (256, 512) for din in (2, 3) for B in (5, 13, 128)] + [(4, 2048, 2)]


@pytest.mark.parametrize("set128", [True, False], ids=["set128", "launches"])
@pytest.mark.parametrize("B,N,din", CASES)
def test_midfuse_equals_launches(dev, B, N, din, set128):
    C = 50
    net = _net(dev, din, C, 900 + N + din)
    X = T(gi.pc_input(8200 + N + B, B, N, din), dev)
    y = T(gi.labels(8201 + N + B, B, C), dev)
    r0 = _run(net, X, y, B, N, fuse=False, set128=set128, witness=True)
    r1 = _run(net, X, y, B, N, fuse=True, set128=set128, witness=True)
    r2 = _run(net, X, y, B, N, fuse=True, set128=set128)
    k0, k1 = r0[3], r1[3]
    print(f"B={B} N={N} din={din} set128={set128}: library launches {len(k0)} -> {len(k1)}")
    assert sum("k_mid_bwd" in n for n in k0) == 2, k0
    assert sum("k_mid_bwd" in n for n in k1) == 0, k1
    assert len(k1) == len(k0) - 2, (len(k0), len(k1), k0, k1)
    _same_bits(net, r1, r0, "fused vs launches")
    _same_bits(net, r2, r1, "fused, second pass")


@pytest.mark.parametrize("set128", [True, False], ids=["set128", "launches"])
@pytest.mark.parametrize("B,N,din", CASES)
def test_midfuse_vs_oracle(dev, B, N, din, set128):
    from oracle import st_oracle as orc
    C = 50
    net = _net(dev, din, C, 950 + N + din)
    p = {k: v.detach().cpu().clone() for k, v in net.state_dict().items()}
    Xn = gi.pc_input(8300 + N + B, B, N, din)
    yn = gi.labels(8301 + N + B, B, C)
    ref_loss, ref_lg, ref_g = orc.st_grads(torch.from_numpy(Xn), torch.from_numpy(yn), p, 4)
    lg, loss, g = _run(net, T(Xn, dev), T(yn, dev), B, N, fuse=True, set128=set128)
    close(lg, ref_lg.reshape(B, C), 3e-2, "logits")
    assert abs(float(loss) - ref_loss) < 3e-2 * max(1.0, abs(ref_loss))
    off = 0
    for k, prm in net.named_parameters():
        close_robust(g[off:off + prm.numel()].view_as(prm), ref_g[k], 5e-2, k, outlier_frac=5e-3)
        off += prm.numel()
    gb.judge(g, ref_g, gb.BF16_VS_ORACLE, gb.shapes_of(net), f"B={B} N={N} din={din} midfuse vs oracle")
