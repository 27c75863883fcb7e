"""The deferred d = 128 weight gradients as ONE launch with several tiles of loads in flight
(csrc/wgrad128.hip: k_wgrad128_step; csrc/bwd_defer.hip: bwd_defer_flush) against

* the two k_wgrad128 launches it replaces (``PCA_WGRAD_FOLD=0``): the same row partition, the same tiles
  per row group in the same order, the same slabs summed in the same order, so logits, loss and all 45
  gradients are the same bits;
* itself: two passes are bitwise equal;
* the CPU oracle (``oracle/st_oracle.py:st_grads``; on the truncated sets where the batch has lengths) at
  the tolerances tests/test_gpu_midfuse.py and tests/test_gpu_varlen.py use for the same comparison.

Launch witness: the kernels of one eager step as the profiler of torch sees them.  With the switch on the
step shows one k_wgrad128 launch, with it off two, and the library launches one kernel fewer in all.

The shapes are the smallest at which the load pipeline (three 32-row tiles per row group in flight, a
guarded fetch only for the last steps of a range) and the fold can go wrong: a second workgroup whose range
is shorter than the pipeline is deep, a ragged last tile, jobs of less than one tile, a short last workgroup.

The non-deferred launch keeps its template kernels: one direct backward of the many-queries block with fp32
activations (the <bf16, float> instance, 390 rows: a ragged tile) against the oracle's bf16 emulation, the
workspaces followed by guard regions as in tests/test_gpu_bf16.py."""
import os

import numpy as np
import pytest
import torch

import grad_bars as gb
from util import T, close, close_robust

import inputs as gi

pytestmark = pytest.mark.gpu

SWITCH = "PCA_WGRAD_FOLD"
D, H, M, C = 128, 4, 16, 10

CASES = [  # B, N, din, lengths
    (3, 256, 2, None),                # set-resident; 768 rows: workgroups of 512 and of 256 rows
    (5, 512, 3, None),
    (3, 300, 2, None),                # per-block path, materialised dZ; 900 rows end in a ragged tile
    (3, 300, 2, [300, 257, 33]),
    (1, 256, 2, None),                # an fp32 job of 16 rows, the PMA's of 1 row: less than one tile
    (9, 128, 2, None),                # 1152 rows: one workgroup of 1024 and one of 128
]
IDS = [f"B{c[0]}-N{c[1]}-din{c[2]}" + ("-lengths" if c[3] else "") for c in CASES]


@pytest.fixture(scope="module")
def dev():
    import pca_hip
    pca_hip.lib()
    return torch.device("cuda", 0)


def _net(dev, din, seed):
    import models
    torch.manual_seed(seed)
    return models.ST(dim_input=din, num_outputs=1, dim_output=C, num_inds=M, dim_hidden=D,
                     num_heads=H).to(dev)


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


def _inputs(case):
    B, N, din, lengths = case
    X = gi.pc_input(8600 + N + B, B, N, din)
    if lengths is not None:
        for b, L in enumerate(lengths):        # padding rows: zeros, as the pack kernel writes
            X[b, L:] = 0.0
    return X, gi.labels(8601 + N + B, B, C)


def _run(net, case, X, y, fold, witness=False):
    """One eager train step with the switch set; witness: also the kernel names of one more step."""
    from pca_hip import _lib, trainer
    B, N, din, lengths = case
    dev = next(net.parameters()).device
    ld = None if lengths is None else torch.tensor(lengths, dtype=torch.int32, device=dev)
    old = os.environ.get(SWITCH)
    os.environ[SWITCH] = "1" if fold else "0"
    try:
        eng = trainer.STEngine(net, B, N, _lib.MODE_BF16, training=True)
        eng.fwd_bwd(X, y, phase=-1, lengths=ld)
        torch.cuda.synchronize()
        eng.check_handoffs()
        out = eng.logits.clone(), eng.loss.clone(), eng.grads.clone()
        if witness:
            names = _kernels(lambda: eng.fwd_bwd(X, y, phase=-1, lengths=ld))
            eng.check_handoffs()
            return (*out, names)
        return out
    finally:
        if old is None:
            del os.environ[SWITCH]
        else:
            os.environ[SWITCH] = old


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


@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_fold_equals_two_launches(dev, case):
    B, N, din, lengths = case
    net = _net(dev, din, 700 + N + din)
    Xn, yn = _inputs(case)
    X, y = T(Xn, dev), T(yn, dev)
    r0 = _run(net, case, X, y, fold=False, witness=True)
    r1 = _run(net, case, X, y, fold=True, witness=True)
    r2 = _run(net, case, X, y, fold=True)
    k0, k1 = r0[3], r1[3]
    print(f"B={B} N={N} din={din} lengths={lengths}: library launches {len(k0)} -> {len(k1)}")
    assert sum("k_wgrad128" in n for n in k0) == 2, k0
    assert sum("k_wgrad128" in n for n in k1) == 1, k1
    assert sum("k_wgrad128_step" in n for n in k1) == 1, k1
    assert len(k1) == len(k0) - 1, (len(k0), len(k1), k0, k1)
    _same_bits(net, r1, r0, "one launch vs two")
    _same_bits(net, r2, r1, "one launch, second pass")


def _oracle(net, case, Xn, yn):
    """loss, logits [B, C] and gradients of the oracle (on X[b, :lengths[b]] where there are lengths)."""
    from oracle import st_oracle as orc
    B, N, din, lengths = case
    p = {k: v.detach().cpu().clone() for k, v in net.state_dict().items()}
    if lengths is None:
        loss, lg, g = orc.st_grads(torch.from_numpy(Xn), torch.from_numpy(yn), p, H)
        return loss, lg.reshape(B, C), g
    params = {k: v.requires_grad_(True) for k, v in p.items()}
    lg = torch.cat([orc.st_forward(torch.from_numpy(Xn[b:b + 1, :lengths[b]]), params, H).reshape(1, -1)
                    for b in range(B)], 0)
    loss = orc.cross_entropy(lg, torch.from_numpy(yn))
    loss.backward()
    return float(loss), lg.detach(), {k: v.grad for k, v in params.items()}


@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_fold_vs_oracle(dev, case):
    B, N, din, lengths = case
    net = _net(dev, din, 750 + N + din)
    Xn, yn = _inputs(case)
    ref_loss, ref_lg, ref_g = _oracle(net, case, Xn, yn)
    lg, loss, g = _run(net, case, T(Xn, dev), T(yn, dev), fold=True)
    close(lg, ref_lg, 3e-2, "logits")
    assert abs(float(loss) - ref_loss) < 3e-2 * max(1.0, abs(ref_loss))
    off = 0
    for k, prm in net.named_parameters():
        close_robust(g[off:off + prm.numel()].view_as(prm), ref_g[k], 5e-2, k,
                     outlier_frac=5e-3 if lengths is None else 2e-3)
        off += prm.numel()
    gb.judge(g, ref_g, gb.BF16_VS_ORACLE, gb.shapes_of(net),
             f"B={B} N={N} din={din} lengths={lengths} one wgrad launch vs oracle")


@pytest.fixture
def guard_workspaces():
    """Every scratch / saved block the autograd glue hands to the library is followed by a guard region,
    verified after the test (pca_hip.ops.check_canaries)."""
    from pca_hip import ops
    ops.CANARY = True
    ops._guards.clear()
    try:
        yield
        ops.check_canaries()
    finally:
        ops.CANARY = False
        ops._guards.clear()


def test_mab1_bwd_f32_activations_ragged(dev, guard_workspaces):
    """The many-queries block on fp32 activations, B = 3, N = 130: its fc_q weight gradient is the
    non-deferred k_wgrad128<bf16, float> launch over 390 rows (a ragged last tile).  Against autograd of
    the oracle's bf16-operand emulation (same rounding points, hence the same ReLU mask), at the
    tolerances of tests/test_gpu_bf16.py:test_mab1_bwd_bf16."""
    import modules
    import pca_hip
    from oracle import st_oracle as orc
    B, N = 3, 130
    g = torch.Generator().manual_seed(4130)
    p = {}
    for nm in ("fc_q", "fc_k", "fc_v", "fc_o"):
        bound = 1.0 / np.sqrt(D)
        p[nm + ".weight"] = (torch.rand(D, D, generator=g) * 2 - 1) * bound
        p[nm + ".bias"] = (torch.rand(D, generator=g) * 2 - 1) * bound
    X = torch.randn(B, N, D, generator=g)
    Hk = torch.randn(B, M, D, generator=g)
    G = torch.randn(B, N, D, generator=g)
    leaves = {k: v.clone().requires_grad_(True) for k, v in p.items()}
    Xe, He = X.clone().requires_grad_(True), Hk.clone().requires_grad_(True)
    Ye = orc.mab1_forward_bf16emu(Xe, He, leaves, H)
    (Ye * G).sum().backward()
    emu = {k: v.grad for k, v in leaves.items()}
    emu["dQ"], emu["dK"] = Xe.grad, He.grad

    mab = modules.MAB(D, D, D, H).to(dev)
    mab.load_state_dict(p)
    Xd = X.to(dev).requires_grad_(True)
    Hd = Hk.to(dev).requires_grad_(True)
    pca_hip.set_mode("bf16")
    try:
        Y = mab(Xd, Hd)
        names = _kernels(lambda: (Y * G.to(dev)).sum().backward())
    finally:
        pca_hip.set_mode("f32")
    assert any("k_wgrad128" in n and "_step" not in n for n in names), names
    close(Y, Ye, 2e-3, "Y vs bf16 emulation")
    got = {"dQ": Xd.grad, "dK": Hd.grad}
    for k, prm in mab.named_parameters():
        got[k] = prm.grad
    for k, v in got.items():
        if k == "fc_k.bias":
            # d/d(bk) is identically 0 (softmax is shift invariant): what is left is the rounding
            # noise of sums of dKp rows, so judge it on the scale of d/d(Wk)
            sc = max(1.0, float(emu["fc_k.weight"].abs().max()))
            assert float((v.cpu() - emu[k]).abs().max()) <= 1.5e-2 * sc
        else:
            close_robust(v, emu[k], 1.5e-2, k, outlier_frac=2e-4)
