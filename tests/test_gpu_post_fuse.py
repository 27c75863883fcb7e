"""Both shared-query post stages of a d = 128 step inside k_terminal1 (csrc/bwd_defer.hip: post_fused_body) and
the layer-1 fc_v job as rows of k_wgrad128_step (csrc/wgrad128.hip), against

* the two post launches (``PCA_POST_FUSE=0``: k_terminal1 with the fc_v job, then k_mab0_post2): the same expressions
  on the same operands in the same order, so logits, loss and all 45 gradients are the same bits;
* itself: two passes are bitwise equal;
* the CPU oracle (``oracle/st_oracle.py:st_grads``) under the bf16 bars of grad_bars.

Launch witness: the kernels of one eager step as the profiler of torch sees them.  With the form on the step
shows no k_mab0_post2, one k_terminal1 and one k_wgrad128_step, one library kernel fewer than with it off.
With ``PCA_WGRAD_FOLD=0`` (no k_wgrad128_step) the fc_v job rides with the fp32 list's own k_wgrad128 launch and the
form still applies, and so it does with ``PCA_WGRAD_SLABS=0`` (the fc_v job adds atomically inside k_terminal1 and
leaves no partials).  A d = 256 step runs k_terminal1 and k_mab0_post2 whatever the switch says (its post jobs have a
shape the fused rows do not cover).

A Trainer run (three steps replayed from the captured graph, B = 5: the flag-clear job of the step's first launch
has a byte count that is no multiple of 16) leaves the same parameters and Adam moments with the form on and off.

Shapes: d = 128, h = 4, m = 16, N = 256, C = 10, the smallest at which every piece is present; B = 1 gives
single-slab sums and a one-row PMA job, B = 5 gives 80 fc_v rows (a ragged second workgroup), B = 13 odd grids.
Every engine pass of a case runs once and is shared by the tests of that case."""
import contextlib
import functools
import os

import numpy as np
import pytest
import torch

import grad_bars as gb
from util import T, close, close_robust

import inputs as gi

pytestmark = pytest.mark.gpu

SWITCH = "PCA_POST_FUSE"
POST2, TERM, STEP = "k_mab0_post2", "k_terminal1", "k_wgrad128_step"
D, H, M, N, C = 128, 4, 16, 256, 10

CASES = [(B, din, set128) for din in (2, 3) for B in (1, 5, 13) for set128 in (True, False)]  # B, din, PCA_SET128
IDS = [f"B{c[0]}-din{c[1]}-" + ("set128" if c[2] else "per-block") for c in CASES]
ORACLE_CASES = [(5, 2, True), (13, 3, True)]
ORACLE_IDS = [IDS[CASES.index(c)] for c in ORACLE_CASES]


@pytest.fixture(scope="module")
def dev():
    import pca_hip
    pca_hip.lib()
    return torch.device("cuda", 0)


def _net(dev, din, seed, d=D, h=H, m=M):
    import models
    torch.manual_seed(seed)
    return models.ST(dim_input=din, num_outputs=1, dim_output=C, num_inds=m, dim_hidden=d,
                     num_heads=h).to(dev)


def _kernels(fn):
    """Names of the library's device kernels one call of fn() launches."""
    from torch.profiler import ProfilerActivity, profile
    torch.cuda.synchronize()
    with profile(activities=[ProfilerActivity.CPU, ProfilerActivity.CUDA]) as prof:
        fn()
        torch.cuda.synchronize()
    cuda = getattr(torch.autograd.DeviceType, "CUDA", None)
    names = [e.name for e in prof.events() if e.device_type == cuda]
    return [n for n in names if "pca" in n]


@contextlib.contextmanager
def _env(**kv):
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


def _run(net, B, X, y, fuse, set128=True, witness=False, n=N, **env):
    """One eager train step with the switch set; witness: also the kernel names of one more step."""
    from pca_hip import _lib, trainer

    with _env(**{SWITCH: "1" if fuse else "0", "PCA_SET128": "1" if set128 else "0"}, **env):
        eng = trainer.STEngine(net, B, n, _lib.MODE_BF16, training=True)

        def step():
            eng.fwd_bwd(X, y, phase=-1)

        step()
        torch.cuda.synchronize()
        eng.check_handoffs()
        out = eng.logits.clone(), eng.loss.clone(), eng.grads.clone()
        if witness:
            names = _kernels(step)
            eng.check_handoffs()
            return (*out, names)
        return out


@functools.lru_cache(maxsize=None)
def _passes(case):
    """The net and inputs of a case and its three engine passes: form off, on, on again."""
    dev = torch.device("cuda", 0)
    B, din, set128 = case
    net = _net(dev, din, 700 + B + din)
    Xn, yn = gi.pc_input(9300 + B + din, B, N, din), gi.labels(9301 + B + din, B, C)
    X, y = T(Xn, dev), T(yn, dev)
    r0 = _run(net, B, X, y, fuse=False, set128=set128, witness=True)
    r1 = _run(net, B, X, y, fuse=True, set128=set128, witness=True)
    r2 = _run(net, B, X, y, fuse=True, set128=set128)
    return net, Xn, yn, X, y, r0, r1, r2


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


def _count(names, sub):
    return sum(sub in n for n in names)


@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_fused_equals_two_launches(dev, case):
    net, _, _, _, _, r0, r1, r2 = _passes(case)
    _same_bits(net, r1, r0, "post stages in k_terminal1 vs k_terminal1 + k_mab0_post2")
    _same_bits(net, r2, r1, "post stages in k_terminal1, second pass")


@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_fused_kernel_names(dev, case):
    _, _, _, _, _, r0, r1, _ = _passes(case)
    k0, k1 = r0[3], r1[3]
    print(f"{case}: library launches {len(k0)} (off), {len(k1)} (on)")
    assert (_count(k1, POST2), _count(k1, TERM), _count(k1, STEP)) == (0, 1, 1), k1
    assert (_count(k0, POST2), _count(k0, TERM), _count(k0, STEP)) == (1, 1, 1), k0
    assert len(k1) == len(k0) - 1, (len(k0), len(k1), k0, k1)


@pytest.mark.parametrize("case", ORACLE_CASES, ids=ORACLE_IDS)
def test_fused_vs_oracle(dev, case):
    from oracle import st_oracle as orc
    B, din, _ = case
    net, Xn, yn, _, _, _, r1, _ = _passes(case)
    p = {k: v.detach().cpu().clone() for k, v in net.state_dict().items()}
    ref_loss, ref_lg, ref_g = orc.st_grads(torch.from_numpy(Xn), torch.from_numpy(yn), p, H)
    lg, loss, g = r1[:3]
    close(lg, ref_lg.reshape(B, C), 3e-2, "logits")
    assert abs(float(loss) - ref_loss) < 3e-2 * max(1.0, abs(ref_loss))
    off = 0
    for k, prm in net.named_parameters():
        close_robust(g[off:off + prm.numel()].view_as(prm), ref_g[k], 5e-2, k, outlier_frac=5e-3)
        off += prm.numel()
    gb.judge(g, ref_g, gb.BF16_VS_ORACLE, gb.shapes_of(net), f"B={B} din={din} fused post stages vs oracle")


def test_lists_as_two_launches(dev):
    """PCA_WGRAD_FOLD=0: no k_wgrad128_step; the fc_v job then rides with the fp32 list's own k_wgrad128 launch,
    so the form still applies (tests/test_gpu_wgrad128_fold.py holds the folded step to exactly one launch fewer
    than this one): no k_mab0_post2, and the bits of the folded form and of the switch-off form."""
    case = (5, 2, True)
    net, _, _, X, y, _, r1, _ = _passes(case)
    f0 = _run(net, 5, X, y, fuse=False, witness=True, PCA_WGRAD_FOLD="0")
    f1 = _run(net, 5, X, y, fuse=True, witness=True, PCA_WGRAD_FOLD="0")
    assert (_count(f0[3], POST2), _count(f0[3], TERM), _count(f0[3], STEP)) == (1, 1, 0), f0[3]
    assert (_count(f1[3], POST2), _count(f1[3], TERM), _count(f1[3], STEP)) == (0, 1, 0), f1[3]
    assert _count(f1[3], "k_wgrad128") == 2 and len(f1[3]) == len(f0[3]) - 1, (f0[3], f1[3])
    _same_bits(net, f1, f0, "two weight-gradient launches, switch on vs off")
    _same_bits(net, f1, r1, "two weight-gradient launches vs the folded form")


def test_without_slabs(dev):
    """PCA_WGRAD_SLABS=0: fp32 atomics.  The fc_v job stays in k_terminal1 and adds atomically, so it leaves no
    partials for a launch behind it and the post stages still share k_terminal1.  The atomics are not bit-stable:
    the two passes are peers."""
    case = (5, 2, True)
    net, _, _, X, y, _, _, _ = _passes(case)
    f0 = _run(net, 5, X, y, fuse=False, witness=True, PCA_WGRAD_SLABS="0")
    f1 = _run(net, 5, X, y, fuse=True, witness=True, PCA_WGRAD_SLABS="0")
    assert (_count(f0[3], POST2), _count(f0[3], TERM)) == (1, 1), f0[3]
    assert (_count(f1[3], POST2), _count(f1[3], TERM)) == (0, 1), f1[3]
    assert len(f1[3]) == len(f0[3]) - 1, (f0[3], f1[3])
    assert torch.equal(f1[0], f0[0]), "logits moved"
    gb.judge(f1[2], f0[2], gb.PEER, gb.shapes_of(net), "atomics, switch on vs off")


def test_d256_step_keeps_post2(dev):
    """The fused rows cover d = 128; a d = 256 step (m = 32) runs k_mab0_post2 with the switch on, and the switch
    moves no bit of it."""
    B = 3
    net = _net(dev, 2, 731, d=256, h=8, m=32)
    X, y = T(gi.pc_input(9401, B, N, 2), dev), T(gi.labels(9402, B, C), dev)
    r0 = _run(net, B, X, y, fuse=False, witness=True)
    r1 = _run(net, B, X, y, fuse=True, witness=True)
    assert _count(r1[3], POST2) >= 1, r1[3]
    assert r0[3] == r1[3]
    for a, b in zip(r1[:3], r0[:3]):
        assert torch.equal(a, b)


def _bits(t):
    return t.view(torch.int32) if t.dtype == torch.float32 else t


def test_trainer_graph_steps(dev):
    """Three Trainer steps replayed from the captured graph at B = 5 with the set-resident forward: parameters
    and both Adam moments are the same bits with the form on and off."""
    import dataset
    from pca_hip import _lib, trainer
    B, din, steps = 5, 2, 3
    x = np.concatenate([gi.pc_input(9500 + s, B, N, din)[:, :, 1].T for s in range(steps)], axis=1)
    y = np.concatenate([gi.labels(9600 + s, B, C) for s in range(steps)])
    ds = dataset.ESC_pc(x, y, np.linspace(0.0, 0.5, N), device=dev)

    def run(fuse):
        with _env(**{SWITCH: "1" if fuse else "0", "PCA_SET128": "1"}):
            tr = trainer.Trainer(_net(dev, din, 741), ds, B, lr=1e-3, weight_decay=1e-3,
                                 mode=_lib.MODE_BF16, use_graph=True, shuffle=False)
            for _ in range(steps):
                tr.step()
            torch.cuda.synchronize()
            return tr.eng.flat.clone(), tr.m.clone(), tr.v.clone()

    on, off = run(True), run(False)
    assert torch.isfinite(on[0]).all() and float(on[1].abs().max()) > 0
    for a, b, name in zip(on, off, ("parameters", "adam m", "adam v")):
        assert torch.equal(_bits(a), _bits(b)), name
