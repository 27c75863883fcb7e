"""The bf16 weight-gradient list of a d = 128 step in the launch of layer 1's few-queries backward
(csrc/wgrad128.hip: k_mab0_small_ride; csrc/mab0_bwd_small_body.hpp; csrc/bwd_defer.hip: bwd_defer_ride)
against

* today's launches (``PCA_WGRAD_RIDE=0``: k_mab0_bwd_small<true>, then the list in k_wgrad128_step): the same
  row partition, tiles, slabs and order of the slab sums, and the same (row, point partition) split of the
  per-set backward with one 512-thread workgroup per set in place of two of 256, so logits, loss and all
  45 gradients are the same bits;
* itself: two passes are bitwise equal;
* the CPU oracle (``oracle/st_oracle.py:st_grads``; on the truncated sets where the batch has lengths) at
  the tolerances tests/test_gpu_wgrad128_fold.py::test_fold_vs_oracle uses for the same shapes.

Launch witness: the kernels of one eager step as the profiler of torch sees them.  With the switch on the
step shows no k_mab0_bwd_small, one k_wgrad128_step and one k_mab0_small_ride; with it off one
k_mab0_bwd_small, one k_wgrad128_step and no k_mab0_small_ride; the same number of library kernels in both.

Where the new form does not apply (``PCA_D128_MIDFUSE=0``, ``PCA_WGRAD_SLABS=0``) the step runs today's
kernels whatever the switch says, and a phase-split step (phase 0, then phase 1) rides in phase 1 only.

The shapes are the smallest at which the joint grid (job rows beside one row of sets, either of them the
wider one) and the 512-thread set row (eight point partitions of 64 rows, dk = 2 and 3, lengths, less than
one, one and two point chunks per set) can go wrong.  Every engine pass of a case runs once and is shared
by the tests of that case."""
import contextlib
import functools
import os

import pytest
import torch

import grad_bars as gb
from util import T, close, close_robust

import inputs as gi

pytestmark = pytest.mark.gpu

SWITCH = "PCA_WGRAD_RIDE"
RIDE, SMALL, STEP = "k_mab0_small_ride", "k_mab0_bwd_small", "k_wgrad128_step"
D, H, M, C = 128, 4, 16, 10

CASES = [  # B, N, din, lengths
    (3, 256, 2, None),                # set-resident forward; workgroups of 512 and 256 rows; sets > job rows
    (5, 512, 3, None),                # dk = 3 guards of the small body and of the mid chain's SMALL branch
    (3, 300, 2, None),                # per-block path, materialised dZ (no mask words), ragged last tile
    (3, 300, 2, (300, 257, 33)),      # lengths in the set rows
    (1, 1024, 2, None),               # one set row, two job workgroups per job
    (9, 128, 2, None),                # 1152 rows: one workgroup of 1024 and one of 128; N below a point chunk
    (13, 2048, 2, None),              # per-block path, two point chunks per set
]
IDS = [f"B{c[0]}-N{c[1]}-din{c[2]}" + ("-lengths" if c[3] else "") for c in CASES]
ORACLE_CASES = [c for c in CASES if c[1] != 2048]        # (N = 2048: against the switch-off form only)
ORACLE_IDS = [i for c, i in zip(CASES, IDS) if c[1] != 2048]


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
    """Names of the library's device kernels one call of fn() launches."""
    from torch.profiler import ProfilerActivity, profile
    torch.cuda.synchronize()
    with profile(activities=[ProfilerActivity.CPU, ProfilerActivity.CUDA]) as prof:
        fn()
        torch.cuda.synchronize()
    cuda = getattr(torch.autograd.DeviceType, "CUDA", None)
    names = [e.name for e in prof.events() if e.device_type == cuda]
    return [n for n in names if "pca" in n]


def _inputs(case):
    B, N, din, lengths = case
    X = gi.pc_input(9100 + N + B, B, N, din)
    if lengths is not None:
        for b, L in enumerate(lengths):        # padding rows: zeros, as the pack kernel writes
            X[b, L:] = 0.0
    return X, gi.labels(9101 + N + B, B, C)


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


def _run(net, case, X, y, ride, witness=False, split=False, **env):
    """One eager train step (split: phase 0, then phase 1) with the switch set; witness: also the kernel
    names of one more step."""
    from pca_hip import _lib, trainer
    B, N, din, lengths = case
    dev = next(net.parameters()).device
    ld = None if lengths is None else torch.tensor(lengths, dtype=torch.int32, device=dev)

    def step():
        for ph in ((0, 1) if split else (-1,)):
            eng.fwd_bwd(X, y, phase=ph, lengths=ld)

    with _env(**{SWITCH: "1" if ride else "0"}, **env):
        eng = trainer.STEngine(net, B, N, _lib.MODE_BF16, training=True)
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
    """The net and inputs of a case and its three engine passes: switch off, on, on again."""
    dev = torch.device("cuda", 0)
    B, N, din, lengths = case
    net = _net(dev, din, 900 + N + din)
    Xn, yn = _inputs(case)
    X, y = T(Xn, dev), T(yn, dev)
    r0 = _run(net, case, X, y, ride=False, witness=True)
    r1 = _run(net, case, X, y, ride=True, witness=True)
    r2 = _run(net, case, X, y, ride=True)
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
def test_ride_equals_separate_launches(dev, case):
    net, _, _, _, _, r0, r1, r2 = _passes(case)
    _same_bits(net, r1, r0, "joint launch vs separate launches")
    _same_bits(net, r2, r1, "joint launch, second pass")


@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_ride_kernel_names(dev, case):
    B, N, din, lengths = case
    _, _, _, _, _, r0, r1, _ = _passes(case)
    k0, k1 = r0[3], r1[3]
    print(f"B={B} N={N} din={din} lengths={lengths}: library launches {len(k0)} (off), {len(k1)} (on)")
    assert (_count(k1, SMALL), _count(k1, STEP), _count(k1, RIDE)) == (0, 1, 1), k1
    assert (_count(k0, SMALL), _count(k0, STEP), _count(k0, RIDE)) == (1, 1, 0), k0
    assert len(k1) == len(k0), (len(k0), len(k1), k0, k1)


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


@pytest.mark.parametrize("case", ORACLE_CASES, ids=ORACLE_IDS)
def test_ride_vs_oracle(dev, case):
    B, N, din, lengths = case
    net, Xn, yn, _, _, _, r1, _ = _passes(case)
    ref_loss, ref_lg, ref_g = _oracle(net, case, Xn, yn)
    lg, loss, g = r1[:3]
    close(lg, ref_lg, 3e-2, "logits")
    assert abs(float(loss) - ref_loss) < 3e-2 * max(1.0, abs(ref_loss))
    off = 0
    for k, prm in net.named_parameters():
        close_robust(g[off:off + prm.numel()].view_as(prm), ref_g[k], 5e-2, k,
                     outlier_frac=5e-3 if lengths is None else 2e-3)
        off += prm.numel()
    gb.judge(g, ref_g, gb.BF16_VS_ORACLE, gb.shapes_of(net),
             f"B={B} N={N} din={din} lengths={lengths} joint launch vs oracle")


FALLBACK = CASES[0]


def test_ride_off_without_fused_mid_chain(dev):
    """PCA_D128_MIDFUSE=0: the mid chain is a launch of its own, so there is nothing to ride in."""
    net, _, _, X, y, _, _, _ = _passes(FALLBACK)
    r0 = _run(net, FALLBACK, X, y, ride=False, witness=True, PCA_D128_MIDFUSE="0")
    r1 = _run(net, FALLBACK, X, y, ride=True, witness=True, PCA_D128_MIDFUSE="0")
    for k in (r0[3], r1[3]):
        assert (_count(k, SMALL), _count(k, STEP), _count(k, RIDE), _count(k, "k_mid_bwd")) == (1, 1, 0, 2), k
    assert r0[3] == r1[3]
    _same_bits(net, r1, r0, "mid chain as a launch, switch on vs off")


def test_ride_off_without_slabs(dev):
    """PCA_WGRAD_SLABS=0: fp32 atomics, no slabs to place early.  The atomics are not bit-stable: the two
    passes are peers."""
    net, _, _, X, y, _, _, _ = _passes(FALLBACK)
    r0 = _run(net, FALLBACK, X, y, ride=False, witness=True, PCA_WGRAD_SLABS="0")
    r1 = _run(net, FALLBACK, X, y, ride=True, witness=True, PCA_WGRAD_SLABS="0")
    for k in (r0[3], r1[3]):
        assert (_count(k, SMALL), _count(k, STEP), _count(k, RIDE)) == (1, 1, 0), k
    assert r0[3] == r1[3]
    assert torch.equal(r1[0], r0[0]), "logits moved"
    gb.judge(r1[2], r0[2], gb.PEER, gb.shapes_of(net), "atomics, switch on vs off")


def test_ride_split_step(dev):
    """phase 0 (no layer-1 block: flushed as before), then phase 1 (its bf16 list is layer 1's dWo alone)."""
    net, _, _, X, y, _, _, _ = _passes(FALLBACK)
    s0 = _run(net, FALLBACK, X, y, ride=False, witness=True, split=True)
    s1 = _run(net, FALLBACK, X, y, ride=True, witness=True, split=True)
    assert (_count(s1[3], SMALL), _count(s1[3], RIDE)) == (0, 1), s1[3]
    assert (_count(s0[3], SMALL), _count(s0[3], RIDE)) == (1, 0), s0[3]
    assert len(s0[3]) == len(s1[3])
    _same_bits(net, s1, s0, "split step, switch on vs off")
