"""The fused kernels at the edges of the predicates that route work to them, each case against the CPU
oracle (oracle/st_oracle.py) AND with the path it took witnessed (tests/dispatch.py: the library's
launch counter per kernel family), so that a case that quietly lands on another path - the exact chain
meets a bf16 tolerance trivially - fails instead of passing.

Predicates and the branches covered here:

* ``set128_shape_ok`` (csrc/set128_fwd.hip): din 1..4, N 256 / 512, 16 * cdiv(B, 8) <= CUs - din 1 and 4,
  B = 1 / 8 / 9, the largest B that fits and the first that does not, N = 384 (refused: per-block);
* ``mab1_bf16_supported`` (csrc/mab1_bf16.hip): dq = d or dq <= 4, nk 16 / 32 - dq 1 and 4 at d = 128 and
  256; nk = 32 at d = 128 (fused mab1 next to an exact mab0);
* ``mab0_bf16_supported`` (csrc/mab0_bf16.hip), d = 128: nq = 16 or nq <= 2, dk <= 4 with R = h nq in
  {64, 128, 256} - nq = 2 (PMA with two seeds), dk 1 and 4;
* ``mab0_d256_supported`` (csrc/d256_host.hip): dk <= 4 with R in {64, 128, 256} - R = 64 / 128 (the
  reassociated kernels at 8 and 16 queries), dk 1 and 4 at R = 256;
* ``sd64_kind`` (csrc/sd64_fwd.hip): dq / dk <= 4 - din 1 and 4, PMA with two seeds;
* the engine with k = 2 PMA seeds (csrc/st_engine.hip: inference runs the PMA epilogue and the
  classifier over B k rows; the train step refuses k != 1);
* mixed dispatch (``shapes()`` in csrc/st_engine.hip): some blocks fused, others on the exact chain, fp32
  activations in between.
"""
import contextlib
import ctypes as C
import os

import numpy as np
import pytest
import torch

from dispatch import launches
import grad_bars as gb
from util import T, close, close_robust

import inputs as gi

pytestmark = pytest.mark.gpu

FWD_TOL = 1.5e-2          # test_gpu_bf16.py
BWD_TOL = 3e-2
ST_FWD_TOL = 3e-2         # test_gpu_set128.py: whole train step vs the oracle
ST_BWD_TOL = 5e-2
F8_FWD_TOL = 6e-2         # test_gpu_fullsize.py: fp8 mode vs the exact oracle
F8_BWD_TOL = 1e-1

FUSED = ("mab1_fwd", "mab1_bwd", "mab0_fwd", "mab0_bwd")


@pytest.fixture(scope="module")
def dev():
    import pca_hip
    pca_hip.lib()
    yield torch.device("cuda", 0)
    pca_hip.set_mode("f32")


@pytest.fixture(autouse=True)
def _guard_workspaces():
    """Scratch / saved blocks handed to the library by the autograd glue carry guard regions."""
    from pca_hip import ops
    ops.CANARY = True
    ops._guards.clear()
    try:
        yield
        ops.check_canaries()
    finally:
        ops.CANARY = False
        ops._guards.clear()


@contextlib.contextmanager
def _env(**kv):
    old = {k: os.environ.get(k) for k in kv}
    for k, v in kv.items():
        os.environ[k] = v
    try:
        yield
    finally:
        for k, v in old.items():
            if v is None:
                del os.environ[k]
            else:
                os.environ[k] = v


def _net(dev, din, d, h, m, C, k=1, seed=0):
    import models
    torch.manual_seed(seed)
    return models.ST(dim_input=din, num_outputs=k, dim_output=C, num_inds=m, dim_hidden=d,
                     num_heads=h).to(dev)


def _params(net):
    return {k: v.detach().cpu().clone() for k, v in net.state_dict().items()}


def _train(dev, net, Xn, yn, mode, set128=True, families=FUSED + ("set_fwd", "gemm_f32")):
    """One eager train step of the whole-model engine -> (logits, loss, grads, launch counts, engine);
    the counts come from further eager steps of the same engine, one per family."""
    from pca_hip import trainer
    B, N = Xn.shape[:2]
    X, y = T(Xn, dev), T(yn, dev)
    with _env(PCA_SET128="1" if set128 else "0"):
        eng = trainer.STEngine(net, B, N, mode, training=True)
        # every workspace byte 0xFF (NaN in fp32 and bf16): a value the step reads without having written
        # it this step comes out non-finite instead of as whatever the allocator left there
        eng.ws.fill_(255)
        if eng._handoff_word is not None:
            eng._handoff_word.zero_()        # (the caller's word: counts expired hand-off waits)
        eng.fwd_bwd(X, y, phase=-1)
        torch.cuda.synchronize()
        eng.check_handoffs()
        out = eng.logits.clone(), float(eng.loss), eng.grads.clone()
        n = launches(lambda: eng.fwd_bwd(X, y, phase=-1), families)
        eng.check_handoffs()
    return (*out, n, eng)


def _vs_oracle(net, Xn, yn, h, lg, loss, g, ftol=ST_FWD_TOL, gtol=ST_BWD_TOL, frac=5e-3,
               bar=gb.BF16_VS_ORACLE):
    from oracle import st_oracle as orc
    B = Xn.shape[0]
    # a ReLU of the PMA's fc_o whose bf16-rounded pre-activation changes sign moves a whole row of that
    # weight's gradient (1/d of it); with a few sets (B k rows) one such flip is the likely case
    frac = max(frac, 2.0 / net.dec[0].mab.dim_V)
    ref_loss, ref_lg, ref_g = orc.st_grads(torch.from_numpy(Xn), torch.from_numpy(yn), _params(net), h)
    e = close(lg, ref_lg.reshape(B, -1), ftol, "logits vs oracle")
    assert abs(loss - ref_loss) < ftol * max(1.0, abs(ref_loss)), (loss, ref_loss)
    off, worst = 0, 0.0
    for k, prm in net.named_parameters():
        worst = max(worst, close_robust(g[off:off + prm.numel()].view_as(prm), ref_g[k], gtol,
                                        k + " vs oracle", outlier_frac=frac))
        off += prm.numel()
    assert off == g.numel()
    gb.judge(g, ref_g, bar, gb.shapes_of(net), f"B={B} N={Xn.shape[1]} vs oracle",
             outlier_frac=max(frac, bar.outlier_frac), zero=gb.SINGLE_KEY if Xn.shape[1] == 1 else ())
    return e, worst


def _vs_per_block(net, lg1, loss1, g1, lg0, loss0, g0):
    """Set-resident launch vs the per-block launches (test_gpu_set128.py's tolerances)."""
    close(lg1, lg0.cpu(), 4e-3, "logits vs per-block")
    assert abs(loss1 - loss0) < 2e-3 * max(1.0, abs(loss0)), (loss1, loss0)
    off = 0
    for k, prm in net.named_parameters():
        close_robust(g1[off:off + prm.numel()].view_as(prm), g0[off:off + prm.numel()].view_as(prm).cpu(),
                     6e-3, k + " vs per-block", outlier_frac=1e-3)
        off += prm.numel()
    gb.judge(g1, g0, gb.PEER, gb.shapes_of(net), "set-resident vs per-block")


def _max_fitting_batch():
    # set128_shape_ok: the 2 cdiv(B, 8) x 8 workgroups of the pairs must all be resident, one per CU
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    return 8 * (cus // 16)


# ---- 1. layer-1 width din = 1 and 4 on every fused family ----------------------------------------------
@pytest.mark.parametrize("B,N,din", [(5, 256, 1), (7, 512, 4), (3, 512, 1), (9, 256, 4)])
def test_set128_din_edges(dev, B, N, din):
    """k_set128_fwd<DIN> for the two layer-1 widths no benchmark uses (set128_shape_ok: 1 <= din <= 4)."""
    from pca_hip import _lib
    d, h, m, C = 128, 4, 16, 50
    net = _net(dev, din, d, h, m, C, seed=300 + din + N)
    Xn = gi.pc_input(8000 + 10 * din + B, B, N, din)
    yn = gi.labels(8001 + 10 * din + B, B, C)
    lg1, loss1, g1, n1, eng = _train(dev, net, Xn, yn, _lib.MODE_BF16, set128=True)
    assert eng._handoff_word is not None
    assert n1["set_fwd"] == 1, n1          # the set-resident launch, once per eager step
    assert n1["mab0_bwd"] > 0 and n1["mab1_bwd"] > 0, n1
    lg0, loss0, g0, n0, _ = _train(dev, net, Xn, yn, _lib.MODE_BF16, set128=False)
    assert n0["set_fwd"] == 0 and n0["mab0_fwd"] > 0 and n0["mab1_fwd"] > 0, n0
    _vs_per_block(net, lg1, loss1, g1, lg0, loss0, g0)
    _vs_oracle(net, Xn, yn, h, lg1, loss1, g1)
    print(f"set128 B={B} N={N} din={din}: set-resident {n1}, per-block {n0}")


@pytest.mark.parametrize("din", [1, 4])
def test_d256_train_din_edges(dev, din):
    """d = 256 / 8 heads / m = 32 train step (every block on its own fused kernel, bf16 activations):
    layer 1 with dq = 1 / 4 (mab1_bf16_supported: dq <= 4) and dk = 1 / 4 (mab0_d256_supported: R = 256)."""
    from pca_hip import _lib
    d, h, m, C = 256, 8, 32, 20
    B, N = 2, 300
    net = _net(dev, din, d, h, m, C, seed=400 + din)
    Xn = gi.pc_input(8100 + din, B, N, din)
    yn = gi.labels(8101 + din, B, C)
    # layer 1's blocks (the few-queries one has no launch counter) - shapes() takes the bf16 activations
    # only when these are fused as well
    assert _fused_block(B, m, N, d, din, d, h, True) and _fused_block(B, N, m, din, d, d, h, False)
    lg, loss, g, n, eng = _train(dev, net, Xn, yn, _lib.MODE_BF16)
    assert all(n[f] > 0 for f in FUSED), n
    assert n["set_fwd"] == 0 and eng._handoff_word is None, n
    e, w = _vs_oracle(net, Xn, yn, h, lg, loss, g)
    print(f"d256 din={din}: {n}; logits {e:.2e}, worst grad {w:.2e}")


def _infer(dev, net, Xn, mode):
    from pca_hip import trainer
    B, N = Xn.shape[:2]
    X = T(Xn, dev)
    eng = trainer.STEngine(net, B, N, mode, training=False)
    lg = eng.forward(X).clone()
    n = launches(lambda: eng.forward(X), FUSED + ("gemm_f32",))
    return lg, n


@pytest.mark.parametrize("din", [1, 4])
def test_d64_inference_din_edges(dev, din):
    """The shipped d = 64 / 8 heads / m = 64 shape in the fused mode: all five blocks on the fp32
    sd64 kernels (sd64_kind: dq / dk <= 4 on layer 1), which have no launch counter of their own - the
    witness is that the classifier's Linear is the only k_gemm_f32 launch left (linear_fwd_f32 in
    forward(), csrc/st_engine.hip), where the exact chain issues several per block."""
    from oracle import st_oracle as orc
    from pca_hip import _lib
    d, h, m, C = 64, 8, 64, 10
    B, N = 3, 301
    net = _net(dev, din, d, h, m, C, seed=500 + din)
    Xn = gi.pc_input(8200 + din, B, N, din)
    ref = orc.st_forward(torch.from_numpy(Xn), _params(net), h)
    lg, n = _infer(dev, net, Xn, _lib.MODE_BF16)
    lg32, n32 = _infer(dev, net, Xn, _lib.MODE_F32)
    assert n["gemm_f32"] == 1 and n32["gemm_f32"] > 1, (n, n32)
    # (sd64 computes in fp32: the exact mode's tolerance)
    close(lg, ref, 1e-4, "logits (sd64)")
    close(lg32, ref, 1e-4, "logits (exact chain)")


def _mab_params(dq, dk, d, seed):
    g = torch.Generator().manual_seed(seed)
    p = {}
    for nm, din in (("fc_q", dq), ("fc_k", dk), ("fc_v", dk), ("fc_o", d)):
        bound = 1.0 / np.sqrt(din)
        p[nm + ".weight"] = (torch.rand(d, din, generator=g) * 2 - 1) * bound
        p[nm + ".bias"] = (torch.rand(d, generator=g) * 2 - 1) * bound
    return p


def _fused_block(B, nq, nk, dq, dk, d, h, q_shared, mode=None):
    """True when the library has a fused kernel for this block in bf16 mode (pca_mab_saved_bytes: the
    bf16 mode refuses a shape whose mab_kind() is the exact chain - api_mab.hip, bf16_demand).  The
    witness of the layer-1 few-queries kernels (dk <= 4: k_mab0_attn_small and its d = 256 siblings),
    which have no launch counter of their own."""
    from pca_hip import _lib
    s = _lib.MabShape(B, nq, nk, dq, dk, d, h, int(q_shared), _lib.MODE_BF16 if mode is None else mode,
                      _lib.PCA_F32, _lib.PCA_F32, _lib.PCA_F32, None, 0)
    return _lib.lib().pca_mab_saved_bytes(C.byref(s)) > 0


def _module_case(dev, kind, case, module=None):
    """One MAB (kind 'mab1': many queries X [B, N, dq] over the keys H [B, m, d]; 'mab0': the shared
    learned query [1, m, d] over the keys X [B, N, dk]) forward + backward in bf16 mode against the
    oracle (forward; explicit adjoint) and, for the gradients, tightly against autograd of the bf16
    operand emulation (same ReLU masks: test_gpu_bf16.py).  The fused kernels of that kind must have run."""
    import modules
    import pca_hip
    from emu import mab0_forward_bf16emu
    from oracle import st_oracle as orc
    B, N, m, dw, d, h = case
    g = torch.Generator().manual_seed(17 + sum(case))
    X = torch.randn(B, N, dw, generator=g)
    if dw <= 4:
        X[..., -1] = X[..., -1] * 3 - 9                      # log-magnitude-like column
    if kind == "mab1":
        p = _mab_params(dw, d, d, seed=sum(case))
        K = torch.randn(B, m, d, generator=g)
        Q, q_shared = X, False
        G = torch.randn(B, N, d, generator=g)
        mab = modules.MAB(dw, d, d, h)
        ref = orc.mab_forward(Q, K, p, h)
        exact = orc.mab_backward(G, Q, K, p, h)
        need = {"dQ": dw > 4, "dK": True}
        emu_fwd = orc.mab1_forward_bf16emu
        assert _fused_block(B, N, m, dw, d, d, h, False), case
    else:
        p = _mab_params(d, dw, d, seed=sum(case) + 7)
        Q = torch.randn(1, m, d, generator=g) * 0.5
        K, q_shared = X, True
        G = torch.randn(B, m, d, generator=g)
        mab = modules.MAB(d, dw, d, h)
        Qb = Q.expand(B, -1, -1).contiguous()
        ref = orc.mab_forward(Qb, K, p, h)
        exact = orc.mab_backward(G, Qb, K, p, h)
        exact["dQ"] = exact["dQ"].sum(0, keepdim=True)
        need = {"dQ": True, "dK": dw > 4}
        emu_fwd = mab0_forward_bf16emu
        assert _fused_block(B, m, N, d, dw, d, h, True), case
    leaves = {k: v.clone().requires_grad_(True) for k, v in p.items()}
    Qe, Ke = Q.clone().requires_grad_(True), K.clone().requires_grad_(True)
    (emu_fwd(Qe, Ke, leaves, h) * G).sum().backward()
    emu = {k: v.grad for k, v in leaves.items()}
    emu["dQ"], emu["dK"] = Qe.grad, Ke.grad
    Kd = K.to(dev).requires_grad_(need["dK"])
    Gd = G.to(dev)
    if module is not None:            # a PMA: its learned seeds S are the shared query
        module.load_state_dict({"S": Q, **{"mab." + k: v for k, v in p.items()}})
        module = module.to(dev)
        mab, Qd = module.mab, module.S

        def fwd():
            return module(Kd)
    else:
        mab.load_state_dict(p)
        mab = mab.to(dev)
        Qd = Q.to(dev).requires_grad_(need["dQ"])

        def fwd():
            return mab(Qd, Kd, q_shared=q_shared)

    def step():
        Y = fwd()
        (Y * Gd).sum().backward()
        return Y

    # the layer-1 few-queries kernels (dk <= 4) have no counter: _fused_block above is their witness
    scoped = kind == "mab1" or dw > 4
    pca_hip.set_mode("bf16")
    try:
        Y = step()
        torch.cuda.synchronize()
        got = {k: Qd.grad.clone() if k == "dQ" else Kd.grad.clone() for k, v in need.items() if v}
        for k, prm in mab.named_parameters():
            got[k] = prm.grad.clone()
        n = launches(step, (f"{kind}_fwd", f"{kind}_bwd", "gemm_f32"))
    finally:
        pca_hip.set_mode("f32")
    if scoped:
        assert n[f"{kind}_fwd"] > 0 and n[f"{kind}_bwd"] > 0, (case, n)
    e = close(Y, ref, FWD_TOL, f"{kind} fwd {case}")
    worst = 0.0
    for k, v in got.items():
        if k == "fc_k.bias":
            # identically 0 (softmax is shift invariant): rounding noise, on the scale of d/d(Wk)
            sc = max(1.0, float(exact["fc_k.weight"].abs().max()))
            assert float((v.cpu() - exact[k]).abs().max()) <= BWD_TOL * sc, k
            continue
        # vs the emulation: a wrong tile cannot hide; vs the exact oracle: the ReLU derivative flips where a
        # bf16-rounded pre-activation changes sign, so more elements may sit beyond the tolerance
        worst = max(worst, close_robust(v, emu[k], 1.5e-2, f"{kind} {k} {case} vs emulation",
                                        outlier_frac=2e-4 if d == 128 else 2e-3))
        close_robust(v, exact[k], BWD_TOL, f"{kind} {k} {case} vs oracle", outlier_frac=5e-2)
    print(f"{kind} {case}: {n}; fwd {e:.2e}, worst grad vs emulation {worst:.2e}")


MAB1_EDGE_CASES = [     # B, N, m, dq, d, h
    (2, 130, 16, 1, 128, 4),
    (3, 77, 16, 4, 128, 4),
    (2, 150, 32, 1, 256, 8),
    (2, 77, 32, 4, 256, 8),
]
MAB0_EDGE_CASES = [     # B, N, m, dk, d, h
    (3, 150, 16, 1, 128, 4),        # d = 128 layer 1: R = 64
    (2, 77, 16, 4, 128, 4),
    (2, 150, 32, 1, 256, 8),        # d = 256 layer 1: R = 256
    (2, 77, 32, 4, 256, 8),
    (2, 333, 8, 2, 256, 8),         # d = 256 layer 1: R = 64 (reassociated)
    (3, 261, 16, 3, 256, 8),        # d = 256 layer 1: R = 128 (reassociated)
]


@pytest.mark.parametrize("case", MAB1_EDGE_CASES, ids=[str(c) for c in MAB1_EDGE_CASES])
def test_mab1_module_din_edges(dev, case):
    _module_case(dev, "mab1", case)


@pytest.mark.parametrize("case", MAB0_EDGE_CASES, ids=[str(c) for c in MAB0_EDGE_CASES])
def test_mab0_module_din_edges(dev, case):
    _module_case(dev, "mab0", case)


# ---- 2. set-resident batch edges ------------------------------------------------------------------
@pytest.mark.parametrize("B", [1, 8, 9])
def test_set128_small_batches_vs_oracle(dev, B):
    """One set (one workgroup pair, seven idle), exactly one group of 8 pairs, and one set past it."""
    from pca_hip import _lib
    d, h, m, C, N, din = 128, 4, 16, 50, 512, 2
    net = _net(dev, din, d, h, m, C, seed=600 + B)
    Xn = gi.pc_input(8300 + B, B, N, din)
    yn = gi.labels(8301 + B, B, C)
    lg, loss, g, n, eng = _train(dev, net, Xn, yn, _lib.MODE_BF16, families=("set_fwd",))
    assert n["set_fwd"] == 1 and eng._handoff_word is not None, n
    e, w = _vs_oracle(net, Xn, yn, h, lg, loss, g)
    print(f"set128 B={B}: logits {e:.2e}, worst grad {w:.2e}")


@pytest.mark.parametrize("edge", ["largest_fitting", "first_refused"])
def test_set128_residency_limit(dev, edge):
    """The largest batch whose workgroup pairs are all resident at once takes the set-resident launch;
    one more set does not (set128_shape_ok) and runs the per-block launches.  Checked against the
    per-block launches (the oracle at this B would cost minutes of CPU)."""
    from pca_hip import _lib
    B = _max_fitting_batch() + (0 if edge == "largest_fitting" else 1)
    d, h, m, C, N, din = 128, 4, 16, 50, 256, 3
    net = _net(dev, din, d, h, m, C, seed=700)
    Xn = gi.pc_input(8400 + B, B, N, din)
    yn = gi.labels(8401 + B, B, C)
    lg1, loss1, g1, n1, eng = _train(dev, net, Xn, yn, _lib.MODE_BF16, set128=True,
                                     families=("set_fwd", "mab0_fwd", "mab1_fwd"))
    if edge == "largest_fitting":
        assert n1["set_fwd"] == 1 and eng._handoff_word is not None, (B, n1)
    else:
        assert n1["set_fwd"] == 0 and eng._handoff_word is None, (B, n1)
        assert n1["mab0_fwd"] > 0 and n1["mab1_fwd"] > 0, (B, n1)
    lg0, loss0, g0, n0, _ = _train(dev, net, Xn, yn, _lib.MODE_BF16, set128=False, families=("set_fwd",))
    assert n0["set_fwd"] == 0, n0
    _vs_per_block(net, lg1, loss1, g1, lg0, loss0, g0)
    print(f"B={B} ({edge}): {n1}")


def test_set128_refuses_n384(dev):
    """N = 384: three 128-point tiles - the fused blocks take it, the set-resident launch does not (N is
    256 or 512 there); the step falls back to the per-block fused launches and still matches the oracle."""
    from pca_hip import _lib
    d, h, m, C, N, din, B = 128, 4, 16, 50, 384, 2, 5
    net = _net(dev, din, d, h, m, C, seed=800)
    Xn = gi.pc_input(8500, B, N, din)
    yn = gi.labels(8501, B, C)
    lg, loss, g, n, eng = _train(dev, net, Xn, yn, _lib.MODE_BF16)
    assert n["set_fwd"] == 0 and eng._handoff_word is None, n
    assert all(n[f] > 0 for f in FUSED), n
    _vs_oracle(net, Xn, yn, h, lg, loss, g)


# ---- 3. two PMA seeds --------------------------------------------------------------------------------
def test_pma_two_seeds_module(dev):
    """PMA(dim = 128, 4 heads, 2 seeds): R = h nq = 8 score rows, mab0_bf16_supported's nq <= 2 branch
    (one query per thread in the epilogue), forward and backward through pca_mab_fwd / pca_mab_bwd."""
    import modules
    _module_case(dev, "mab0", (3, 150, 2, 128, 128, 4), module=modules.PMA(dim=128, num_heads=4,
                                                                           num_seeds=2))


@pytest.mark.parametrize("B", [1, 3])
@pytest.mark.parametrize("mode", ["f32", "bf16"])
@pytest.mark.parametrize("arch", [(128, 4, 16), (256, 8, 32), (64, 8, 64)], ids=["d128", "d256", "d64"])
def test_engine_two_seeds_inference(dev, arch, mode, B):
    """ST(num_outputs = 2) through pca_st_forward: the PMA epilogue runs for both seeds and the classifier
    over B k rows; logits [B k, C] are the oracle's [B, k, C] after the same .squeeze() (B = 1: [k, C])."""
    from oracle import st_oracle as orc
    from pca_hip import _lib
    d, h, m = arch
    k, C, N, din = 2, 10, 200, 2
    net = _net(dev, din, d, h, m, C, k=k, seed=900 + d)
    Xn = gi.pc_input(8600 + d + B, B, N, din)
    ref = orc.st_forward(torch.from_numpy(Xn), _params(net), h)
    md = _lib.MODE_F32 if mode == "f32" else _lib.MODE_BF16
    if mode == "bf16" and d != 64:
        assert _fused_block(B, k, N, d, d, d, h, True)         # the PMA: mab0_bf16_supported nq <= 2 / d256
    lg, n = _infer(dev, net, Xn, md)
    assert tuple(lg.shape) == (B * k, C)
    got = lg.view(B, k, C).squeeze()
    assert got.shape == ref.shape, (got.shape, ref.shape)
    if mode == "f32":
        assert all(n[f] == 0 for f in FUSED) and n["gemm_f32"] > 1, n
        close(got, ref, 1e-4, "logits")
    else:
        # the classifier's Linear is the one fp32 GEMM left when every block is fused
        assert n["gemm_f32"] == 1, n
        if d != 64:     # (d = 64: the sd64 kernels, which have no counter)
            # one counted launch each for enc.1's few-queries block and the PMA (k_mab0_attn at d = 128,
            # the d256_host.hip paths at d = 256); enc.0's (dk = din <= 4) has no counter
            assert n["mab0_fwd"] == 2 and n["mab1_fwd"] > 0, n
        close(got, ref, 1e-4 if d == 64 else FWD_TOL, "logits")


def test_train_step_refuses_two_seeds(dev):
    """The train step is built for k = 1 (pca_st_train_fwd_bwd: PCA_EINVAL otherwise)."""
    from pca_hip import _lib, trainer
    L = _lib.lib()
    net = _net(dev, 2, 128, 4, 16, 10, k=2, seed=1)
    B, N = 2, 256
    eng = trainer.STEngine(net, B, N, _lib.MODE_BF16, training=True)
    X, y = T(gi.pc_input(8700, B, N, 2), dev), T(gi.labels(8701, B, 10), dev)
    rc = L.pca_st_train_fwd_bwd(C.byref(eng.cfg), eng.flat.data_ptr(), X.data_ptr(), None, y.data_ptr(),
                                eng.grads.data_ptr(), eng.loss.data_ptr(), eng.stats.data_ptr(),
                                eng.logits.data_ptr(), 1.0, -1, eng.ws.data_ptr(), eng._stream())
    assert rc == -1, rc                     # PCA_EINVAL
    assert b"k == 1" in L.pca_last_error()
    with pytest.raises(_lib.PcaHipError):
        eng.fwd_bwd(X, y)


# ---- 4. / 5. mixed dispatch -------------------------------------------------------------------------
def test_d256_m16_mixed_dispatch(dev):
    """ST(d = 256, 8 heads, m = 16): the few-queries blocks are fused (layer 1 on the reassociated R = 128
    kernels, mab0_d256_supported), the many-queries blocks are not (mab1_bf16_supported: d = 256 needs
    nk = 32), so the activations between the blocks stay fp32 (shapes(): blocks256 is false)."""
    from pca_hip import _lib
    d, h, m, C, din = 256, 8, 16, 20, 3
    B, N = 3, 257
    net = _net(dev, din, d, h, m, C, seed=1000)
    Xn = gi.pc_input(8800, B, N, din)
    yn = gi.labels(8801, B, C)
    assert _fused_block(B, m, N, d, din, d, h, True)            # layer 1: R = 128, no launch counter
    assert not _fused_block(B, N, m, din, d, d, h, False)       # mab1: refused
    lg, loss, g, n, eng = _train(dev, net, Xn, yn, _lib.MODE_BF16)
    # layer 2's few-queries block and the PMA (d256_host.hip); the exact chain of the many-queries blocks
    # runs k_gemm_bf16 in this mode, which has no counter: its witness is that no fused mab1 launched
    assert n["mab0_fwd"] > 0 and n["mab0_bwd"] > 0, n
    assert n["mab1_fwd"] == 0 and n["mab1_bwd"] == 0, n
    e, w = _vs_oracle(net, Xn, yn, h, lg, loss, g)
    print(f"d256 m16: {n}; logits {e:.2e}, worst grad {w:.2e}")


@pytest.mark.parametrize("mode", ["bf16", "fp8"])
def test_d128_m32_mixed_dispatch(dev, mode):
    """ST(d = 128, 4 heads, m = 32): no ISAB fusion (isab_bf16_supported needs m = 16) and the few-queries
    ISAB blocks on the exact chain (mab0_bf16_supported: nq = 16 or nq <= 2); the PMA stays fused.  bf16:
    the many-queries blocks fused with nk = 32.  fp8: mab1_bf16_supported's f8_ok refuses them (fp8
    projections at d = 128 need nk = 16), so they run on the exact chain as well."""
    from pca_hip import _lib
    d, h, m, C, din = 128, 4, 32, 20, 2
    B, N = 3, 200
    net = _net(dev, din, d, h, m, C, seed=1100)
    Xn = gi.pc_input(8900, B, N, din)
    yn = gi.labels(8901, B, C)
    md = _lib.MODE_BF16 if mode == "bf16" else _lib.MODE_FP8
    assert not _fused_block(B, m, N, d, din, d, h, True, md)    # the ISABs' few-queries blocks
    assert _fused_block(B, N, m, din, d, d, h, False, md) == (mode == "bf16")
    lg, loss, g, n, eng = _train(dev, net, Xn, yn, md)
    assert n["mab0_fwd"] > 0, n                                 # the PMA
    if mode == "bf16":
        assert n["mab1_fwd"] > 0 and n["mab1_bwd"] > 0, n
        e, w = _vs_oracle(net, Xn, yn, h, lg, loss, g)
    else:
        assert n["mab1_fwd"] == 0 and n["mab1_bwd"] == 0, n
        e, w = _vs_oracle(net, Xn, yn, h, lg, loss, g, F8_FWD_TOL, F8_BWD_TOL, 1e-2, bar=gb.FP8_VS_ORACLE)
    assert n["set_fwd"] == 0, n
    print(f"d128 m32 {mode}: {n}; logits {e:.2e}, worst grad {w:.2e}")


# ---- 6. ragged point counts on the per-block fused path ---------------------------------------------
@pytest.mark.parametrize("N", [1, 127, 129, 257, 513])
def test_d128_ragged_points(dev, N):
    """Where the 128-point tiles of the few-queries kernels and the 32-point tiles of the many-queries
    kernels end.  The fused families run, and no more k_gemm_f32 launches than a fully fused step at
    N = 256 makes (the exact fp32 chain of the same model makes more)."""
    from pca_hip import _lib
    d, h, m, C, din, B = 128, 4, 16, 30, 2, 3
    net = _net(dev, din, d, h, m, C, seed=1200)
    Xn = gi.pc_input(9000 + N, B, N, din)
    yn = gi.labels(9001 + N, B, C)
    lg, loss, g, n, eng = _train(dev, net, Xn, yn, _lib.MODE_BF16)
    assert all(n[f] > 0 for f in FUSED) and n["set_fwd"] == 0, n
    X256, y256 = gi.pc_input(9100, B, 256, din), gi.labels(9101, B, C)
    ref = _train(dev, net, X256, y256, _lib.MODE_BF16, set128=False, families=("gemm_f32",))[3]
    exact = _train(dev, net, X256, y256, _lib.MODE_F32, families=("gemm_f32",))[3]
    # a fully fused d = 128 train step has no k_gemm_f32 launch at all: the classifier, the loss and their
    # gradients run in k_pma_head (pma_head_launch, csrc/st_engine.hip), the fused blocks on MFMA kernels
    assert ref["gemm_f32"] == 0 and exact["gemm_f32"] > 0, (ref, exact)
    assert n["gemm_f32"] <= ref["gemm_f32"], (n, ref)
    e, w = _vs_oracle(net, Xn, yn, h, lg, loss, g)
    print(f"N={N}: {n} (fully fused gemm_f32 {ref['gemm_f32']}, exact {exact['gemm_f32']}); "
          f"logits {e:.2e}, worst grad {w:.2e}")
