"""The guarded optimiser step on the device: pca_grad_sumsq / pca_adam_step_ex (csrc/optim.hip) against
tests/optim_ref.py, stock torch and the unguarded kernel, and the Trainer options built on them
(max_grad_norm, skip_nonfinite, lr_schedule): against a stock loop, graph against eager, exact resume,
two ranks, fit.  Run with ``-m gpu``."""
import ctypes as C
import math
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import inputs as gi
import grad_bars as gb
import optim_ref
from conftest import ROOT
from test_gpu_clip import HostReads
from test_gpu_ddp import _free_port
from util import T, close

pytestmark = pytest.mark.gpu

ADAM_TOL = 1e-6          # the bar test_cross_entropy_and_adam holds pca_adam_step to
U = 2.0 ** -24           # half an ulp of fp32, relative


@pytest.fixture(scope="module")
def dev():
    import pca_hip
    pca_hip.lib()
    pca_hip.set_mode("f32")
    return torch.device("cuda", 0)


# ---- the two entry points through ctypes ---------------------------------------------------------------
def _sumsq(x, n=None, ptr=None):
    """(partials as float64 numpy, the device buffer) of one pca_grad_sumsq call; the buffer carries two
    sentinel doubles behind the partials that the launch must leave alone."""
    from pca_hip import _lib
    L = _lib.lib()
    n = x.numel() if n is None else n
    P = int(L.pca_grad_sumsq_partials(n))
    buf = torch.full((P + 2,), -7.0, dtype=torch.float64, device=x.device)
    _lib.check(L.pca_grad_sumsq(x.data_ptr() if ptr is None else ptr, n, buf.data_ptr(), P, None),
               "pca_grad_sumsq")
    host = buf.cpu().numpy()
    assert host[P] == -7.0 and host[P + 1] == -7.0, "wrote past its partials"
    return host[:P].copy(), buf


def _fp32_terms(n, aligned=True):
    """The most terms one thread of k_grad_sumsq adds in fp32: the grid is pca_grad_sumsq_partials(n)
    workgroups of 256 threads; an aligned vector is read as float4 quadruples, grid-strided (4 terms per
    quadruple), and the n % 4 tail gives at most one more term to a thread; a misaligned one is read
    element by element."""
    import pca_hip
    threads = int(pca_hip.lib().pca_grad_sumsq_partials(n)) * 256
    if not aligned:
        return -(-n // threads)
    return 4 * -(-(n // 4) // threads) + (1 if n % 4 else 0)


def _norm_bar(n, aligned=True):
    """A thread's sum of K squares in fp32, acc = fl(acc + fl(x * x)) from acc = 0: each term passes
    through its own rounding of the product and at most K - 1 roundings of later sums, so the sum is off
    by at most (1 + u)^K - 1 ~ K u, relative (all terms are >= 0: no cancellation).  Everything after
    that is fp64 (2^-53 per operation, at most 6 + 4 + 256 of them).  The square root halves a relative
    error: K u / 2, padded by 1 % for the second-order terms.  n = 1 151 026: K = 21, bar 6.3e-7."""
    K = _fp32_terms(n, aligned)
    return 0.5 * K * U * 1.01 + 300 * 2.0 ** -53


SUMSQ_N = [0, 1, 3, 4, 255, 2048, 2049, 292_530, 1_151_026]


@pytest.mark.parametrize("n", SUMSQ_N)
def test_norm_against_float64(dev, n):
    g = torch.Generator().manual_seed(100 + n % 97)
    x = (torch.randn(max(n, 1), generator=g) * 0.37)[:n].contiguous()
    xd = x.to(dev) if n else torch.zeros(4, device=dev)
    parts, _ = _sumsq(xd, n)
    again, _ = _sumsq(xd, n)
    assert parts.view(np.int64).tolist() == again.view(np.int64).tolist()        # the same bits
    want = float(np.sqrt(np.sum(x.numpy().astype(np.float64) ** 2)))
    got = float(np.sqrt(np.sum(parts)))
    bar = _norm_bar(n)
    print(f"n={n}: {len(parts)} partials, {_fp32_terms(n)} fp32 terms a thread, norm {got:.9g} "
          f"(float64 {want:.9g}), rel err {abs(got - want) / max(want, 1e-300):.2e}, bar {bar:.2e}")
    if n == 0:
        assert parts.tolist() == [0.0]
    else:
        assert abs(got - want) <= bar * want


def test_norm_misaligned_pointer_and_nonfinite(dev):
    n = 2049
    g = torch.Generator().manual_seed(8)
    base = torch.randn(n + 1, generator=g)
    based = base.to(dev)
    assert based.data_ptr() % 16 == 0
    parts, _ = _sumsq(based, n, ptr=based.data_ptr() + 4)                        # one float in: scalar path
    want = float(np.sqrt(np.sum(base[1:].numpy().astype(np.float64) ** 2)))
    got = float(np.sqrt(np.sum(parts)))
    assert abs(got - want) <= _norm_bar(n, aligned=False) * want
    again, _ = _sumsq(based, n, ptr=based.data_ptr() + 4)
    assert parts.view(np.int64).tolist() == again.view(np.int64).tolist()
    for bad, judge in ((float("inf"), np.isposinf), (float("-inf"), np.isposinf), (float("nan"), np.isnan)):
        x = base[:n].clone()
        x[1000] = bad
        parts, _ = _sumsq(x.to(dev))
        assert judge(np.sqrt(np.sum(parts))), (bad, parts)


class Dev:
    """p, g, m, v, the step words and the pca_optim_state words of one flat vector on the device."""

    def __init__(self, p, dev):
        self.n = p.numel()
        self.p = p.clone().to(dev)
        self.g = torch.zeros(self.n, device=dev)
        self.m = torch.zeros(self.n, device=dev)
        self.v = torch.zeros(self.n, device=dev)
        self.step = torch.zeros(2, dtype=torch.int32, device=dev)
        self.state = torch.zeros(8, dtype=torch.int32, device=dev)

    def ex(self, grad, max_norm=0.0, skip=0, table=None, lr=1e-3, zero_grad=0, grad_scale=1.0):
        """pca_grad_sumsq + pca_adam_step_ex with test_cross_entropy_and_adam's hyper-parameters."""
        from pca_hip import _lib
        L = _lib.lib()
        self.g.copy_(grad)
        _, buf = _sumsq(self.g)
        o = _lib.OptimCfg(lr, 0.9, 0.999, 1e-8, 1e-3, grad_scale, max_norm, skip)
        _lib.check(L.pca_adam_step_ex(self.p.data_ptr(), self.g.data_ptr(), self.m.data_ptr(),
                                      self.v.data_ptr(), self.n, C.byref(o), buf.data_ptr(),
                                      buf.numel() - 2, None if table is None else table.data_ptr(),
                                      0 if table is None else table.numel(), self.step.data_ptr(),
                                      self.state.data_ptr(), zero_grad, None), "pca_adam_step_ex")
        torch.cuda.synchronize()

    def fields(self):
        h = self.state.cpu()
        return dict(skipped=int(h[0]), clipped=int(h[1]), last_norm=float(h.view(torch.float32)[2]),
                    last_lr=float(h.view(torch.float32)[3]), norm_sum=float(h.view(torch.float64)[2]),
                    norm_count=int(h[6]))


def _adam_inputs():
    """p and five gradients, n = 10007: the draws of test_cross_entropy_and_adam."""
    g = torch.Generator().manual_seed(9)
    torch.randn(37, 50, generator=g)
    torch.randint(0, 50, (37,), generator=g)
    n = 10007
    p = torch.randn(n, generator=g)
    return n, p, [torch.randn(n, generator=g) for _ in range(5)]


def test_no_clip_is_todays_kernel_bitwise(dev):
    """clip == 1, a constant table and no non-finite norm: pca_adam_step_ex is pca_adam_step, bit for bit."""
    from pca_hip import _lib
    L = _lib.lib()
    n, p, grads = _adam_inputs()
    pd, m, v = p.clone().to(dev), torch.zeros(n, device=dev), torch.zeros(n, device=dev)
    step = torch.zeros(2, dtype=torch.int32, device=dev)
    ex = Dev(p, dev)
    table = torch.full((3,), 1e-3, dtype=torch.float32, device=dev)
    for gr in grads:
        gd = gr.to(dev)
        _lib.check(L.pca_adam_step(pd.data_ptr(), gd.data_ptr(), m.data_ptr(), v.data_ptr(), n,
                                   1e-3, 0.9, 0.999, 1e-8, 1e-3, 1.0, step.data_ptr(), 0, None))
        ex.ex(gr, max_norm=1e30, skip=1, table=table)
    torch.cuda.synchronize()
    assert step.tolist() == [5, 0]
    assert torch.equal(ex.step, step)
    for a, b, name in ((ex.p, pd, "p"), (ex.m, m, "m"), (ex.v, v, "v")):
        assert torch.equal(a.view(torch.int32), b.view(torch.int32)), name
    f = ex.fields()
    assert f["skipped"] == 0 and f["clipped"] == 0 and f["norm_count"] == 5
    assert f["last_lr"] == np.float32(1e-3)


def _against_refs(ex, P, ref, truth, what):
    close(ex.p, P["w"], ADAM_TOL, what + " p")
    close(ex.m, ref.m["w"], ADAM_TOL, what + " m")
    close(ex.v, ref.v["w"], ADAM_TOL, what + " v")
    tm, tv = truth.moments("w")
    close(ex.p, truth.p["w"], ADAM_TOL, what + " p (torch.optim.Adam)")
    close(ex.m, tm, ADAM_TOL, what + " m (torch.optim.Adam)")
    close(ex.v, tv, ADAM_TOL, what + " v (torch.optim.Adam)")


def test_clip_against_restatement_and_stock_torch(dev):
    """max_norm = 50 under gradients of norm ~100 (four steps clipped) and ~20 (one not).  m and v are
    compared, not only p: m / sqrt(v) hardly moves under a uniform gradient scale."""
    n, p, grads = _adam_inputs()
    grads[2] = grads[2] * 0.2
    P = {"w": p.clone()}
    ref = optim_ref.OptimRef(P, max_norm=50.0)
    truth = optim_ref.TorchTruth({"w": p}, max_norm=50.0)
    ex = Dev(p, dev)
    for it, gr in enumerate(grads):
        ref.step(P, {"w": gr})
        truth.step({"w": gr})
        ex.ex(gr, max_norm=50.0)
        f = ex.fields()
        assert (ref.last_norm > 50.0) == (it != 2)
        assert abs(f["last_norm"] - ref.last_norm) <= 2 * _norm_bar(n) * ref.last_norm, (it, f, ref.last_norm)
        assert f["clipped"] == ref.clipped
    assert ex.fields()["clipped"] == 4 and ex.fields()["skipped"] == 0
    assert ex.step.tolist() == [5, 0]
    _against_refs(ex, P, ref, truth, "clip")


def test_schedule_table_lookup(dev):
    """A 4-entry table replayed over 6 steps: the rate of step t is table[min(t, 4) - 1], exactly."""
    n, p, grads = _adam_inputs()
    grads.append(grads[0] * 0.5)
    host = [2e-4, 6e-4, 1e-3, 5e-4]
    table = torch.tensor(host, dtype=torch.float64).to(torch.float32).to(dev)
    P = {"w": p.clone()}
    ref = optim_ref.OptimRef(P, table=host)
    truth = optim_ref.TorchTruth({"w": p}, table=host)
    ex = Dev(p, dev)
    for it, gr in enumerate(grads):
        ref.step(P, {"w": gr})
        truth.step({"w": gr})
        ex.ex(gr, table=table, lr=123.0)                         # o->lr is not used with a table
        assert ex.fields()["last_lr"] == float(table[min(it + 1, 4) - 1]) == ref.last_lr
    assert ex.step.tolist() == [6, 0] and ex.fields()["clipped"] == 0
    _against_refs(ex, P, ref, truth, "schedule")


def test_skip_of_a_nonfinite_step(dev):
    """A NaN in the gradient of step 3 of 5: that launch leaves p, m, v bit for bit, clears the gradient,
    counts the skip and still advances step[0]; the run ends where a run that never made step 3 ends."""
    n, p, grads = _adam_inputs()
    grads[2] = grads[2].clone()
    grads[2][4321] = float("nan")
    P = {"w": p.clone()}
    ref = optim_ref.OptimRef(P, max_norm=50.0, skip_nonfinite=True)
    truth = optim_ref.TorchTruth({"w": p}, max_norm=50.0, skip_nonfinite=True)
    ex = Dev(p, dev)
    for it, gr in enumerate(grads):
        before = (ex.p.clone(), ex.m.clone(), ex.v.clone())
        ref.step(P, {"w": gr})
        truth.step({"w": gr})
        ex.ex(gr, max_norm=50.0, skip=1, zero_grad=1)
        assert int(ex.step[0]) == it + 1 and int(ex.step[1]) == 0
        assert float(ex.g.abs().max()) == 0.0                      # cleared, the NaN included
        same = all(torch.equal(a.view(torch.int32), b.view(torch.int32))
                   for a, b in zip(before, (ex.p, ex.m, ex.v)))
        assert same == (it == 2), it
        f = ex.fields()
        assert f["skipped"] == (it >= 2)
        if it == 2:
            assert math.isnan(f["last_norm"])
    f = ex.fields()
    assert f["skipped"] == 1 and f["clipped"] == 4 and f["norm_count"] == 4 and ref.adam.t == 4
    _against_refs(ex, P, ref, truth, "skip")


# ---- the Trainer against a stock loop -------------------------------------------------------------------
def _stock_loop(golden_train, dev, table, max_norm):
    """The module path of test_train_trajectory_golden with torch.nn.utils.clip_grad_norm_ in front of
    the per-tensor pca_adam_step, whose lr is the host table's entry of the step."""
    import models
    import pca_hip
    from pca_hip import _lib
    B, N, din, d, h, m, Cc, steps = [int(v) for v in golden_train["cfg"]]
    net = models.ST(dim_input=din, num_outputs=1, dim_output=Cc, num_inds=m, dim_hidden=d,
                    num_heads=h).to(dev)
    net.load_state_dict({k: T(v) for k, v in golden_train.sub("p0/").items()})
    params = list(net.parameters())
    ms = [torch.zeros_like(p) for p in params]
    vs = [torch.zeros_like(p) for p in params]
    stepc = [torch.zeros(2, dtype=torch.int32, device=dev) for _ in params]
    L = _lib.lib()
    losses, norms = [], []
    for s in range(steps):
        X = T(gi.pc_input(5000 + s, B, N, din), dev)
        y = T(gi.labels(6000 + s, B, Cc), dev)
        loss = pca_hip.cross_entropy(net(X), y)
        net.zero_grad(set_to_none=True)
        loss.backward()
        norms.append(float(torch.nn.utils.clip_grad_norm_(params, max_norm)))
        for p, mm, vv, sc in zip(params, ms, vs, stepc):
            _lib.check(L.pca_adam_step(p.data_ptr(), p.grad.contiguous().data_ptr(), mm.data_ptr(),
                                       vv.data_ptr(), p.numel(), float(np.float32(table[s])), 0.9,
                                       0.999, 1e-8, 1e-3, 1.0, sc.data_ptr(), 0, None))
        losses.append(float(loss))
    torch.cuda.synchronize()
    flat = lambda ts: torch.cat([t.detach().reshape(-1) for t in ts]).cpu()
    return dict(losses=losses, norms=norms, net=net, m=flat(ms), v=flat(vs),
                state={k: v.detach().cpu().clone() for k, v in net.state_dict().items()})


@pytest.fixture(scope="module")
def stock(dev, golden_train):
    from pca_hip import trainer
    steps = int(golden_train["cfg"][7])
    table = trainer.warmup_cosine(1e-3, 5, steps)
    plain = _stock_loop(golden_train, dev, table, float("inf"))        # no clipping: the norms to choose M from
    M = float(np.median(plain["norms"]))
    ref = _stock_loop(golden_train, dev, table, M)
    n_clip = sum(x > M for x in ref["norms"])
    print(f"stock loop: M = {M:.5f}, pre-clip norms {min(ref['norms']):.4f} .. {max(ref['norms']):.4f}, "
          f"{n_clip} of {steps} steps clip")
    assert 1 <= n_clip <= steps - 1, ref["norms"]
    return dict(ref, table=table, M=M, n_clip=n_clip)


MOMENT_BAR = gb.Bar(tol=1e-3, tol_n=1e-3, outlier_frac=0.0, cap=1.0)


@pytest.mark.parametrize("use_graph", [False, True], ids=["eager", "hipgraph"])
def test_trainer_against_stock_loop(dev, golden_train, stock, use_graph):
    import dataset
    import models
    from pca_hip import trainer
    B, N, din, d, h, m, Cc, steps = [int(v) for v in golden_train["cfg"]]
    x = np.concatenate([gi.pc_input(5000 + s, B, N, din)[:, :, 1].T for s in range(steps)], axis=1)
    y = np.concatenate([gi.labels(6000 + s, B, Cc) for s in range(steps)])
    ds = dataset.ESC_pc(x, y, np.linspace(0.0, 0.5, N), device=dev)
    net = models.ST(dim_input=din, num_outputs=1, dim_output=Cc, num_inds=m, dim_hidden=d,
                    num_heads=h).to(dev)
    net.load_state_dict({k: T(v) for k, v in golden_train.sub("p0/").items()})
    tr = trainer.Trainer(net, ds, B, lr=1e-3, weight_decay=1e-3, use_graph=use_graph, shuffle=False,
                         lr_schedule=stock["table"], max_grad_norm=stock["M"])
    losses, norms, lrs = [], [], []
    for s in range(steps):
        tr.step()
        losses.append(float(tr.eng.loss))
        o = tr.read_optim_stats(reset=False)
        norms.append(o["last_grad_norm"])
        lrs.append(o["lr"])
    print("norm rel err", max(abs(a - b) / b for a, b in zip(norms, stock["norms"])),
          "loss err", max(abs(a - b) for a, b in zip(losses, stock["losses"])))
    assert lrs == [float(np.float32(v)) for v in stock["table"]]
    np.testing.assert_allclose(losses, stock["losses"], rtol=0, atol=5e-4)
    np.testing.assert_allclose(norms, stock["norms"], rtol=1e-3, atol=0)
    for k, v in net.state_dict().items():
        close(v, stock["state"][k], 3e-3, k)
    shapes = gb.shapes_of(net)
    gb.judge(tr.m, stock["m"], MOMENT_BAR, shapes, "Trainer.m vs stock loop")
    gb.judge(tr.v, stock["v"], MOMENT_BAR, shapes, "Trainer.v vs stock loop")
    o = tr.read_optim_stats()
    assert o["skipped"] == 0
    # a step whose norm sits within the norm bar of M may fall on either side
    near = sum(abs(x - stock["M"]) <= 1e-3 * stock["M"] for x in stock["norms"])
    assert abs(o["clipped"] - stock["n_clip"]) <= near
    assert abs(o["grad_norm_mean"] - float(np.mean(stock["norms"]))) <= 1e-3 * float(np.mean(stock["norms"]))


# ---- cfg2, bf16: graph against eager, exact resume ----------------------------------------------------------
@pytest.fixture(scope="module")
def cfg2(dev):
    """The cfg2 data of test_trainer_bf16_graph_equals_eager_bitwise, a factory for its model, and the
    median gradient norm of 12 plain steps (measured with skip_nonfinite alone, which changes no step)."""
    import bench
    import models
    from pca_hip import _lib, trainer
    cfg = dict(bench.CONFIGS["cfg2"])
    ds, _ = bench.build_dataset(cfg, 4, dev, seed=0)

    def net():
        torch.manual_seed(1)
        return models.ST(dim_input=2, dim_output=50, num_inds=16, dim_hidden=128, num_heads=4).to(dev)

    tr = trainer.Trainer(net(), ds, 128, mode=_lib.MODE_BF16, seed=1, skip_nonfinite=True)
    norms = []
    for _ in range(12):
        tr.step()
        norms.append(tr.read_optim_stats(reset=False)["last_grad_norm"])
    assert all(math.isfinite(x) and x > 0 for x in norms), norms
    print("cfg2 plain norms", [f"{x:.3f}" for x in norms])
    return dict(ds=ds, net=net, M=float(np.median(norms)))


def _bits(t):
    return t.view(torch.int32) if t.dtype == torch.float32 else t


def test_trainer_bf16_graph_equals_eager_bitwise_options_on(dev, cfg2):
    from pca_hip import _lib, trainer
    table = trainer.warmup_cosine(1e-3, 12, 12)

    def run(graph):
        tr = trainer.Trainer(cfg2["net"](), cfg2["ds"], 128, mode=_lib.MODE_BF16, use_graph=graph, seed=1,
                             keep_grads=True, lr_schedule=table, max_grad_norm=cfg2["M"],
                             skip_nonfinite=True)
        for _ in range(12):
            tr.step()
        torch.cuda.synchronize()
        return (tr.eng.flat.clone(), tr.eng.grads.clone(), tr.m.clone(), tr.v.clone(),
                tr.step_count.clone(), tr.optim_state.clone()), tr.read_optim_stats()

    (g1, o1), (e1, _), (g2, _) = run(True), run(False), run(True)
    print("options on:", o1)
    assert torch.isfinite(g1[0]).all() and float(g1[1].abs().max()) > 0
    assert o1["skipped"] == 0 and o1["lr"] == float(np.float32(table[-1])) and int(g1[4][0]) == 12
    for other in (e1, g2):
        for a, b, name in zip(g1, other, ("parameters", "gradients", "m", "v", "step words", "optim state")):
            assert torch.equal(_bits(a), _bits(b)), name


def test_exact_resume_options_on(dev, cfg2, tmp_path):
    """cfg2, bf16, device cursor, hipGraph replay, 13 steps per epoch: stop after step 8 (mid-epoch, and
    inside the 12-step warm-up), save, load into a fresh Trainer, continue: bit for bit the straight run."""
    import runfiles
    from pca_hip import _lib, trainer
    K = 8
    kw = dict(mode=_lib.MODE_BF16, seed=1, lr_schedule=trainer.warmup_cosine(1e-3, 12, 26),
              max_grad_norm=cfg2["M"], skip_nonfinite=True)

    def state(tr):
        torch.cuda.synchronize()
        return (tr.eng.flat.clone(), tr.m.clone(), tr.v.clone(), tr.step_count.clone(),
                tr.optim_state.clone())

    def same(a, b):
        for x, y, name in zip(a, b, ("parameters", "m", "v", "step_count", "optim state")):
            assert torch.equal(_bits(x), _bits(y)), name

    straight = trainer.Trainer(cfg2["net"](), cfg2["ds"], 128, **kw)
    for _ in range(2 * K):
        straight.step()
    want = state(straight)
    first = trainer.Trainer(cfg2["net"](), cfg2["ds"], 128, **kw)
    spe = first.indices.steps_per_epoch()
    assert K % spe and (2 * K) // spe > K // spe and K < 12
    for _ in range(K):
        first.step()
    path = str(tmp_path / "optim.ckpt")
    runfiles.save_checkpoint(path, first)
    saved = torch.load(path, weights_only=True)["trainer"]["optim"]        # tensors and plain values only
    assert saved["max_grad_norm"] == cfg2["M"] and saved["skip_nonfinite"] is True
    assert saved["lr_schedule"].dtype == torch.float32 and saved["lr_schedule"].numel() == 26
    assert saved["last_lr"] == float(np.float32(kw["lr_schedule"][K - 1]))
    half = state(first)
    del first

    net2 = cfg2["net"]()
    with torch.no_grad():
        for p in net2.parameters():
            p.add_(1.0)
    second = trainer.Trainer(net2, cfg2["ds"], 128, **kw)
    runfiles.load_checkpoint(path, second)
    same(state(second), half)
    for _ in range(K):
        second.step()
    same(state(second), want)
    assert second.read_optim_stats()["clipped"] == straight.read_optim_stats()["clipped"]

    # other options than the checkpoint's are refused, by name
    other = trainer.Trainer(cfg2["net"](), cfg2["ds"], 128,
                            **dict(kw, lr_schedule=trainer.warmup_cosine(2e-3, 12, 26)))
    with pytest.raises(ValueError, match="lr_schedule"):
        runfiles.load_checkpoint(path, other)
    other = trainer.Trainer(cfg2["net"](), cfg2["ds"], 128, **dict(kw, max_grad_norm=2 * cfg2["M"]))
    with pytest.raises(ValueError, match="max_grad_norm"):
        runfiles.load_checkpoint(path, other)
    plain = trainer.Trainer(cfg2["net"](), cfg2["ds"], 128, mode=_lib.MODE_BF16, seed=1)
    with pytest.raises(ValueError, match="max_grad_norm|lr_schedule|skip_nonfinite"):
        runfiles.load_checkpoint(path, plain)
    # and a checkpoint without options still loads into a Trainer without them
    runfiles.save_checkpoint(path, plain)
    assert "optim" not in torch.load(path, weights_only=True)["trainer"]
    runfiles.load_checkpoint(path, plain)
    with pytest.raises(ValueError, match="max_grad_norm"):
        runfiles.load_checkpoint(path, second)


# ---- two ranks -----------------------------------------------------------------------------------------------
def test_two_ranks_clip_the_averaged_gradient(tmp_path):
    env = dict(os.environ, HSA_ENABLE_IPC_MODE_LEGACY="0")
    r = subprocess.run([sys.executable, "-m", "torch.distributed.run", "--nnodes=1",
                        "--nproc-per-node", "2", "--master-addr", "127.0.0.1",
                        "--master-port", str(_free_port()),
                        os.path.join(ROOT, "scripts", "optim_ddp_check.py")],
                       env=env, capture_output=True, text=True, timeout=600)
    print(r.stdout[-3000:])
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-3000:]
    for line in ("RANKS_IDENTICAL True", "LOCAL_NORMS_DIFFER True", "NORM_IS_OF_THE_AVERAGE True",
                 "NORM_IS_NOT_LOCAL True", "GRAPH_RANKS_IDENTICAL True"):
        assert line in r.stdout, (line, r.stdout)
    clipped = int(r.stdout.split("CLIPPED ")[1].split()[0])
    assert clipped >= 1


# ---- fit ---------------------------------------------------------------------------------------------------------
def test_fit_reports_the_optimiser_once_per_epoch(dev):
    from pca_hip import _lib, trainer
    from test_gpu_trainer_eval import _dense_2d, _net
    ds = _dense_2d(dev)
    table = trainer.warmup_cosine(1e-3, 5, 15)
    tr = trainer.Trainer(_net(dev, 2), ds, 32, mode=_lib.MODE_F32, seed=1, lr_schedule=table,
                         max_grad_norm=1.0, skip_nonfinite=True)
    spe = tr.indices.steps_per_epoch()
    assert spe == 10
    lines = []
    with HostReads() as reads:
        hist = tr.fit(2, log=lines.append)
    # what fit reads without the options (test_fit_logs_like_the_reference_and_resumes_bitwise), plus one
    per_epoch = 1 + (tr.eng._handoff_word is not None)
    assert reads.n == 2 * (per_epoch + 1), reads.n
    assert len(lines) == 4 and lines[1].startswith("Epoch 0: grad norm") and "lr" in lines[3]
    for e, h in enumerate(hist):
        assert h["grad_norm"] > 0 and math.isfinite(h["grad_norm"])
        assert h["lr"] == float(np.float32(table[min(spe * (e + 1), len(table)) - 1]))
        assert type(h["clipped_steps"]) is int and type(h["skipped_steps"]) is int
        assert 0 <= h["clipped_steps"] <= spe * (e + 1) and h["skipped_steps"] == 0
    assert hist[1]["clipped_steps"] >= hist[0]["clipped_steps"]
    # a Trainer without the options holds none of this and reads nothing more
    plain = trainer.Trainer(_net(dev, 2), ds, 32, mode=_lib.MODE_F32, seed=1)
    assert plain.optim_state is None and plain.lr_table is None and plain.norm_partials is None
    with HostReads() as reads:
        h = plain.fit(1, log=lines.append)
    assert reads.n == per_epoch and "grad_norm" not in h[0]
    with pytest.raises(_lib.PcaHipError):
        plain.read_optim_stats()
