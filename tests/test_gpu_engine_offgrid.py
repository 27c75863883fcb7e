"""Whole models in the exact fp32 mode (PCA_MODE_F32) at widths no fused kernel sees: d not in
{16, 32, 64, 128, 256}, d % 4 != 0, one class, one point, one inducing point, C and m off every tile size.
The engine accepts any d % h == 0 and so does modules.MAB; every other whole-model case of the suite sits on
the fused grid.

Per architecture: STEngine(training=False).forward and STEngine(training=True).fwd_bwd against
orc.st_forward + orc.cross_entropy differentiated on the CPU (as tests/test_gpu_varlen.py::_oracle_truncated
does), at the bars of tests/test_gpu_parity.py - logits 1e-4, loss 2e-4, every gradient 2e-4, relative to
max(1, max|ref|) - plus grad_bars.judge(F32) on every tensor's own scale; then the same model through the
nn.Module path (pca_linear_* + pca_cross_entropy instead of the engine's fused classifier head), which must
meet the same bars and agree with the engine: the two routes use different head kernels, so a disagreement
localises a failure.

The train step's classifier head (cls_fwd_bwd_body, csrc/pma_head_bodies.hpp) read its weight rows with
16-byte loads whatever the width; d6, d10 and d130 are the widths at which that was wrong.

test_oracle_alone_meets_the_bars needs no GPU: the bars must hold for the reference alone (the float32
oracle against the float64 one), or they say nothing about the kernels."""
import numpy as np
import pytest
import torch

import inputs as gi
import grad_bars as gb
from util import T, close

FWD_TOL = 1e-4        # tests/test_gpu_parity.py
LOSS_TOL = 2e-4
BWD_TOL = 2e-4

ARCHS = [  # name, din, d, h, m, C, B, N
    ("d6", 2, 6, 3, 3, 3, 3, 5),
    ("d10", 3, 10, 5, 1, 1, 1, 1),
    ("d12", 1, 12, 3, 5, 65, 5, 33),
    ("d20", 4, 20, 2, 2, 2, 2, 65),
    ("d36", 5, 36, 6, 7, 130, 4, 17),
    ("d100", 2, 100, 4, 7, 300, 3, 70),
    ("d130", 3, 130, 2, 3, 10, 2, 9),
    ("d192", 8, 192, 6, 33, 50, 2, 40),
]
BY_NAME = {a[0]: a for a in ARCHS}
# (arch, PMA seeds, variable-length sets): every dense architecture; d6 and d100 again on padded sets;
# d12 with three seeds (inference engine and module path only: the train step needs k = 1)
RUNS = [(a[0], 1, False) for a in ARCHS] + [("d6", 1, True), ("d100", 1, True), ("d12", 3, False)]
RUN_IDS = [f"{n}{'_k%d' % k if k != 1 else ''}{'_lengths' if v else ''}" for n, k, v in RUNS]
# torch.manual_seed before models.ST, per architecture (none had to be changed for the reference's sake:
# test_oracle_alone_meets_the_bars holds at the first seed tried for each)
SEED = {a[0]: 40 + i for i, a in enumerate(ARCHS)}

_cache = {}


def _lengths(B, N):
    return ([N, 1, N // 2 + 1] * B)[:B]


def _case(name, k, varlen):
    """Model (CPU), inputs, labels and lengths of one run; built once per session."""
    key = (name, k, varlen)
    if key not in _cache:
        import models
        _, din, d, h, m, C, B, N = BY_NAME[name]
        i = [a[0] for a in ARCHS].index(name)
        torch.manual_seed(SEED[name])
        net = models.ST(dim_input=din, num_outputs=k, dim_output=C, num_inds=m, dim_hidden=d, num_heads=h)
        X = gi.pc_input(7100 + i, B, N, din)
        X2 = gi.pc_input(7200 + i, B, N, din)
        lengths = _lengths(B, N) if varlen else [N] * B
        for b, L in enumerate(lengths):            # padding rows: zeros, as the pack kernel writes
            X[b, L:] = 0.0
            X2[b, L:] = 0.0
        y = gi.labels(7300 + i, B, C)
        _cache[key] = dict(net=net, X=X, X2=X2, y=y, lengths=lengths,
                           p={k_: v.detach().clone() for k_, v in net.state_dict().items()})
    return _cache[key]


def _oracle(p, X, y, lengths, h, k, dtype=torch.float32):
    """logits [B * k, C], mean CE loss and gradients from the oracle on X[b, :lengths[b]], set by set
    (tests/test_gpu_varlen.py::_oracle_truncated, for k seeds and a choice of precision)."""
    from oracle import st_oracle as orc
    params = {n: v.detach().to(dtype).clone().requires_grad_(True) for n, v in p.items()}
    C = params["dec.1.weight"].shape[0]
    lg = [orc.st_forward(torch.from_numpy(X[b:b + 1, :lengths[b]]).to(dtype), params, h).reshape(k, C)
          for b in range(X.shape[0])]
    lg = torch.cat(lg, 0)
    loss = orc.cross_entropy(lg, torch.from_numpy(np.repeat(y, k)))
    loss.backward()
    return lg.detach().numpy(), float(loss.detach()), {n: v.grad.numpy() for n, v in params.items()}


def _reference(name, k, varlen):
    c = _case(name, k, varlen)
    if "ref" not in c:
        c["ref"] = _oracle(c["p"], c["X"], c["y"], c["lengths"], BY_NAME[name][3], k)
    return c["ref"]


def _judge(got, ref_g, shapes, C, what):
    """Every gradient at BWD_TOL relative to max(1, max|ref|) and on its own scale (grad_bars.F32).  One
    class: the softmax over one logit is 1, so the loss is identically 0 and every gradient an exact zero -
    there is no scale to judge on, and the result must be zero bit for bit."""
    got = got if isinstance(got, dict) else gb.split(got, shapes)
    for n, _ in shapes:
        close(got[n], np.asarray(ref_g[n]).reshape(tuple(got[n].shape)), BWD_TOL, f"{what} {n}")
    if C == 1:
        for n, _ in shapes:
            assert float(np.abs(np.asarray(ref_g[n])).max()) == 0.0, n
            assert float(got[n].abs().max()) == 0.0, f"{what} {n}: not an exact zero"
        return
    gb.judge(got, ref_g, gb.F32, shapes, what)


@pytest.mark.parametrize("run", RUNS, ids=RUN_IDS)
def test_oracle_alone_meets_the_bars(run):
    """No GPU: the oracle is finite on every case, its float32 evaluation (the reference of the GPU tests)
    stays within the stated bars of its float64 evaluation, and two different inputs give logits 2e-3 apart
    (so a path within 1e-4 of the oracle passes the GPU tests' 1e-3 non-vacuity guard)."""
    name, k, varlen = run
    _, din, d, h, m, C, B, N = BY_NAME[name]
    c = _case(name, k, varlen)
    lg32, loss32, g32 = _reference(name, k, varlen)
    lg64, loss64, g64 = _oracle(c["p"], c["X"], c["y"], c["lengths"], h, k, torch.float64)
    assert np.all(np.isfinite(lg64)) and np.isfinite(loss64)
    assert all(np.all(np.isfinite(v)) for v in g64.values())
    close(lg32, lg64, FWD_TOL, "logits")
    assert abs(loss32 - loss64) < LOSS_TOL
    shapes = [(n, tuple(v.shape)) for n, v in c["net"].named_parameters()]
    _judge({n: torch.from_numpy(g32[n]) for n, _ in shapes}, g64, shapes, C, f"{RUN_IDS[RUNS.index(run)]} f32 vs f64")
    other, _, _ = _oracle(c["p"], c["X2"], c["y"], c["lengths"], h, k, torch.float64)
    assert np.abs(other - lg64).max() > 2e-3
    if C > 1:       # the GPU test counts correct predictions exactly: no row's two best logits may be close
        top = np.sort(lg64, 1)
        assert (top[:, -1] - top[:, -2]).min() > 4 * FWD_TOL * max(1.0, float(np.abs(lg64).max()))


@pytest.fixture(scope="module")
def dev():
    import pca_hip
    pca_hip.lib()
    pca_hip.set_mode("f32")
    return torch.device("cuda", 0)


@pytest.mark.gpu
@pytest.mark.parametrize("run", RUNS, ids=RUN_IDS)
def test_engine_and_modules_offgrid(dev, run):
    import pca_hip
    from pca_hip import _lib, trainer
    name, k, varlen = run
    _, din, d, h, m, C, B, N = BY_NAME[name]
    rid = RUN_IDS[RUNS.index(run)]
    c = _case(name, k, varlen)
    ref_lg, ref_loss, ref_g = _reference(name, k, varlen)
    net = c["net"].to(dev)
    shapes = gb.shapes_of(net)
    Xd, X2d = T(c["X"], dev), T(c["X2"], dev)
    yd = T(np.repeat(c["y"], k), dev)
    ld = torch.tensor(c["lengths"], dtype=torch.int32, device=dev) if varlen else None

    # ---- the engine: inference, then the train step ----
    inf = trainer.STEngine(net, B, N, _lib.MODE_F32, training=False)
    lg_inf = inf.forward(Xd, ld).clone()
    close(lg_inf, ref_lg, FWD_TOL, f"{rid} logits(inf)")
    other = inf.forward(X2d, ld).clone()
    assert float((other - lg_inf).abs().max()) > 1e-3, f"{rid}: the logits do not depend on the input"
    eng = None
    if k == 1:
        eng = trainer.STEngine(net, B, N, _lib.MODE_F32, training=True)
        eng.fwd_bwd(Xd, yd, lengths=ld)
        torch.cuda.synchronize()
        close(eng.logits, ref_lg, FWD_TOL, f"{rid} logits(train)")
        assert abs(float(eng.loss) - ref_loss) < LOSS_TOL, (rid, float(eng.loss), ref_loss)
        assert abs(float(eng.stats[0]) / B - ref_loss) < LOSS_TOL
        assert float(eng.stats[1]) == float((ref_lg.argmax(1) == c["y"]).sum())
        _judge(eng.grads, ref_g, shapes, C, f"{rid} engine vs oracle")

    # ---- the nn.Module path: pca_mab_*, pca_linear_*, pca_cross_entropy ----
    pca_hip.set_mode("f32")
    net.zero_grad(set_to_none=True)
    lg_mod = (net(Xd) if not varlen else net(Xd, torch.tensor(c["lengths"]))).reshape(B * k, C)
    close(lg_mod, ref_lg, FWD_TOL, f"{rid} logits(modules)")
    loss = pca_hip.cross_entropy(lg_mod, yd)
    assert abs(float(loss.detach()) - ref_loss) < LOSS_TOL, (rid, float(loss.detach()), ref_loss)
    loss.backward()
    g_mod = {n: (p.grad if p.grad is not None else torch.zeros_like(p)).detach().clone()
             for n, p in net.named_parameters()}
    _judge(g_mod, ref_g, shapes, C, f"{rid} modules vs oracle")
    with torch.no_grad():
        lg_ng = (net(Xd) if not varlen else net(Xd, torch.tensor(c["lengths"]))).reshape(B * k, C)
    close(lg_ng, ref_lg, FWD_TOL, f"{rid} logits(modules, no_grad)")

    # ---- the two routes agree ----
    close(lg_inf, lg_mod, FWD_TOL, f"{rid} engine(inf) vs modules logits")
    if eng is not None:
        close(eng.logits, lg_mod, FWD_TOL, f"{rid} engine vs modules logits")
        assert abs(float(eng.loss) - float(loss.detach())) < LOSS_TOL
        _judge(eng.grads, {n: v.cpu().numpy() for n, v in g_mod.items()}, shapes, C, f"{rid} engine vs modules")


@pytest.mark.gpu
def test_train_step_refuses_a_head_beyond_lds(dev):
    """The train step's classifier head keeps d + C floats of a set in LDS: the widest head that fits
    (d + C = 16368) runs and agrees with the oracle, one class more is refused before anything is enqueued."""
    import models
    from pca_hip import _lib, trainer
    din, d, h, m, B, N = 2, 6, 3, 1, 2, 3
    X = gi.pc_input(7400, B, N, din)
    for C, ok in ((16368 - d, True), (16368 - d + 1, False)):
        torch.manual_seed(60)
        net = models.ST(dim_input=din, num_outputs=1, dim_output=C, num_inds=m, dim_hidden=d, num_heads=h)
        p = {n: v.detach().clone() for n, v in net.state_dict().items()}
        y = gi.labels(7401, B, C)
        net = net.to(dev)
        eng = trainer.STEngine(net, B, N, _lib.MODE_F32, training=True)
        if not ok:
            with pytest.raises(_lib.PcaHipError, match="do not fit the classifier head's LDS"):
                eng.fwd_bwd(T(X, dev), T(y, dev))
            torch.cuda.synchronize()
            assert float(eng.grads.abs().max()) == 0.0 and float(eng.stats.abs().max()) == 0.0
            continue
        eng.fwd_bwd(T(X, dev), T(y, dev))
        ref_lg, ref_loss, ref_g = _oracle(p, X, y, [N] * B, h, 1)
        close(eng.logits, ref_lg, FWD_TOL, "logits")
        assert abs(float(eng.loss) - ref_loss) < LOSS_TOL
        _judge(eng.grads, ref_g, gb.shapes_of(net), C, "widest head vs oracle")
