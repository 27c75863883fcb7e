"""Soft targets on the device (between-class training: two labelled clips mixed, the loss on the mixed
label): pca_cross_entropy_soft and the four loss sites of the train step against the float64 restatement
(tests/soft_ce_ref.py), the hard step's bits at w = 1 / eps = 0, the whole step against the CPU oracle
with probability targets, the two extra outputs of the frame kernel, and the Trainer.

Every comparison asserts the path its arm took: the launch count of k_set128_fwd (tests/dispatch.py) and
the ``PCA_SET128`` / ``PCA_SET128_HEAD`` switches, as tests/test_gpu_set128.py does."""
import contextlib
import ctypes as C
import os

import numpy as np
import pytest
import torch

import abi_mab as am
import grad_bars as gb
import inputs as gi
import soft_ce_ref as ref
from dispatch import launches
from oracle import st_oracle as orc
from util import T, close, close_robust

pytestmark = pytest.mark.gpu

NAN = float("nan")
FS = 44100


@pytest.fixture(scope="module")
def dev():
    import pca_hip
    pca_hip.lib()
    return torch.device("cuda", 0)


def _bits(t):
    return t.view(torch.int32) if t.dtype == torch.float32 else t


def _targets(seed, B, Cc):
    """y1, y2, w: row 0 has w = 1, row 1 w = 0, row 2 y1 == y2 (rows that exist); every other row two
    different classes at a weight in [0.1, 0.9]."""
    rng = np.random.Generator(np.random.PCG64(seed))
    y1 = rng.integers(0, Cc, size=B)
    y2 = (y1 + 1 + rng.integers(0, Cc - 1, size=B)) % Cc
    assert (y1 != y2).all()
    w = rng.uniform(0.1, 0.9, size=B).astype(np.float32)
    w[0] = 1.0
    if B > 1:
        w[1] = 0.0
    if B > 2:
        y2[2] = y1[2]
    return y1.astype(np.int64), y2.astype(np.int64), w


# ---- 1. pca_cross_entropy_soft ----------------------------------------------------------------------------
@pytest.mark.parametrize("eps", [0.0, 0.1])
@pytest.mark.parametrize("B,Cc,big", [(1, 5, False), (5, 50, False), (7, 70, False), (6, 130, False),
                                      (5, 50, True)], ids=["B1", "C50", "C70", "C130", "pm3e4"])
def test_cross_entropy_soft_contract(dev, B, Cc, big, eps):
    from pca_hip import _lib
    L = _lib.lib()
    g = torch.Generator().manual_seed(B * Cc + 1)
    logits = torch.randn(B, Cc, generator=g) * 3
    if big:
        logits = torch.where(torch.rand(B, Cc, generator=g) < 0.5, -3e4, 3e4) + torch.randn(B, Cc, generator=g)
    y1, y2, w = _targets(B + Cc, B, Cc)
    y1[0] = Cc - 1
    x64 = logits.double().numpy()
    ar = am.Arena(dev)
    ld = logits.to(dev)
    y1d, y2d, wd = T(y1, dev), T(y2, dev), T(w, dev)
    for gs in (1.0, 0.37):
        want = ref.soft_ce(x64, y1, y2, w.astype(np.float64), eps, gs)
        per = want["per"]
        loss = ar.tensor((1,), torch.float32, NAN)
        dlog = ar.tensor((B, Cc), torch.float32, NAN)
        stats = ar.tensor((2,), torch.float32, torch.tensor([3.25, 2.0]))
        soft = _lib.PcaSoftTargets(y2d.data_ptr(), wd.data_ptr(), eps)
        rc = L.pca_cross_entropy_soft(ld.data_ptr(), y1d.data_ptr(), C.byref(soft), B, Cc, gs, loss.data_ptr(),
                                      dlog.data_ptr(), stats.data_ptr(), None)
        assert rc == 0, L.pca_last_error()
        torch.cuda.synchronize()
        lv = float(loss.cpu())
        print(f"B={B} C={Cc} eps={eps} gs={gs}: loss {lv!r} want {want['loss']!r}, max|per| {np.abs(per).max():.3g}")
        assert np.isfinite(lv) and abs(lv - want["loss"]) <= 1e-6 * max(1.0, float(np.abs(per).max())), \
            (lv, want["loss"])
        gb.own_close(dlog, want["dlogits"], gb.F32, f"dlogits (grad_scale {gs})")
        st = stats.cpu().double()
        assert abs(float(st[0]) - (3.25 + float(per.sum()))) <= 1e-6 * (3.25 + float(np.abs(per).sum())), (st, per)
        assert float(st[1]) == 2.0 + want["correct"], (st, want["correct"])
    assert ar.check() == []


def test_cross_entropy_autograd_soft_and_hard(dev):
    """pca_hip.cross_entropy: the five-argument call against the restatement, its backward, and w = 1 /
    eps = 0 (whatever labels2 holds) against the two-argument call, bit for bit."""
    import pca_hip
    B, Cc = 7, 50
    y1, y2, w = _targets(3, B, Cc)
    x = torch.randn(B, Cc, generator=torch.Generator().manual_seed(4)) * 3
    xd = x.to(dev).requires_grad_(True)
    loss = pca_hip.cross_entropy(xd, T(y1, dev), T(y2, dev), T(w, dev), label_smoothing=0.1)
    (loss * 0.5).backward()
    want = ref.soft_ce(x.double().numpy(), y1, y2, w.astype(np.float64), 0.1, 0.5)
    assert abs(float(loss.detach()) - want["loss"]) <= 1e-6 * max(1.0, float(np.abs(want["per"]).max()))
    gb.own_close(xd.grad, want["dlogits"], gb.F32, "autograd dlogits")
    hard = pca_hip.cross_entropy(x.to(dev).requires_grad_(True), T(y1, dev))
    for kw in (dict(labels2=T(y2, dev), weight=torch.ones(B, device=dev)), dict(labels2=T(y2, dev)),
               dict(weight=torch.ones(B, device=dev))):
        xs = x.to(dev).requires_grad_(True)
        soft = pca_hip.cross_entropy(xs, T(y1, dev), **kw)
        soft.backward()
        # (the mean is a float atomic over the samples: its order is not fixed, the gradient's is)
        assert abs(float(soft.detach()) - float(hard.detach())) <= 1e-6 * abs(float(hard.detach()))
        xh = x.to(dev).requires_grad_(True)
        pca_hip.cross_entropy(xh, T(y1, dev)).backward()
        assert torch.equal(_bits(xs.grad), _bits(xh.grad))


# ---- the engine at a loss site ------------------------------------------------------------------------------
# name: (mode, d, h, m, N, din, B, C, PCA_SET128_HEAD, k_set128_fwd launches per step)
SITES = {
    "tail-C50": ("bf16", 128, 4, 16, 256, 2, 5, 50, "1", 1),            # head_stages of k_set128_fwd
    "tail-C64": ("bf16", 128, 4, 16, 256, 2, 5, 64, "1", 1),
    "head1": ("bf16", 128, 4, 16, 256, 2, 5, 50, "0", 1),               # k_pma_head1, a launch of its own
    "head-generic": ("bf16", 128, 4, 16, 256, 2, 5, 70, "1", 1),        # C > 64: k_pma_head (cls_fwd_bwd_body)
    "cls-f32-d32": ("f32", 32, 4, 4, 33, 3, 3, 7, "1", 0),              # cls_train_head
    "cls-f32-d128": ("f32", 128, 4, 16, 64, 2, 3, 10, "1", 0),
    "cls-bf16-d64": ("bf16", 64, 8, 64, 65, 2, 3, 10, "1", 0),
}


@contextlib.contextmanager
def _switches(head):
    old = {k: os.environ.get(k) for k in ("PCA_SET128", "PCA_SET128_HEAD")}
    os.environ["PCA_SET128"] = "1"
    os.environ["PCA_SET128_HEAD"] = head
    try:
        yield
    finally:
        for k, v in old.items():
            if v is None:
                del os.environ[k]
            else:
                os.environ[k] = v


def _site(dev, name, seed=0):
    import models
    from pca_hip import _lib
    mode, d, h, m, N, din, B, Cc, head, n_set = SITES[name]
    torch.manual_seed(300 + d + Cc + seed)
    net = models.ST(dim_input=din, num_outputs=1, dim_output=Cc, num_inds=m, dim_hidden=d, num_heads=h).to(dev)
    Xn = gi.pc_input(7300 + N + seed, B, N, din)
    return net, Xn, (_lib.MODE_BF16 if mode == "bf16" else _lib.MODE_F32), (h, N, B, Cc, head, n_set)


def _step(dev, net, Xn, mode, shape, y1, witness=True, **soft):
    """One eager fwd_bwd on a fresh engine -> (logits, loss, grads); asserts the path."""
    from pca_hip import trainer
    h, N, B, Cc, head, n_set = shape
    kw = {k: (T(v, dev) if isinstance(v, np.ndarray) else v) for k, v in soft.items()}
    with _switches(head):
        eng = trainer.STEngine(net, B, N, mode, training=True)
        X, y = T(Xn, dev), T(y1, dev)
        eng.fwd_bwd(X, y, phase=-1, **kw)
        torch.cuda.synchronize()
        eng.check_handoffs()
        out = eng.logits.clone(), float(eng.loss), eng.grads.clone()
        if witness:
            n = launches(lambda: eng.fwd_bwd(X, y, phase=-1, **kw), ("set_fwd",))["set_fwd"]
            eng.check_handoffs()
            assert n == n_set, f"k_set128_fwd launched {n} times per step, expected {n_set}"
    return out


# ---- 2. each loss site on the engine's own logits ---------------------------------------------------------
@pytest.mark.parametrize("eps", [0.0, 0.1])
@pytest.mark.parametrize("name", list(SITES))
def test_loss_site_on_its_own_logits(dev, name, eps):
    net, Xn, mode, shape = _site(dev, name)
    h, N, B, Cc, head, n_set = shape
    y1, y2, w = _targets(11 + Cc, B, Cc)
    lg, loss, g = _step(dev, net, Xn, mode, shape, y1, labels2=y2, weight=w, label_smoothing=eps)
    assert torch.isfinite(lg).all() and torch.isfinite(g).all()
    want = ref.soft_ce(lg.double().cpu().numpy(), y1, y2, w.astype(np.float64), eps)
    per = want["per"]
    print(f"{name} eps={eps}: loss {loss!r} want {want['loss']!r}, max|per| {np.abs(per).max():.3g}")
    assert abs(loss - want["loss"]) <= 1e-6 * max(1.0, float(np.abs(per).max())), (loss, want["loss"])
    # dec.1.bias' gradient is the plain fp32 sum of the B dlogits rows
    dbc = gb.split(g, gb.shapes_of(net))["dec.1.bias"]
    gb.own_close(dbc, want["dlogits"].sum(axis=0), gb.F32, f"{name}: dec.1.bias gradient")


# ---- 3. hard == soft at w = 1, eps = 0, bitwise --------------------------------------------------------------
def _same_gradients(net, g1, g0, what, exact):
    """The whole gradient vector bit for bit - or, where the hard step itself is not reproducible from one
    run to the next, the tensors the loss stage writes bit for bit and all 45 under grad_bars.F32, the bar of
    two fp32 paths that differ in reduction order only."""
    if exact:
        assert torch.equal(_bits(g1), _bits(g0)), f"{what}: {int((_bits(g1) != _bits(g0)).sum())} gradients differ"
        return
    a, b = gb.split(g1, gb.shapes_of(net)), gb.split(g0, gb.shapes_of(net))
    for k in ("dec.1.weight", "dec.1.bias"):
        assert torch.equal(_bits(a[k]), _bits(b[k])), f"{what}: {k} differs"
    gb.judge(g1, g0, gb.F32, gb.shapes_of(net), what, quiet=True)


@pytest.mark.parametrize("name", ["tail-C50", "head1", "cls-f32-d32", "cls-f32-d128"])
def test_hard_equals_soft_at_weight_one_bitwise(dev, name):
    """Logits, loss and gradients of the soft step at w = 1, eps = 0 are the hard step's bits.  The bf16
    step is bit-reproducible (no float atomics), so there the whole gradient vector is compared.  The fp32
    chain sums its bias gradients over workgroups with float atomics (k_colsum): two HARD steps on the same
    inputs already differ - measured on an MI355X at the d = 32 shape, three repeats against a first run:
    24, 34 and 24 elements, all in bias gradients of enc.0 / enc.1 (fc_k, fc_q, fc_o), logits and loss equal;
    none at the d = 128 fp32 shape in three repeats, which the code does not guarantee.  So at the fp32
    shapes the bits are asserted for logits, loss and the gradients the loss stage itself produces
    (dec.1.weight, dec.1.bias: a fixed-order sum), and the whole vector is held to grad_bars.F32, the bar of
    two fp32 paths that differ in reduction order only - the judgement a second hard run gets, too."""
    net, Xn, mode, shape = _site(dev, name, seed=1)
    exact = not name.startswith("cls-f32")
    h, N, B, Cc, head, n_set = shape
    y1, y2, _ = _targets(21 + Cc, B, Cc)
    y2[2] = (y1[2] + 1) % Cc
    assert (y1 != y2).all()
    ones = np.ones(B, dtype=np.float32)
    lg0, loss0, g0 = _step(dev, net, Xn, mode, shape, y1)
    assert float(g0.abs().max()) > 0
    if not exact:                       # the control: hard against hard
        lg, loss, g = _step(dev, net, Xn, mode, shape, y1, witness=False)
        assert torch.equal(_bits(lg), _bits(lg0)) and loss == loss0
        _same_gradients(net, g, g0, "hard again", exact)
        print(f"{name}: two hard steps differ in {int((_bits(g) != _bits(g0)).sum())} of {g.numel()} gradients")
    for what, kw in (("labels2 + weight", dict(labels2=y2, weight=ones)),
                     ("weight None", dict(labels2=y2)), ("labels2 None", dict(weight=ones))):
        lg1, loss1, g1 = _step(dev, net, Xn, mode, shape, y1, witness=False, **kw)
        assert torch.equal(_bits(lg1), _bits(lg0)), what
        assert np.float32(loss1).tobytes() == np.float32(loss0).tobytes(), (what, loss1, loss0)
        _same_gradients(net, g1, g0, what, exact)
    # ... and the second label does reach the loss: at w = 0.5 the step differs
    _, loss2, g2 = _step(dev, net, Xn, mode, shape, y1, witness=False, labels2=y2, weight=0.5 * ones)
    assert loss2 != loss0 and not torch.equal(g2, g0)


# ---- 4. the whole step against the oracle -------------------------------------------------------------------
def _oracle(Xn, p, h, t):
    leaves = {k: v.detach().clone().requires_grad_(True) for k, v in p.items()}
    logits = orc.st_forward(torch.from_numpy(Xn), leaves, h)
    if logits.dim() == 1:
        logits = logits.unsqueeze(0)
    loss = torch.nn.functional.cross_entropy(logits, torch.from_numpy(t).to(logits.dtype))
    loss.backward()
    return float(loss.detach()), logits.detach(), {k: v.grad for k, v in leaves.items()}


@pytest.mark.parametrize("kind", ["bf16-set-resident", "f32-d32"])
def test_soft_step_vs_oracle(dev, kind):
    import models
    from pca_hip import _lib
    eps = 0.1
    if kind == "bf16-set-resident":
        d, h, m, N, din, B, Cc, mode, n_set = 128, 4, 16, 256, 2, 6, 50, _lib.MODE_BF16, 1
    else:
        d, h, m, N, din, B, Cc, mode, n_set = 32, 4, 4, 33, 3, 3, 7, _lib.MODE_F32, 0
    torch.manual_seed(200 + N)
    net = models.ST(dim_input=din, num_outputs=1, dim_output=Cc, num_inds=m, dim_hidden=d, num_heads=h).to(dev)
    p = {k: v.detach().cpu().clone() for k, v in net.state_dict().items()}
    Xn = gi.pc_input(7100 + N, B, N, din)
    y1, y2, w = _targets(31 + Cc, B, Cc)
    t = ref.targets(y1, y2, w.astype(np.float64), eps, Cc)
    ref_loss, ref_lg, ref_g = _oracle(Xn, p, h, t)
    lg, loss, g = _step(dev, net, Xn, mode, (h, N, B, Cc, "1", n_set), y1, labels2=y2, weight=w,
                        label_smoothing=eps)
    # logits and loss: the bounds of test_set128_train_step_vs_oracle
    close(lg, ref_lg.reshape(B, Cc), 3e-2, "logits")
    assert abs(loss - ref_loss) < 3e-2 * max(1.0, abs(ref_loss)), (loss, ref_loss)
    if mode == _lib.MODE_BF16:
        off = 0
        for k, prm in net.named_parameters():
            close_robust(g[off:off + prm.numel()].view_as(prm), ref_g[k], 5e-2, k, outlier_frac=5e-3)
            off += prm.numel()
        gb.judge(g, ref_g, gb.BF16_VS_ORACLE, gb.shapes_of(net), f"{kind} soft step vs oracle")
    else:
        gb.judge(g, ref_g, gb.F32, gb.shapes_of(net), f"{kind} soft step vs oracle")


# ---- 5. the frame kernel's targets --------------------------------------------------------------------------
@pytest.fixture(scope="module")
def corpus():
    secs = (0.05, 0.11, 0.2, 0.3667, 0.5)
    clips = [orc.synth_clip(40 + i, 3 * i + 1, seconds=s) for i, s in enumerate(secs)]
    rng = np.random.Generator(np.random.PCG64(8))
    bgs = [orc.synth_clip(60, 2, seconds=0.03), (0.3 * rng.standard_normal(100)).astype(np.float32),
           np.zeros(500, dtype=np.float32), orc.synth_clip(61, 8, seconds=0.08)]     # bgs[2] is silent
    return clips, np.array([4, 9, 2, 7, 5]), bgs, np.array([11, 12, 13, 14])


def _wave_ds(corpus, dev, ntemp, seed, **kw):
    import dataset
    clips, y, bgs, bg_y = corpus
    opts = dict(device=dev, mix_clips=bgs, mix_prob=0.5, mix_snr_db=(-20.0, 20.0), seed=seed)
    opts.update(kw)
    if ntemp == 1:
        return dataset.ESC_wave_pc(clips, y, FS, 256, **opts)
    return dataset.ESC_wave_pc_temp(clips, y, FS, 256, ntemp, **opts)


def _check_targets(ds, bg_y, lab, meta, lab2, wgt, min_each=8, silent=None):
    """labels2 / weight of a batch against what its meta reports; returns the mask of the mixing slots."""
    rms, _, _, brms, _ = ds._mix_resident()
    rms, brms = rms.cpu().numpy(), brms.cpu().numpy()
    meta = meta.cpu().numpy()
    lab, lab2, wgt = lab.cpu().numpy(), lab2.cpu().numpy(), wgt.cpu().numpy()
    assert lab2.dtype == np.int64 and wgt.dtype == np.float32
    alpha = meta[:, 7].copy().view(np.float32).astype(np.float64)
    c, c2 = meta[:, 0], meta[:, 5]
    mixes = (c2 >= 0) & (alpha != 0.0)
    assert mixes.sum() >= min_each and (~mixes).sum() >= min_each, (mixes.sum(), (~mixes).sum())
    if silent is not None:
        assert (c2 == silent).any(), "the silent background clip was never drawn: pick another seed"
        assert not mixes[c2 == silent].any()
    assert np.array_equal(lab2[mixes], np.asarray(bg_y)[c2[mixes]])
    want = 1.0 / (1.0 + alpha[mixes] * brms[c2[mixes]] / rms[c[mixes]])
    err = float(np.abs(wgt[mixes].astype(np.float64) - want).max())
    print(f"weights of {mixes.sum()} mixing slots in [{wgt[mixes].min():.3f}, {wgt[mixes].max():.3f}], "
          f"max error {err:.2e}")
    assert err <= 1e-6                      # alpha and w are one fp32 rounding each
    assert (wgt[mixes] > 0.08).all() and (wgt[mixes] < 0.92).all()          # SNR in (-20, 20) dB
    assert np.array_equal(lab2[~mixes], lab[~mixes]) and (wgt[~mixes] == 1.0).all()
    return mixes


@pytest.mark.parametrize("ntemp", [1, 3])
def test_frame_kernel_targets(dev, corpus, ntemp):
    bg_y = corpus[3]
    seed = 12
    ds = _wave_ds(corpus, dev, ntemp, seed, mix_targets=True, mix_labels=bg_y)
    plain = _wave_ds(corpus, dev, ntemp, seed)
    assert ds.soft_targets and not plain.soft_targets
    rng = np.random.Generator(np.random.PCG64(5))
    idx = torch.from_numpy(rng.integers(0, len(ds), size=64)).to(dev)
    pts, lab, meta, smp, lab2, wgt = ds.batch(idx, want_meta=True, want_samples=True)
    pts0, lab0, meta0, smp0 = plain.batch(idx, want_meta=True, want_samples=True)   # pca_frame_points_ex
    assert torch.equal(_bits(pts), _bits(pts0)) and torch.equal(lab, lab0)
    assert torch.equal(meta, meta0) and torch.equal(_bits(smp), _bits(smp0))
    _check_targets(ds, bg_y, lab, meta, lab2, wgt, silent=2)
    # the same call twice: the same bits, into buffers the caller owns
    ds._draw = 0
    l2 = torch.full((64,), -1, dtype=torch.int64, device=dev)
    wt = torch.full((64,), NAN, dtype=torch.float32, device=dev)
    again = ds.batch(idx, want_meta=True, want_samples=True, labels2_out=l2, weight_out=wt)
    assert again[4] is l2 and again[5] is wt
    for a, b in zip(again, (pts, lab, meta, smp, lab2, wgt)):
        assert torch.equal(_bits(a), _bits(b))


# ---- 6. the Trainer -----------------------------------------------------------------------------------------
LENGTHS, LABELS = [3000, 5200, 4100, 6000], [1, 8, 3, 6]              # 12 + 21 + 17 + 24 = 74 sets of N = 256


def _train_ds(dev, **opts):
    import dataset
    clips = [orc.synth_clip(90 + i, 2 * i, seconds=n / FS)[:n] for i, n in enumerate(LENGTHS)]
    kw = dict(mix_clips="self", mix_prob=0.5, mix_snr_db=(-20.0, 20.0), mix_targets=True)
    kw.update(opts)
    d = dataset.ESC_wave_pc(clips, LABELS, FS, 512, seed=9, drop_nyquist=True, device=dev, **kw)
    assert len(d) == 74 and d.num_points == 256
    return d


def _net(dev, seed=4):
    import models
    torch.manual_seed(seed)
    return models.ST(dim_input=2, dim_output=10, num_inds=16, dim_hidden=128, num_heads=4).to(dev)


def _trainer(dev, graph, ds, ls=0.1):
    from pca_hip import _lib, trainer
    return trainer.Trainer(_net(dev), ds, batch_size=4, mode=_lib.MODE_BF16, use_graph=graph, seed=5,
                           label_smoothing=ls)


def _state(tr):
    torch.cuda.synchronize()
    return (tr.eng.flat.clone(), tr.m.clone(), tr.v.clone(), tr.step_count.clone())


def _same(a, b, what):
    for x, y, name in zip(a, b, ("parameters", "m", "v", "step_count")):
        assert torch.equal(_bits(x), _bits(y)), f"{what}: {name} not bitwise equal"


def test_trainer_graph_equals_eager_on_soft_targets(dev):
    """Three steps replayed from the captured graph against three steps enqueued eagerly.  A captured step
    freezes the host draw number of its recorded ``batch`` call (2: one warm-up, one recording) and advances
    on the device; the eager run is handed the same numbers (``_draw`` = 1 before every step)."""
    g = _trainer(dev, True, _train_ds(dev))
    assert g.labels2 is not None and g.weight is not None
    for _ in range(3):
        g.step()
    want = _state(g)
    assert torch.isfinite(want[0]).all() and int(want[3][0]) == 3
    e = _trainer(dev, False, _train_ds(dev))
    seen = []
    for _ in range(3):
        e.ds._draw = 1
        e.step()
        torch.cuda.synchronize()
        seen.append(e.weight.clone())
    _same(_state(e), want, "graph vs eager")
    assert not torch.equal(seen[0], seen[1]) or not torch.equal(seen[1], seen[2])     # drawn afresh per step
    assert torch.equal(_bits(e.weight), _bits(g.weight)) and torch.equal(e.labels2, g.labels2)
    loss_sum, correct = g.read_stats()
    assert np.isfinite(loss_sum) and 0 <= correct <= 12
    # the soft step is the set-resident launch, and no launch more than the hard step
    n = launches(lambda: e.eng.fwd_bwd(e.X, e.labels, labels2=e.labels2, weight=e.weight, label_smoothing=0.1),
                 ("set_fwd",))["set_fwd"]
    assert n == 1


@pytest.mark.parametrize("graph", [True, False], ids=["hipgraph", "eager"])
def test_trainer_resume_on_soft_targets(dev, tmp_path, graph):
    import runfiles
    straight = _trainer(dev, graph, _train_ds(dev))
    for _ in range(3):
        straight.step()
    want = _state(straight)
    first = _trainer(dev, graph, _train_ds(dev))
    first.step()
    path = str(tmp_path / "soft.ckpt")
    runfiles.save_checkpoint(path, first)
    state = torch.load(path, weights_only=True)["trainer"]
    assert not any("labels2" in k or "weight" == k for k in state)          # no new state
    second = _trainer(dev, graph, _train_ds(dev))
    with torch.no_grad():
        second.eng.flat.add_(1.0)
    runfiles.load_checkpoint(path, second)
    for _ in range(2):
        second.step()
    _same(_state(second), want, "resumed vs straight")


@pytest.mark.parametrize("graph", [True, False], ids=["hipgraph", "eager"])
def test_trainer_without_mix_is_the_hard_trainer_bitwise(dev, graph):
    """mix_prob = 0 with mix_targets: every slot carries its own label twice at weight 1, the step runs the
    soft entry - and lands on the bits of the Trainer on the dataset without mix_targets."""
    soft = _trainer(dev, graph, _train_ds(dev, mix_prob=0.0), ls=0.0)
    hard = _trainer(dev, graph, _train_ds(dev, mix_prob=0.0, mix_targets=False), ls=0.0)
    assert soft.labels2 is not None and hard.labels2 is None and soft._soft_kw() and not hard._soft_kw()
    for _ in range(3):
        soft.step()
        hard.step()
    _same(_state(soft), _state(hard), "mix_targets at mix_prob 0 vs without")
    assert torch.equal(soft.labels2, soft.labels) and (soft.weight == 1.0).all()
    assert soft.read_stats() == hard.read_stats()


def test_trainer_buffers_match_meta_and_fit_runs(dev):
    ds = _train_ds(dev)
    tr = _trainer(dev, False, ds)
    tr.step()
    tr.step()
    torch.cuda.synchronize()
    # the second step's batch again, from a dataset of its own: host draw 2, device count 1
    twin = _train_ds(dev)
    twin._draw = 1
    count = torch.tensor([1, 0], dtype=torch.int32, device=dev)
    pts, lab, meta, lab2, wgt = twin.batch(tr.idx, draw_dev=count, want_meta=True)
    assert torch.equal(_bits(pts), _bits(tr.X)) and torch.equal(lab, tr.labels)
    assert torch.equal(lab2, tr.labels2) and torch.equal(_bits(wgt), _bits(tr.weight))
    # B = 4: too few slots for the counts of test 5; a larger batch of the same dataset for those
    idx = torch.arange(64, device=dev)
    pts, lab, meta, lab2, wgt = twin.batch(idx, want_meta=True)
    _check_targets(twin, LABELS, lab, meta, lab2, wgt)
    # fit with a plain() held-out set: the Evaluator sees hard labels and no mix
    held = ds.plain()
    assert not held.soft_targets and not held.stochastic
    hist = tr.fit(1, test_dataset=held, eval_every=1, log=lambda s: None)
    assert len(hist) == 1 and np.isfinite(hist[0]["train_loss"]) and np.isfinite(hist[0]["test_loss"])
    assert 0.0 <= hist[0]["train_acc"] <= 1.0 and 0.0 <= hist[0]["test_acc"] <= 1.0
