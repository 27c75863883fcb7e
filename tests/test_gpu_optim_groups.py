"""pca_adam_step_groups on the device (csrc/optim.hip): AdamW, per-segment scales and the averaged
copy against tests/optim_groups_ref.py, stock torch and pca_adam_step_ex, and the Trainer options built
on it (decoupled_weight_decay, param_groups, average_decay, eval_weights, Evaluator.use_params): against a stock loop, graph
against eager, exact resume, evaluation on the averaged weights.  Run with ``-m gpu``.

Hyper-parameters of the kernel tests: lr = 1e-2, weight_decay = 0.1 (optim_groups_ref.LR / WD).  With
them, after the five steps, stock torch has coupled and decoupled 5e-2 apart at max|p| = 4.1, the EMA 2.9e-2
from p, and the four segments 0 / 6.5e-3 / 1.9e-2 / 2.5e-2 from the ungrouped run
(tests/test_optim_groups_host.py asserts it): every switch shows four orders above ADAM_TOL."""
import ctypes as C
import math

import numpy as np
import pytest
import torch

import inputs as gi
import grad_bars as gb
import optim_groups_ref as ogr
from test_gpu_clip import HostReads
from test_gpu_optim import MOMENT_BAR, cfg2  # noqa: F401  (cfg2: the fixture, on this module's ``dev``)
from util import T, close

pytestmark = pytest.mark.gpu

ADAM_TOL = 1e-6          # the bar test_cross_entropy_and_adam holds pca_adam_step to


@pytest.fixture(scope="module")
def dev():
    import pca_hip
    pca_hip.lib()
    pca_hip.set_mode("f32")
    return torch.device("cuda", 0)


def _bits(t):
    return t.view(torch.int32) if t.dtype == torch.float32 else t


class GDev:
    """p, g, m, v, avg, the step words and the state words of one flat vector on the device, every
    vector ``offset`` floats behind a 16-byte boundary, and the two entry points on them."""

    def __init__(self, p, dev, seg_end=None, lr_scale=None, wd_scale=None, decoupled=False, avg_decay=None,
                 avg_start=1, max_norm=None, skip_nonfinite=False, table=None, offset=0, zero_grad=0,
                 lr=ogr.LR, wd=ogr.WD):
        from pca_hip import _lib
        self.n = n = p.numel()

        def vec(src=None):
            base = torch.zeros(n + 4 + offset, device=dev)
            assert base.data_ptr() % 16 == 0
            view = base[offset:offset + n]
            if src is not None:
                view.copy_(src)
            return view

        self.p, self.g, self.m, self.v = vec(p), vec(), vec(), vec()
        self.avg = vec() if avg_decay is not None else None
        if self.avg is not None:
            self.avg.fill_(-7.0)                      # the first applied step must overwrite it
        self.step = torch.zeros(2, dtype=torch.int32, device=dev)
        self.state = torch.zeros(8, dtype=torch.int32, device=dev)
        L = _lib.lib()
        self.part = torch.zeros(int(L.pca_grad_sumsq_partials(n)), dtype=torch.float64, device=dev)
        self.table = None if table is None else \
            torch.tensor(table, dtype=torch.float64).to(torch.float32).to(dev)
        self.need_norm = max_norm is not None or skip_nonfinite
        self.cfg = _lib.OptimCfg(lr, 0.9, 0.999, 1e-8, wd, 1.0, max_norm or 0.0, int(skip_nonfinite))
        self.zero_grad = zero_grad
        ends = list(seg_end or [])
        self.ends_host = (C.c_int64 * max(len(ends), 1))(*ends)
        self.ends = torch.tensor(ends, dtype=torch.int64, device=dev) if ends else None
        f32v = lambda x: None if x is None else torch.tensor(x, dtype=torch.float32, device=dev)
        self.ls, self.ws = f32v(lr_scale), f32v(wd_scale)
        ptr = lambda t: None if t is None else t.data_ptr()
        self.gr = _lib.OptimGroups(int(decoupled), len(ends), ptr(self.ends), ptr(self.ls), ptr(self.ws),
                                   None if self.avg is None else self.at(self.avg), 1.0 if avg_decay is None else 1.0 - avg_decay, avg_start)

    @staticmethod
    def at(view):
        """The address of a vector: its place in its allocation, also when it is empty."""
        return view._base.data_ptr() + 4 * view.storage_offset()

    def enqueue(self, grad, entry="groups"):
        """[pca_grad_sumsq ->] one optimiser launch on the current stream; no host sync."""
        from pca_hip import _lib
        L = _lib.lib()
        st = C.c_void_p(torch.cuda.current_stream().cuda_stream)
        self.g.copy_(grad)
        part, npart = (self.part.data_ptr(), self.part.numel()) if self.need_norm else (None, 0)
        if self.need_norm:
            _lib.check(L.pca_grad_sumsq(self.at(self.g), self.n, part, npart, st), "pca_grad_sumsq")
        tab = self.table
        args = (self.at(self.p), self.at(self.g), self.at(self.m), self.at(self.v), self.n,
                C.byref(self.cfg), part, npart, None if tab is None else tab.data_ptr(),
                0 if tab is None else tab.numel(), self.step.data_ptr(), self.state.data_ptr(),
                self.zero_grad)
        if entry == "ex":
            _lib.check(L.pca_adam_step_ex(*args, st), "pca_adam_step_ex")
        else:
            _lib.check(L.pca_adam_step_groups(*args, C.byref(self.gr), self.ends_host, st),
                       "pca_adam_step_groups")

    def run(self, grads, entry="groups"):
        for g in grads:
            self.enqueue(g, entry)
        torch.cuda.synchronize()
        return self

    def fields(self):
        h = self.state.cpu()
        return dict(skipped=int(h[0]), clipped=int(h[1]), last_norm=float(h.view(torch.float32)[2]),
                    norm_count=int(h[6]))

    def tensors(self):
        out = dict(p=self.p, m=self.m, v=self.v, step=self.step, state=self.state)
        if self.avg is not None:
            out["avg"] = self.avg
        return out


def _same_bits(a, b, names, what):
    ta, tb = a.tensors(), b.tensors()
    for k in names:
        assert torch.equal(_bits(ta[k]), _bits(tb[k])), f"{what}: {k} differs"


@pytest.fixture(scope="module")
def data(dev):
    n, p, grads = ogr.adam_inputs()
    return dict(n=n, p=p, grads=grads, on_dev={k: [g.to(dev) for g in ogr.case_grads(k, grads)]
                                               for k in ("clip", "skip")})


@pytest.fixture(scope="module")
def refs(data):
    """The restatement and stock torch over the five steps of every case: computed once, read only."""
    out = {}
    for name, kw in ogr.CASES.items():
        ref, truth = ogr.GroupsRef(data["p"], **kw), ogr.StockTruth(data["p"], **kw)
        for g in ogr.case_grads(name, data["grads"]):
            ref.step(g)
            truth.step(g)
        out[name] = (ref, truth)
    return out


def _case_grads(data, name):
    return data["on_dev"]["skip" if name == "skip" else "clip"]


def _against_refs(d, ref, truth, what):
    for k in ("p", "m", "v") + (("avg",) if d.avg is not None else ()):
        e1 = close(getattr(d, k), getattr(ref, k), ADAM_TOL, f"{what} {k} (restatement)")
        e2 = close(getattr(d, k), getattr(truth, k), ADAM_TOL, f"{what} {k} (stock torch)")
        print(f"{what} {k}: max|d| {e1:.2e} restatement, {e2:.2e} stock torch")


# ---- 1. the two rounding contracts ------------------------------------------------------------------------
GUARDS = {"plain": dict(), "guarded": dict(max_norm=50.0, skip_nonfinite=True,
                                           table=[2e-3, 6e-3, 1e-2, 5e-3])}


@pytest.mark.parametrize("guards", sorted(GUARDS))
@pytest.mark.parametrize("avg", [False, True], ids=["no_option", "avg_only"])
def test_rounding_contracts_bitwise_against_adam_step_ex(dev, data, avg, guards):
    kw = GUARDS[guards]
    grads = data["on_dev"]["clip"]
    ex = GDev(data["p"], dev, **kw).run(grads, "ex")
    gr = GDev(data["p"], dev, avg_decay=0.9 if avg else None, avg_start=2, **kw).run(grads)
    _same_bits(gr, ex, ("p", "m", "v", "step", "state"), f"{guards}, avg={avg}")
    assert ex.step.tolist() == [5, 0]
    assert ex.fields()["clipped"] == (4 if guards == "guarded" else 0)
    if avg:
        assert float((gr.avg - gr.p).abs().max()) > 1e-3 and torch.isfinite(gr.avg).all()


# ---- 2. / 3. decoupled or coupled, grouped, averaged, clipped -----------------------------------------------
@pytest.mark.parametrize("name", ["decoupled_grouped_averaged_clipped", "coupled_grouped"])
def test_groups_average_and_clip_against_restatement_and_stock_torch(dev, data, refs, name):
    ref, truth = refs[name]
    d = GDev(data["p"], dev, **ogr.CASES[name]).run(_case_grads(data, name))
    _against_refs(d, ref, truth, name)
    f = d.fields()
    assert f["clipped"] == 4 == ref.clipped and f["skipped"] == 0 and d.step.tolist() == [5, 0]
    # the lr_scale = 0 segment has not moved, its moments have
    p0 = data["p"].to(dev)
    assert torch.equal(_bits(d.p[4099:4101]), _bits(p0[4099:4101]))
    assert float(d.m[4099:4101].abs().min()) > 0.0 and float(d.v[4099:4101].min()) > 0.0
    # the neighbours on both sides of it did
    assert float((d.p[4095:4099] - p0[4095:4099]).abs().min()) > 0.0
    assert float((d.p[4101:4105] - p0[4101:4105]).abs().min()) > 0.0
    if name.startswith("decoupled"):
        # segment 1 (both scales 1) is the ungrouped decoupled run
        ung = GDev(data["p"], dev, **ogr.CASES["decoupled_ungrouped"]).run(_case_grads(data, name))
        close(d.p[:4099], ung.p[:4099], ADAM_TOL, "segment 1 against the ungrouped run")
        close(ung.p, refs["decoupled_ungrouped"][1].p, ADAM_TOL, "ungrouped decoupled (stock torch)")
        close(ung.avg, refs["decoupled_ungrouped"][1].avg, ADAM_TOL, "ungrouped decoupled avg")
        # and the coupled run is far from the decoupled one: the switch is not ignored
        assert float((d.p - refs["coupled_grouped"][1].p.to(dev)).abs().max()) > 1e-2


# ---- 4. unit scales -----------------------------------------------------------------------------------------
def test_unit_scales_equal_the_ungrouped_launch(dev, data, refs):
    grads = data["on_dev"]["clip"]
    seg = GDev(data["p"], dev, **ogr.CASES["unit_scales"]).run(grads)
    one = GDev(data["p"], dev).run(grads)
    ex = GDev(data["p"], dev).run(grads, "ex")
    for k in ("p", "m", "v"):
        close(getattr(seg, k), getattr(one, k), ADAM_TOL, f"unit scales {k}")
        close(getattr(seg, k), getattr(ex, k), ADAM_TOL, f"unit scales {k} (pca_adam_step_ex)")
    _against_refs(seg, *refs["unit_scales"], "unit scales")
    assert torch.equal(seg.step, one.step) and torch.equal(seg.state, one.state)


# ---- 5. skip --------------------------------------------------------------------------------------------------
def test_a_skipped_step_leaves_the_average_and_is_not_counted(dev, data, refs):
    ref, truth = refs["skip"]
    d = GDev(data["p"], dev, zero_grad=1, **ogr.CASES["skip"])
    for it, g in enumerate(_case_grads(data, "skip")):
        before = [t.clone() for t in (d.p, d.m, d.v, d.avg)]
        d.run([g])
        assert d.step.tolist() == [it + 1, 0]
        assert float(d.g.abs().max()) == 0.0                      # cleared, the NaN included
        same = [torch.equal(_bits(a), _bits(b)) for a, b in zip(before, (d.p, d.m, d.v, d.avg))]
        assert all(same) if it == 2 else not any(same), (it, same)
        assert d.fields()["skipped"] == (it >= 2)
    f = d.fields()
    assert f["skipped"] == 1 and f["norm_count"] == 4 and math.isfinite(f["last_norm"])
    assert truth.applied == 4 and truth.averaged == 4            # four times, not five
    _against_refs(d, ref, truth, "skip")


# ---- 6. the scalar path and tiny n ------------------------------------------------------------------------------
def test_misaligned_vectors_take_the_scalar_path(dev, data, refs):
    name = "decoupled_grouped_averaged_clipped"
    grads = _case_grads(data, name)
    mis = GDev(data["p"], dev, offset=1, zero_grad=1, **ogr.CASES[name])
    assert all(t.data_ptr() % 16 == 4 for t in (mis.p, mis.g, mis.m, mis.v, mis.avg))
    guard = [t._base[0].item() for t in (mis.p, mis.m, mis.v)]    # the float in front of each vector
    mis.run(grads)
    ali = GDev(data["p"], dev, **ogr.CASES[name]).run(grads)
    for k in ("p", "m", "v", "avg"):
        close(getattr(mis, k), getattr(ali, k), ADAM_TOL, f"misaligned {k}")
    _against_refs(mis, *refs[name], "misaligned")
    assert torch.equal(mis.step, ali.step) and torch.equal(mis.state, ali.state)
    assert float(mis.g.abs().max()) == 0.0
    assert guard == [t._base[0].item() for t in (mis.p, mis.m, mis.v)] == [0.0] * 3
    assert all(float(t._base[-4:].abs().max()) == 0.0 for t in (mis.p, mis.m, mis.v, mis.avg))


def test_three_elements_in_two_segments_and_an_empty_vector(dev):
    g = torch.Generator().manual_seed(3)
    p = torch.randn(3, generator=g)
    grads = [torch.randn(3, generator=g) for _ in range(3)]
    kw = dict(seg_end=(1, 3), lr_scale=(0.5, 1.0), wd_scale=(0.0, 1.0), decoupled=True, avg_decay=0.9)
    ref, truth = ogr.GroupsRef(p, **kw), ogr.StockTruth(p, **kw)
    for x in grads:
        ref.step(x)
        truth.step(x)
    d = GDev(p, dev, **kw).run([x.to(dev) for x in grads])
    _against_refs(d, ref, truth, "n = 3")
    assert d.step.tolist() == [3, 0] and float(d.p._base[3:].abs().max()) == 0.0
    # n = 0: nothing but the count moves
    e = GDev(torch.zeros(0), dev, avg_decay=0.5)
    for t in (e.p, e.g, e.m, e.v, e.avg):
        t._base.fill_(3.0)
    e.run([torch.zeros(0, device=dev)] * 2)
    assert e.step.tolist() == [2, 0] and e.fields()["skipped"] == 0
    assert all(bool((t._base == 3.0).all()) for t in (e.p, e.g, e.m, e.v, e.avg))


# ---- 7. replay --------------------------------------------------------------------------------------------------
def test_graph_replay_equals_eager_and_eager_repeats_bitwise(dev, data):
    name = "decoupled_grouped_averaged_clipped"
    grads = _case_grads(data, name)
    kw = dict(ogr.CASES[name], skip_nonfinite=True, table=[2e-3, 6e-3, 1e-2, 5e-3], zero_grad=1)
    e1 = GDev(data["p"], dev, **kw).run(grads)
    e2 = GDev(data["p"], dev, **kw).run(grads)
    names = ("p", "m", "v", "avg", "step", "state")
    _same_bits(e1, e2, names, "two eager runs")
    r = GDev(data["p"], dev, **kw)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        for g in grads:
            r.enqueue(g)
    torch.cuda.synchronize()
    assert r.step.tolist() == [0, 0] and torch.equal(r.p, data["p"].to(dev))     # captured, not run
    graph.replay()
    torch.cuda.synchronize()
    _same_bits(r, e1, names, "graph replay against eager")
    assert r.fields()["clipped"] == 4


# ---- 8. the Trainer against a stock loop ----------------------------------------------------------------------
WD_T, DECAY_T = 0.1, 0.9


@pytest.fixture(scope="module")
def stock_adamw(dev, golden_train):
    """The module path of test_train_trajectory_golden under torch.optim.AdamW in two param groups (decay,
    and none for biases, I and S) and an AveragedModel with the EMA update."""
    import models
    import pca_hip
    from torch.optim.swa_utils import AveragedModel, get_ema_multi_avg_fn
    B, N, din, d, h, m, Cc, steps = [int(v) for v in golden_train["cfg"]]
    net = models.ST(dim_input=din, num_outputs=1, dim_output=Cc, num_inds=m, dim_hidden=d,
                    num_heads=h).to(dev)
    net.load_state_dict({k: T(v) for k, v in golden_train.sub("p0/").items()})
    plain = lambda k: k.endswith(".bias") or k.endswith(".I") or k.endswith(".S")
    named = list(net.named_parameters())
    opt = torch.optim.AdamW([dict(params=[p for k, p in named if not plain(k)], weight_decay=WD_T),
                             dict(params=[p for k, p in named if plain(k)], weight_decay=0.0)],
                            lr=1e-3, betas=(0.9, 0.999), eps=1e-8)
    assert len(opt.param_groups[1]["params"]) == 24
    ema = AveragedModel(net, multi_avg_fn=get_ema_multi_avg_fn(DECAY_T))
    losses = []
    for s in range(steps):
        X = T(gi.pc_input(5000 + s, B, N, din), dev)
        y = T(gi.labels(6000 + s, B, Cc), dev)
        loss = pca_hip.cross_entropy(net(X), y)
        opt.zero_grad(set_to_none=True)
        loss.backward()
        opt.step()
        ema.update_parameters(net)
        losses.append(float(loss))
    torch.cuda.synchronize()
    params = [p for _, p in named]
    flat = lambda ts: torch.cat([t.detach().reshape(-1) for t in ts]).cpu()
    return dict(losses=losses, m=flat([opt.state[p]["exp_avg"] for p in params]),
                v=flat([opt.state[p]["exp_avg_sq"] for p in params]),
                state={k: v.detach().cpu().clone() for k, v in net.state_dict().items()},
                avg={k: v.detach().cpu().clone() for k, v in ema.module.state_dict().items()})


@pytest.mark.parametrize("use_graph", [False, True], ids=["eager", "hipgraph"])
def test_trainer_against_stock_adamw_loop(dev, golden_train, stock_adamw, use_graph):
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
    tr = trainer.Trainer(net, ds, B, lr=1e-3, weight_decay=WD_T, use_graph=use_graph, shuffle=False,
                         decoupled_weight_decay=True, param_groups=trainer.no_decay_groups(),
                         average_decay=DECAY_T)
    assert tr.norm_partials is None and tr.optim_state is not None        # one launch, no norm
    losses = []
    for s in range(steps):
        tr.step()
        losses.append(float(tr.eng.loss))
    stock = stock_adamw
    print("loss err", max(abs(a - b) for a, b in zip(losses, stock["losses"])))
    np.testing.assert_allclose(losses, stock["losses"], rtol=0, atol=5e-4)
    for k, v in net.state_dict().items():
        close(v, stock["state"][k], 3e-3, k)
    avg = tr.averaged_state_dict()
    assert list(avg) == list(net.state_dict()) and all(not t.is_cuda for t in avg.values())
    for k, v in avg.items():
        close(v, stock["avg"][k], 3e-3, "averaged " + k)
    # the average is not the weights: the run moved
    assert float((tr.averaged - tr.eng.flat).abs().max()) > 1e-4
    shapes = gb.shapes_of(net)
    gb.judge(tr.m, stock["m"], MOMENT_BAR, shapes, "Trainer.m vs stock AdamW loop")
    gb.judge(tr.v, stock["v"], MOMENT_BAR, shapes, "Trainer.v vs stock AdamW loop")
    o = tr.read_optim_stats()
    assert o["skipped"] == 0 and o["clipped"] == 0 and o["lr"] == float(np.float32(1e-3))


# ---- 9. / 10. cfg2, bf16: graph against eager, exact resume --------------------------------------------------
def _options(cfg2):
    from pca_hip import trainer
    return dict(decoupled_weight_decay=True, param_groups=trainer.no_decay_groups(), average_decay=0.99,
                max_grad_norm=cfg2["M"])


def test_trainer_bf16_graph_equals_eager_bitwise_new_options_on(dev, cfg2):
    from pca_hip import _lib, trainer

    def run(graph):
        tr = trainer.Trainer(cfg2["net"](), cfg2["ds"], 128, mode=_lib.MODE_BF16, use_graph=graph, seed=1,
                             **_options(cfg2))
        for _ in range(12):
            tr.step()
        torch.cuda.synchronize()
        return (tr.eng.flat.clone(), tr.m.clone(), tr.v.clone(), tr.averaged.clone(),
                tr.step_count.clone(), tr.optim_state.clone()), tr.read_optim_stats()

    (g1, o1), (e1, _), (g2, _) = run(True), run(False), run(True)
    print("new options on:", o1)
    assert torch.isfinite(g1[0]).all() and torch.isfinite(g1[3]).all() and int(g1[4][0]) == 12
    assert o1["skipped"] == 0 and o1["clipped"] >= 1
    assert float((g1[3] - g1[0]).abs().max()) > 0.0
    for other in (e1, g2):
        for a, b, name in zip(g1, other, ("parameters", "m", "v", "averaged", "step words", "optim state")):
            assert torch.equal(_bits(a), _bits(b)), name


def test_exact_resume_new_options_on(dev, cfg2, tmp_path):
    import runfiles
    from pca_hip import _lib, trainer
    K = 8
    kw = dict(mode=_lib.MODE_BF16, seed=1, lr_schedule=trainer.warmup_cosine(1e-3, 12, 26),
              skip_nonfinite=True, **_options(cfg2))

    def state(tr):
        torch.cuda.synchronize()
        return (tr.eng.flat.clone(), tr.m.clone(), tr.v.clone(), tr.step_count.clone(),
                tr.optim_state.clone(), tr.averaged.clone())

    def same(a, b):
        for x, y, name in zip(a, b, ("parameters", "m", "v", "step_count", "optim state", "averaged")):
            assert torch.equal(_bits(x), _bits(y)), name

    straight = trainer.Trainer(cfg2["net"](), cfg2["ds"], 128, **kw)
    for _ in range(2 * K):
        straight.step()
    want = state(straight)
    first = trainer.Trainer(cfg2["net"](), cfg2["ds"], 128, **kw)
    for _ in range(K):
        first.step()
    path = str(tmp_path / "groups.ckpt")
    runfiles.save_checkpoint(path, first)
    saved = torch.load(path, weights_only=True)["trainer"]                 # tensors and plain values only
    assert saved["avg"].dtype == torch.float32 and saved["avg"].numel() == first.eng.flat.numel()
    so = saved["optim"]
    assert so["decoupled"] is True and so["average_decay"] == 0.99 and so["average_start"] == 1
    assert so["seg_end"].dtype == torch.int64 and int(so["seg_end"][-1]) == first.eng.flat.numel()
    assert so["seg_lr_scale"].numel() == so["seg_wd_scale"].numel() == so["seg_end"].numel()
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

    # other options than the checkpoint's are refused, by name
    def refused(match, **change):
        other = trainer.Trainer(cfg2["net"](), cfg2["ds"], 128, **dict(kw, **change))
        with pytest.raises(ValueError, match=match):
            runfiles.load_checkpoint(path, other)
        return other

    refused("average_decay", average_decay=0.9)
    refused("average_start", average_start=3)
    refused("decoupled_weight_decay", decoupled_weight_decay=False)
    refused("param_groups", param_groups=[(r"\.bias$", 1.0, 0.0)])
    refused("param_groups", param_groups=[(r"\.bias$", 0.5, 0.0), (r"\.I$", 1.0, 0.0), (r"\.S$", 1.0, 0.0)])
    refused("param_groups", param_groups=None)
    # a checkpoint from a Trainer without the new options holds none of them: it loads where they are
    # off, and a Trainer with them on refuses it by name
    old = dict(kw, decoupled_weight_decay=False, param_groups=None, average_decay=None)
    plain = trainer.Trainer(cfg2["net"](), cfg2["ds"], 128, **old)
    with pytest.raises(ValueError, match="decoupled_weight_decay"):
        runfiles.load_checkpoint(path, plain)
    runfiles.save_checkpoint(path, plain)
    so = torch.load(path, weights_only=True)["trainer"]
    assert "avg" not in so and "decoupled" not in so["optim"] and "seg_end" not in so["optim"]
    runfiles.load_checkpoint(path, plain)
    with pytest.raises(ValueError, match="decoupled_weight_decay"):
        runfiles.load_checkpoint(path, second)
    with pytest.raises(ValueError, match="average_decay"):
        runfiles.load_checkpoint(path, trainer.Trainer(cfg2["net"](), cfg2["ds"], 128,
                                                       **dict(old, average_decay=0.99)))


# ---- 11. evaluation on the averaged weights -------------------------------------------------------------------
def test_evaluation_on_the_averaged_weights(dev):
    from pca_hip import _lib, trainer
    from test_gpu_trainer_eval import _dense_2d, _net
    ds = _dense_2d(dev)
    kw = dict(mode=_lib.MODE_F32, seed=1, lr=1e-2, average_decay=0.9)
    net = _net(dev, 2)
    tr = trainer.Trainer(net, ds, 32, **kw)
    for _ in range(10):
        tr.step()
    on_avg = trainer.Evaluator(net, ds, 32).use_params(tr.averaged).run()
    on_model = trainer.Evaluator(net, ds, 32).run()
    net2 = _net(dev, 2, seed=11)
    net2.load_state_dict(tr.averaged_state_dict())
    want = trainer.Evaluator(net2, ds, 32).run()
    for k in ("n", "n_skipped", "acc", "topk_acc"):
        assert on_avg[k] == want[k], k
    assert torch.equal(on_avg["confusion"], want["confusion"])
    assert abs(on_avg["loss"] - want["loss"]) <= 1e-6 * abs(want["loss"])
    assert abs(on_avg["loss"] - on_model["loss"]) > 1e-4 * abs(on_model["loss"])
    # an engine asked for the attention reads the given weights too
    eng = trainer.STEngine(net, 32, ds.num_points, training=False)
    X = ds.batch(torch.arange(32, device=dev))[0]
    got = eng.attention(X, params=tr.averaged)[0].clone()
    assert torch.equal(got, eng.forward(X, params=tr.averaged))
    assert not torch.equal(got, eng.forward(X))

    def fit(which):
        t = trainer.Trainer(_net(dev, 2), ds, 32, eval_weights=which, **kw)
        lines = []
        with HostReads() as reads:
            hist = t.fit(2, test_dataset=ds, eval_every=1, log=lines.append)
        return hist, reads.n, lines

    (hm, nm, lm), (hb, nb, lb), (ha, na, _) = fit("model"), fit("both"), fit("averaged")
    assert nb == nm + 2 and na == nm, (nm, nb, na)                 # one more read per evaluated epoch
    assert len(lb) == len(lm) + 2 and "averaged weights test loss" in lb[2]
    # (the three runs are separate fp32 trainings, which repeat to rounding only: not compared in value)
    for e in range(2):
        assert "test_avg_loss" not in hm[e] and "test_avg_loss" not in ha[e]
        assert {"test_loss", "test_acc", "test_topk_acc"} <= set(hm[e]) & set(ha[e]) & set(hb[e])
        assert {"test_avg_loss", "test_avg_acc", "test_avg_topk_acc"} <= set(hb[e])
        assert 0.0 <= hb[e]["test_avg_acc"] <= hb[e]["test_avg_topk_acc"] <= 1.0
        assert math.isfinite(hb[e]["test_avg_loss"]) and hb[e]["test_avg_loss"] != hb[e]["test_loss"]
    with pytest.raises(ValueError, match="average_decay"):
        trainer.Trainer(_net(dev, 2), ds, 32, mode=_lib.MODE_F32, eval_weights="averaged")
    plain = trainer.Trainer(_net(dev, 2), ds, 32, mode=_lib.MODE_F32)
    plain.eval_weights = "both"                                    # the attribute is checked by fit
    with pytest.raises(ValueError, match="average_decay"):
        plain.fit(1)


# ---- 12. defaults untouched -----------------------------------------------------------------------------------
def test_a_default_trainer_holds_none_of_it(dev, cfg2):
    """cfg2 in bf16, the configuration the existing bitwise tests run: its step repeats bit for bit."""
    from pca_hip import _lib, trainer

    def run():
        tr = trainer.Trainer(cfg2["net"](), cfg2["ds"], 128, mode=_lib.MODE_BF16, seed=1)
        for _ in range(5):
            tr.step()
        torch.cuda.synchronize()
        return tr

    a, b = run(), run()
    assert a.averaged is None and a.optim_state is None and a.groups is None and not a._groups_on
    assert a._seg_end is None and a.norm_partials is None
    for x, y, name in ((a.eng.flat, b.eng.flat, "parameters"), (a.m, b.m, "m"), (a.v, b.v, "v"),
                       (a.step_count, b.step_count, "step words")):
        assert torch.equal(_bits(x), _bits(y)), name
    assert "optim" not in a.state_dict() and "avg" not in a.state_dict()
    with pytest.raises(_lib.PcaHipError):
        a.averaged_state_dict()
    with pytest.raises(_lib.PcaHipError):
        a.read_optim_stats()
