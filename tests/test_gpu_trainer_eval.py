"""trainer.Evaluator, Trainer.fit and the exact resume (Trainer.state_dict / load_state_dict,
runfiles.save_checkpoint / load_checkpoint) on the device.

Resume is held to bitwise equality, so it is tested where the step is bit-reproducible: bf16 at d = 128
(the shapes of test_trainer_bf16_graph_equals_eager_bitwise and test_d128_step_is_bit_reproducible) and
fp32 at a toy size whose weight-gradient GEMMs stay below the split-K threshold.  d = 64 is excluded: its
weight gradients (csrc/wgrad64.hip) still use fp32 atomics, so two identical runs differ there already."""
import importlib.util
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from conftest import ROOT
from test_gpu_clip import HostReads
from test_gpu_ddp import _free_port

pytestmark = pytest.mark.gpu

TOL = 1e-4          # the fp32 forward bar of tests/test_gpu_clip.py


@pytest.fixture(scope="module")
def dev():
    return torch.device("cuda", 0)


def _dense_2d(dev, T=333, F=64, C=10, seed=17):
    import dataset
    rng = np.random.Generator(np.random.PCG64(seed))
    x = rng.normal(-9, 3, size=(F, T)).astype(np.float32)
    y = rng.integers(0, C, size=(T,))
    return dataset.ESC_pc(x, y, np.linspace(0, 0.5, F), device=dev)


def _varlen_3d(dev, S=45, F=32, Nt=4, C=10, seed=23):
    import dataset
    rng = np.random.Generator(np.random.PCG64(seed))
    x = rng.normal(-9, 3, size=(F, Nt, S)).astype(np.float32)
    y = rng.integers(0, C, size=(S,))
    ntv = rng.integers(1, Nt + 1, size=(S,)).astype(np.int32)
    assert ntv.min() < Nt
    return dataset.ESC_pc_temp(x, y, np.linspace(0, 0.5, F), np.linspace(0, 1, Nt), device=dev,
                               nt_valid=ntv)


def _net(dev, din, C=10, d=128, h=4, m=16, seed=5):
    import models
    torch.manual_seed(seed)
    return models.ST(dim_input=din, dim_output=C, num_inds=m, dim_hidden=d, num_heads=h).to(dev)


def _engine_logits(net, ds, batch, dev):
    """The engine's own logits and the labels of the whole set, in order, batch by batch."""
    from pca_hip.trainer import STEngine
    parts, labs, done, n = [], [], 0, len(ds)
    while done < n:
        b = min(batch, n - done)
        eng = STEngine(net, b, ds.num_points, training=False)
        while done + b <= n:
            res = ds.batch(torch.arange(done, done + b, device=dev))
            parts.append(eng.forward(res[0], res[2] if len(res) > 2 else None).clone())
            labs.append(res[1].clone())
            done += b
    return torch.cat(parts), torch.cat(labs)


# ---- Evaluator ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["dense2d", "varlen3d"])
def test_evaluator_equals_evaluate_and_float64_loss(kind, dev):
    from pca_hip import trainer
    ds = _dense_2d(dev) if kind == "dense2d" else _varlen_3d(dev)
    net = _net(dev, 2 if kind == "dense2d" else 3)
    batch = 32 if kind == "dense2d" else 16
    n = len(ds)
    assert n % batch
    acc, n_ev = trainer.evaluate(net, ds, batch)
    ev = trainer.Evaluator(net, ds, batch, topk=3)
    assert len(ev.engines) == 2                                    # full batches and the tail
    with HostReads() as reads:
        out = ev.run()
    assert reads.n == 1, reads.n
    assert out["n"] == n == n_ev and out["n_skipped"] == 0
    correct = round(acc * n)
    assert abs(acc * n - correct) < 1e-6
    assert round(out["acc"] * n) == correct and abs(out["acc"] * n - correct) < 1e-6
    logits, labels = _engine_logits(net, ds, batch, dev)
    assert torch.equal(ev.logits, logits) and torch.equal(ev.labels, labels)
    ref = torch.nn.functional.cross_entropy(logits.double().cpu(), labels.cpu(), reduction="none")
    want = float(ref.mean())
    print(f"{kind}: loss {out['loss']:.6f} fp64 {want:.6f}, acc {out['acc']:.4f}, top-3 {out['topk_acc']:.4f}")
    assert abs(out["loss"] - want) <= TOL * max(1.0, abs(want))
    conf = out["confusion"]
    pred = logits.argmax(1).cpu()
    want_conf = torch.zeros(10, 10, dtype=torch.int64).index_put_((labels.cpu(), pred),
                                                                   torch.ones(n, dtype=torch.int64), accumulate=True)
    assert torch.equal(conf, want_conf) and int(conf.diagonal().sum()) == correct
    rank = (logits > logits.gather(1, labels[:, None])).sum(1).cpu()     # no ties in these logits
    assert round(out["topk_acc"] * n) == int((rank < 3).sum())
    pc = out["per_class_acc"]
    rows = conf.sum(1)
    assert torch.equal(pc[rows > 0], conf.diagonal()[rows > 0].double() / rows[rows > 0].double())
    # a second run gives the same figures (the accumulators are cleared per run)
    again = ev.run()
    assert again["loss"] == out["loss"] and torch.equal(again["confusion"], conf)


def test_evaluator_shares_the_trainers_weights(dev):
    """Built after the Trainer, the Evaluator's engines read the flat vector Adam updates: no copy."""
    from pca_hip import _lib, trainer
    ds = _dense_2d(dev)
    net = _net(dev, 2)
    tr = trainer.Trainer(net, ds, 32, lr=1e-2, mode=_lib.MODE_F32, seed=1)
    ev = trainer.Evaluator(net, ds, 32)
    assert all(e.flat.data_ptr() == tr.eng.flat.data_ptr() for e, _, _ in ev.engines)
    before = ev.run()
    for _ in range(3):
        tr.step()
    after = ev.run()
    assert after["loss"] != before["loss"]
    logits, labels = _engine_logits(net, ds, 32, dev)                 # the weights as they are now
    want = float(torch.nn.functional.cross_entropy(logits.double().cpu(), labels.cpu()))
    assert abs(after["loss"] - want) <= TOL * max(1.0, abs(want))


def test_two_ranks_give_the_single_rank_figures(tmp_path, dev):
    """Two gloo ranks on the one GPU (the pattern of tests/test_gpu_ddp.py): contiguous shards of 166
    and 167 sets, one all-reduce of the integers and one of the loss."""
    from pca_hip import _lib, trainer
    script = os.path.join(ROOT, "scripts", "eval_ddp_check.py")
    out = str(tmp_path / "eval.pt")
    env = dict(os.environ, PCA_OUT=out, HSA_ENABLE_IPC_MODE_LEGACY="0")
    r = subprocess.run([sys.executable, "-m", "torch.distributed.run", "--nnodes=1",
                        "--nproc-per-node", "2", "--master-addr", "127.0.0.1",
                        "--master-port", str(_free_port()), script],
                       env=env, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-3000:]
    assert "SHARDS [166, 167]" in r.stdout, r.stdout
    two = torch.load(out, weights_only=True)
    spec = importlib.util.spec_from_file_location("eval_ddp_check", script)
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    net, ds = mod.held_out(dev)
    one = trainer.Evaluator(net, ds, 32, _lib.MODE_F32, topk=3).run()
    assert int(two["n"]) == one["n"] == 333 and int(two["n_skipped"]) == 0
    assert torch.equal(two["confusion"], one["confusion"])
    for k in ("acc", "topk_acc"):
        assert round(float(two[k]) * 333) == round(one[k] * 333), k
    print(f"loss: two ranks {float(two['loss']):.7f}, one rank {one['loss']:.7f}")
    assert abs(float(two["loss"]) - one["loss"]) <= TOL * max(1.0, abs(one["loss"]))


# ---- exact resume ---------------------------------------------------------------------------------------
def _state(tr):
    torch.cuda.synchronize()
    return (tr.eng.flat.clone(), tr.m.clone(), tr.v.clone(), tr.step_count.clone())


def _same_bits(a, b):
    for x, y, name in zip(a, b, ("parameters", "m", "v", "step_count")):
        xi = x.view(torch.int32) if x.dtype == torch.float32 else x
        yi = y.view(torch.int32) if y.dtype == torch.float32 else y
        assert torch.equal(xi, yi), f"{name}: not bitwise equal ({int((xi != yi).sum())} elements differ)"


def _resume_case(make, K, tmp_path, graph):
    """2K steps straight against K steps + checkpoint + a NEW model, dataset object and Trainer +
    load + K steps.  ``make()`` -> (net, dataset, trainer keyword arguments)."""
    import runfiles
    from pca_hip import trainer
    net, ds, kw = make()
    straight = trainer.Trainer(net, ds, use_graph=graph, **kw)
    for _ in range(2 * K):
        straight.step()
    want = _state(straight)
    assert torch.isfinite(want[0]).all() and int(want[3][0]) == 2 * K

    net, ds, kw = make()
    first = trainer.Trainer(net, ds, use_graph=graph, **kw)
    for _ in range(K):
        first.step()
    path = str(tmp_path / "run.ckpt")
    runfiles.save_checkpoint(path, first, config=dict(note="resume test", epochs=3))
    loaded = torch.load(path, weights_only=True)                      # tensors and plain values only
    assert loaded["config"]["epochs"] == 3
    spe = first.indices.steps_per_epoch()
    assert K % spe and (2 * K) // spe > K // spe                      # mid-epoch, and an epoch boundary follows
    half = _state(first)
    del first

    net2, ds2, kw = make()
    with torch.no_grad():
        for p in net2.parameters():
            p.add_(1.0)                                               # not the saved weights
    second = trainer.Trainer(net2, ds2, use_graph=graph, **kw)
    assert runfiles.load_checkpoint(path, second)["note"] == "resume test"
    _same_bits(_state(second), half)
    assert second.g0 is None                                          # the next step re-captures
    for _ in range(K):
        second.step()
    _same_bits(_state(second), want)
    # the module's parameters are the restored vector, not a copy
    assert next(net2.parameters()).data_ptr() == second.eng.flat.data_ptr()
    return path, make


def test_resume_bf16_cfg2_cursor_mode_graph(dev, tmp_path):
    """BASELINE cfg2 (B = 128, N = 512, d = 128, bf16), device cursor, hipGraph replay: 13 steps per
    epoch, checkpoint after step 8."""
    import bench
    import models
    from pca_hip import _lib
    cfg = dict(bench.CONFIGS["cfg2"])
    ds, _ = bench.build_dataset(cfg, 4, dev, seed=0)

    def make():
        torch.manual_seed(1)
        net = models.ST(dim_input=2, dim_output=50, num_inds=16, dim_hidden=128, num_heads=4).to(dev)
        return net, ds, dict(batch_size=128, mode=_lib.MODE_BF16, seed=1)

    path, _ = _resume_case(make, 8, tmp_path, graph=True)
    # a checkpoint of another batch size is refused, and the field is named
    import runfiles
    from pca_hip import trainer
    net, ds, kw = make()
    other = trainer.Trainer(net, ds, **dict(kw, batch_size=64))
    with pytest.raises(ValueError, match=r"\bB\b.*128.*64"):
        runfiles.load_checkpoint(path, other)


def test_resume_f32_toy_plain_batch_mode(dev, tmp_path):
    """fp32, d = 128, B = 4 sets of 48 points (B * N = 192 rows: below the 256 from which the fp32
    weight-gradient GEMM splits K and adds with atomics), a dataset without batch_seq: the Trainer
    uploads an index batch per step.  Eager launches."""
    import dataset
    from pca_hip import _lib
    rng = np.random.Generator(np.random.PCG64(31))
    Kp, Tn, C = 48, 42, 10
    x = rng.normal(-9, 3, size=(Kp, Tn)).astype(np.float32)
    f = np.sort(rng.random((Kp, Tn)).astype(np.float32) * 0.5, axis=0)
    y = rng.integers(0, C, size=(Tn,))

    def make():
        ds = dataset.ESC_pc_ss(x, y, f, device=dev)
        assert not callable(getattr(ds, "batch_seq", None))
        return _net(dev, 2, seed=2), ds, dict(batch_size=4, mode=_lib.MODE_F32, seed=3, lr=1e-3)

    _resume_case(make, 7, tmp_path, graph=False)                      # 10 steps per epoch


@pytest.mark.parametrize("graph", [True, False], ids=["hipgraph", "eager"])
def test_resume_stochastic_random_k(dev, tmp_path, graph):
    """Random-K sub-sampling: the draw number of step s is the device step counter (restored) plus a host
    number that the capture froze / that advances per call (restored with the state), so the resumed
    run draws the same points."""
    import dataset
    from pca_hip import _lib
    rng = np.random.Generator(np.random.PCG64(37))
    F, Nt, S, C = 32, 8, 64, 10
    x = rng.normal(-9, 3, size=(F, Nt, S)).astype(np.float32)
    y = rng.integers(0, C, size=(S,))

    def make():
        ds = dataset.ESC_pc_temp_randKSS(x, y, np.linspace(0, 0.5, F), np.linspace(0, 1, Nt), 100,
                                         device=dev, seed=9)
        assert ds.stochastic
        return _net(dev, 3, seed=4), ds, dict(batch_size=16, mode=_lib.MODE_BF16, seed=5)

    _resume_case(make, 3, tmp_path, graph=graph)                      # 4 steps per epoch
    # the draws do matter: the same run on another dataset seed ends elsewhere
    from pca_hip import trainer
    net, ds, kw = make()
    a = trainer.Trainer(net, ds, use_graph=graph, **kw)
    net, ds, kw = make()
    ds.seed = 10
    b = trainer.Trainer(net, ds, use_graph=graph, **kw)
    for _ in range(2):
        a.step(); b.step()
    assert not torch.equal(_state(a)[0], _state(b)[0])


# ---- fit --------------------------------------------------------------------------------------------------
def test_fit_logs_like_the_reference_and_resumes_bitwise(dev, tmp_path):
    import bench
    import models
    import runfiles
    from pca_hip import _lib, trainer
    cfg = dict(bench.CONFIGS["cfg2"])
    ds, _ = bench.build_dataset(cfg, 3, dev, seed=0)
    test_ds, _ = bench.build_dataset(cfg, 1, dev, seed=1)
    assert len(test_ds) % 128

    def make():
        torch.manual_seed(1)
        net = models.ST(dim_input=2, dim_output=50, num_inds=16, dim_hidden=128, num_heads=4).to(dev)
        return trainer.Trainer(net, ds, 128, mode=_lib.MODE_BF16, seed=1)

    lines = []
    tr = make()
    spe = tr.indices.steps_per_epoch()
    with HostReads() as reads:
        hist = tr.fit(3, test_dataset=test_ds, eval_every=2, log=lines.append)
    # per epoch read_stats' one read of the statistics (and one of the hand-off word where the
    # set-resident forward runs); per held-out pass one
    per_epoch = 1 + (tr.eng._handoff_word is not None)
    assert reads.n == 3 * per_epoch + 2, reads.n
    assert [h["epoch"] for h in hist] == [0, 1, 2]
    assert ["test_loss" in h for h in hist] == [True, False, True]
    assert all(0 <= h["train_acc"] <= 1 and np.isfinite(h["train_loss"]) for h in hist)
    assert len(lines) == 5
    assert lines[0] == f"Epoch 0: train loss {hist[0]['train_loss']:.3f} train acc {hist[0]['train_acc']:.3f}"
    assert lines[1] == f"Epoch 0: test loss {hist[0]['test_loss']:.3f} test acc {hist[0]['test_acc']:.3f}"
    assert lines[2].startswith("Epoch 1: train loss") and lines[4].startswith("Epoch 2: test loss")
    want = _state(tr)
    assert int(want[3][0]) == 3 * spe
    # the held-out figures are those of an Evaluator on the final weights
    res = trainer.Evaluator(tr.eng.model, test_ds, 128, _lib.MODE_BF16).run()
    assert res["loss"] == hist[2]["test_loss"] and res["acc"] == hist[2]["test_acc"]

    # stopped after epoch 1 (two epochs run), continued by a new Trainer from the checkpoint
    path = str(tmp_path / "fit.ckpt")
    first = make()
    h01 = first.fit(2, test_dataset=test_ds, eval_every=2, checkpoint_path=path, log=lines.append)
    assert [h["epoch"] for h in h01] == [0, 1] and h01 == hist[:2]
    second = make()
    runfiles.load_checkpoint(path, second)
    h2 = second.fit(3, test_dataset=test_ds, eval_every=2, log=lines.append)
    assert [h["epoch"] for h in h2] == [2] and h2 == hist[2:]
    _same_bits(_state(second), want)
