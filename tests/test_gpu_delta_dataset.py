"""Delta point sets through the datasets, the Trainer, the Evaluator and the sweep on the device:
ESC_wave_pc[_temp](deltas=) is the pca_hip.frame_points_delta call, with_deltas(None) is the underlying dataset
bit for bit, a d = 128 model trains on 256-point delta sets of din 3 and din 4 on the set-resident launch with
fresh draws per replay and resumes, and evalsweep.delta_sweep is one _dataset_accuracy pass per width."""
import json

import numpy as np
import pytest
import torch

from dispatch import launches
from oracle import st_oracle as orc
from test_gpu_trainer_eval import _net, _resume_case, _same_bits, _state

pytestmark = pytest.mark.gpu

FS = 44100


@pytest.fixture(scope="module")
def dev():
    return torch.device("cuda", 0)


@pytest.fixture(scope="module")
def corpus():
    secs = (0.05, 0.11, 0.2)
    return [orc.synth_clip(40 + i, 3 * i + 1, seconds=s) for i, s in enumerate(secs)], np.array([4, 9, 2])


def _bits(t):
    return t.contiguous().view(torch.int32)


KINDS = {   # Ntemp (1: ESC_wave_pc), bank, drop_nyquist, spec
    "2d-grid-tf": (1, False, False, ("tf", 2)),
    "2d-grid-dropnyq-t": (1, False, True, ("t", 3)),
    "2d-mel-f": (1, True, False, ("f", 1)),
    "3d-grid-f": (4, False, False, ("f", 4)),
    "3d-mel-t": (4, True, False, ("t", 4)),
}


@pytest.mark.parametrize("kind", list(KINDS))
def test_dataset_batch_is_the_ops_call_and_with_deltas_none_the_base_dataset(kind, corpus, dev):
    import dataset
    import pca_hip
    ntemp, banded, dropnyq, (axes, W) = KINDS[kind]
    clips, y = corpus
    bank = pca_hip.mel_bank(FS, 256, 16) if banded else None
    spec = pca_hip.Deltas(axes, W)
    kw = dict(jitter=40, gain_db=6.0, win_lengths=(256, 200), norm="win", seed=4, device=dev, bands=bank)
    make = (lambda **k: dataset.ESC_wave_pc(clips, y, FS, 256, drop_nyquist=dropnyq, **kw, **k)) if ntemp == 1 \
        else (lambda **k: dataset.ESC_wave_pc_temp(clips, y, FS, 256, ntemp, **kw, **k))
    ds, base = make(deltas=spec), make()
    din0 = 2 if ntemp == 1 else 3
    F = 16 if banded else (128 if dropnyq or ntemp > 1 else 129)
    n = len(ds)
    assert ds.stochastic and ds.F == base.F == F and ds.num_points == base.num_points == F * ntemp
    assert n == len(base) and ds.din == din0 + len(axes) and base.din == din0
    idx = torch.tensor([0, n - 1, 5, 5, 9, 2, n // 2], device=dev)
    ds._draw = 6
    pts, lab, meta = ds.batch(idx, want_meta=True)
    assert ds._draw == 7 and tuple(pts.shape) == (7, F * ntemp, ds.din) and tuple(meta.shape) == (7, 4)
    waves, woff, soff, f32, t32, clab = ds._resident()
    if banded:
        f32 = torch.as_tensor(bank.centres / FS).float().to(dev)
    wins = torch.tensor([256, 200], dtype=torch.int32, device=dev)
    want = pca_hip.frame_points_delta(waves, woff, soff, idx, 256, 128, F, f32, t32, ntemp, deltas=spec, bank=bank,
                                      max_len=max(len(c) for c in clips), min_len=min(len(c) for c in clips),
                                      clip_labels=clab, norm_mode=pca_hip.NORM_WIN, seed=4, jitter=40,
                                      gain_db=6.0, win_lengths=wins, draw=7, want_meta=True)
    assert torch.equal(_bits(pts), _bits(want[0])) and torch.equal(lab, want[1]) and torch.equal(meta, want[2])
    assert bool(torch.isfinite(pts).all()) and float(pts[:, :, din0:].abs().max()) > 1e-3
    # the underlying dataset: the same draws, the same rows, no delta columns
    base._draw = 6
    bpts, blab, bmeta = base.batch(idx, want_meta=True)
    assert tuple(bpts.shape) == (7, F * ntemp, din0)
    assert torch.equal(meta, bmeta) and torch.equal(lab, blab)
    assert torch.equal(_bits(pts[:, :, :din0]), _bits(bpts))
    # with_deltas(None) is it, bit for bit, on the same resident waveforms
    back = ds.with_deltas(None)
    assert back._draw == 7 and back._store is ds._store and back.bands is bank and back.din == din0
    back._draw = 6
    a = back.batch(idx, want_meta=True)
    assert torch.equal(_bits(a[0]), _bits(bpts)) and torch.equal(a[1], blab) and torch.equal(a[2], bmeta)
    # buffers passed in, as the Trainer passes them; plain() keeps the spec and drops the draws
    o2, l2 = torch.full_like(pts, 3.0), torch.zeros(7, dtype=torch.int64, device=dev)
    ds._draw = 6
    ds.batch(idx, out=o2, labels_out=l2)
    assert torch.equal(_bits(o2), _bits(pts)) and torch.equal(l2, lab)
    p = ds.plain()
    assert p.deltas is spec and not p.stochastic
    q1, q2 = p.batch(idx), p.batch(idx)
    assert torch.equal(_bits(q1[0]), _bits(q2[0]))
    item, lbl = p[5]
    assert torch.equal(item, q1[0][2].cpu()) and int(lbl) == int(q1[1][2])


def _din3(dev, **over):
    """n_fft 512 without the Nyquist bin: N = 256 grid points of (f, value, dt), 66 sets, 4 steps per epoch."""
    import dataset
    import pca_hip
    lengths, y = [5000, 7000, 4500], [1, 8, 3]                            # 20 + 28 + 18 frames
    clips = [orc.synth_clip(90 + i, 2 * i, seconds=n / FS + 0.01)[:n] for i, n in enumerate(lengths)]
    kw = dict(drop_nyquist=True, jitter=64, gain_db=6.0, seed=9, device=dev, deltas=pca_hip.Deltas("t", 2))
    kw.update(over)
    d = dataset.ESC_wave_pc(clips, y, FS, 512, **kw)
    assert len(d) == 66 and d.num_points == 256 and d.F == 256 and d.din == 3
    return d


def _din4(dev, **over):
    """64 mel bands x 4 frames of n_fft 512: N = 256 points of (f, t, value, dt), 66 sets."""
    import dataset
    import pca_hip
    lengths, y = [20000, 30000, 19000], [1, 8, 3]                         # 79, 118, 75 frames: 19 + 29 + 18 sets
    clips = [orc.synth_clip(90 + i, 2 * i, seconds=n / FS + 0.01)[:n] for i, n in enumerate(lengths)]
    kw = dict(jitter=64, gain_db=6.0, seed=9, device=dev, bands=pca_hip.mel_bank(FS, 512, 64),
              deltas=pca_hip.Deltas("t", 2))
    kw.update(over)
    d = dataset.ESC_wave_pc_temp(clips, y, FS, 512, 4, **kw)
    assert len(d) == 66 and d.num_points == 256 and d.F == 64 and d.din == 4
    return d


MAKERS = {"din3": _din3, "din4": _din4}
B = 16


def _set_resident(net, ds, dev):
    """How often one eager training step on a batch of ``ds`` launches k_set128_fwd (tests/dispatch.py)."""
    from pca_hip import _lib, trainer
    eng = trainer.STEngine(net, B, ds.num_points, _lib.MODE_BF16, training=True)
    X, lab = ds.batch(torch.arange(B, device=dev))
    assert tuple(X.shape) == (B, 256, ds.din) == (eng.cfg.B, eng.cfg.N, eng.cfg.din)
    n = launches(lambda: eng.fwd_bwd(X, lab, phase=-1), ("set_fwd",))["set_fwd"]
    eng.check_handoffs()
    return n


@pytest.mark.parametrize("which", list(MAKERS))
@pytest.mark.parametrize("graph", [True, False], ids=["hipgraph", "eager"])
def test_trainer_steps_on_a_delta_set_and_resumes(dev, tmp_path, graph, which):
    from pca_hip import _lib, trainer

    def make():
        d = MAKERS[which](dev)
        assert d.stochastic
        return _net(dev, d.din, seed=4), d, dict(seed=5, batch_size=B, mode=_lib.MODE_BF16)

    net, ds, kw = make()
    assert _set_resident(_net(dev, ds.din, seed=4), ds.plain(), dev) == 1, "not the set-resident launch"
    tr = trainer.Trainer(net, ds, use_graph=graph, **kw)
    assert tr.lengths is None and tr.N == 256 and tuple(tr.X.shape) == (B, 256, ds.din)
    losses, batches = [], []
    for _ in range(3):
        tr.step()
        torch.cuda.synchronize()
        losses.append(float(tr.eng.loss))
        batches.append(tr.X.clone())
    assert all(np.isfinite(losses)) and len(set(losses)) == 3, losses
    assert torch.isfinite(_state(tr)[0]).all()
    assert all(bool(torch.isfinite(x).all()) for x in batches)
    assert not torch.equal(batches[0], batches[1])                        # fresh draws per step / replay
    # the batches are the dataset's: step s by hand
    _, ds2, _ = make()
    X = torch.empty((B, 256, ds.din), device=dev)
    lab = torch.zeros(B, dtype=torch.int64, device=dev)
    step_count = torch.zeros(2, dtype=torch.int32, device=dev)
    stream = trainer.ShardedIndexStream(len(ds2), B, 0, 1, 5, True, dev)
    for s in range(3):
        if graph:                  # a captured step froze the host draw number of its recorded call, the 2nd
            ds2._draw = 1
        step_count[0] = s
        ds2.batch(stream.next().clone(), out=X, labels_out=lab, draw_dev=step_count)
        assert torch.equal(_bits(X), _bits(batches[s])), s
    if tr.bit_reproducible:
        # 6 steps straight = 3 steps + checkpoint + a fresh Trainer + 3 steps, bitwise
        _resume_case(make, 3, tmp_path, graph=graph)
    else:
        assert which == "din4"         # layer 1's fc_q gradient is summed with atomics at din 4
    r = trainer.Evaluator(net, ds.plain(), B, _lib.MODE_BF16).run()
    assert r["n"] == 66 and np.isfinite(r["loss"])


@pytest.mark.parametrize("which", list(MAKERS))
def test_graph_equals_eager_on_the_same_batches(dev, which):
    """Without augmentation the captured and the eager Trainer see the same batches: where the step is
    bit-reproducible their states are equal bit for bit after 3 steps; elsewhere (din 4: layer 1's fc_q gradient
    is summed with atomics) both runs are finite."""
    from pca_hip import _lib, trainer
    states, losses, rep = [], [], None
    for graph in (True, False):
        ds = MAKERS[which](dev, jitter=0, gain_db=0.0)
        assert not ds.stochastic
        tr = trainer.Trainer(_net(dev, ds.din, seed=4), ds, use_graph=graph, seed=5, batch_size=B,
                             mode=_lib.MODE_BF16)
        rep = tr.bit_reproducible
        run = []
        for _ in range(3):
            tr.step()
            torch.cuda.synchronize()
            run.append(float(tr.eng.loss))
        states.append(_state(tr))
        losses.append(run)
    assert all(np.isfinite(v) for run in losses for v in run), losses
    assert all(bool(torch.isfinite(s[0]).all()) for s in states)
    print(f"delta sets {which}: bit_reproducible {rep}, losses graph {losses[0]} eager {losses[1]}")
    if rep:
        _same_bits(states[0], states[1])
        assert losses[0] == losses[1]
    else:
        assert which == "din4"


def test_delta_sweep(corpus, dev, tmp_path):
    import dataset
    import evalsweep
    import models
    import pca_hip
    from pca_hip import trainer
    clips, y = corpus
    clips = [torch.from_numpy(c).to(dev) for c in (clips[0], clips[1], clips[2][:5600])]   # 4 + 9 + 11 sets
    torch.manual_seed(11)
    net = models.ST(dim_input=4, num_outputs=1, dim_output=10, num_inds=4, dim_hidden=16,
                    num_heads=4).to(dev).eval()
    bank = pca_hip.mel_bank(FS, 256, 16)
    path = str(tmp_path / "delta.json")
    out = evalsweep.delta_sweep(net, clips, y, FS, 256, (1, 2), axes="t", bank=bank, Ntemp=4, batch_size=8,
                                json_file=path, sets_per_call=6)
    assert sorted(out) == ["bank", "data", "list_specs", "specs"]
    assert list(out["data"]) == out["list_specs"] == ["w1", "w2"]
    assert out["specs"] == [dict(axes="t", width=1), dict(axes="t", width=2)]
    assert out["bank"] == bank.summary()
    assert json.load(open(path)) == json.loads(json.dumps(out))
    acc = lambda d: evalsweep._dataset_accuracy(net, d, None, 4, 8, evalsweep._lib.MODE_F32, 6)  # noqa: E731
    for name, W in (("w1", 1), ("w2", 2)):
        ds = dataset.ESC_wave_pc_temp(clips, y, FS, 256, 4, device=dev, bands=bank, deltas=pca_hip.Deltas("t", W))
        assert len(ds) == 24                                              # three full batches, no tail
        assert out["data"][name] == [acc(ds), 0]
        # the Evaluator's accuracy on the same view
        r = trainer.Evaluator(net, ds, 8, evalsweep._lib.MODE_F32).run()
        assert r["n"] == 24 and abs(r["acc"] - out["data"][name][0]) < 1e-12, (name, r["acc"], out["data"][name])
    assert all(np.isfinite(v[0]) and 0.0 <= v[0] <= 1.0 for v in out["data"].values())
    # grid sets, 2-D, two axes: din 4 again
    out = evalsweep.delta_sweep(net, clips, y, FS, 256, [3], axes="tf", batch_size=8, sets_per_call=6,
                                drop_nyquist=True)
    assert out["list_specs"] == ["w3"] and out["bank"] is None and len(out["data"]) == 1
