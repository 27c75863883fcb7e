"""PCEN point sets through the datasets, the Trainer, the Evaluator and the sweep on the device:
ESC_wave_pc[_temp](bands=, pcen=) is the pca_hip.frame_points_pcen call, with_pcen(None) is the band dataset
bit for bit, a d = 128 model trains on a 256-point PCEN set with fresh draws per replay and resumes bit for
bit, and evalsweep.pcen_sweep is one _dataset_accuracy pass per spec beside the log-band column."""
import json

import numpy as np
import pytest
import torch

from oracle import st_oracle as orc
from test_gpu_trainer_eval import _net, _resume_case, _state

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


@pytest.mark.parametrize("ntemp", [1, 4], ids=["2d", "3d"])
def test_dataset_batch_is_the_ops_call_and_with_pcen_none_the_band_dataset(ntemp, corpus, dev):
    import dataset
    import pca_hip
    clips, y = corpus
    bank = pca_hip.mel_bank(FS, 256, 16)
    spec = pca_hip.Pcen(context=5, time_constant=0.02)
    kw = dict(jitter=40, gain_db=6.0, win_lengths=(256, 200), norm="win", seed=4, device=dev, bands=bank)
    make = (lambda **k: dataset.ESC_wave_pc(clips, y, FS, 256, **kw, **k)) if ntemp == 1 else \
        (lambda **k: dataset.ESC_wave_pc_temp(clips, y, FS, 256, ntemp, **kw, **k))
    ds, band = make(pcen=spec), make()
    din = 2 if ntemp == 1 else 3
    n = len(ds)
    assert ds.stochastic and ds.F == 16 and ds.num_points == 16 * ntemp and n == len(band)
    idx = torch.tensor([0, n - 1, 5, 5, 9, 2, n // 2], device=dev)
    ds._draw = 6
    pts, lab, meta = ds.batch(idx, want_meta=True)
    assert ds._draw == 7 and tuple(pts.shape) == (7, 16 * ntemp, din) and tuple(meta.shape) == (7, 4)
    waves, woff, soff, _, t32, clab = ds._resident()
    f32 = torch.as_tensor(bank.centres / FS).float().to(dev)
    wins = torch.tensor([256, 200], dtype=torch.int32, device=dev)
    want = pca_hip.frame_points_pcen(waves, woff, soff, idx, 256, 128, bank, f32, t32, ntemp, pcen=spec, fs=FS,
                                     max_len=max(len(c) for c in clips), min_len=min(len(c) for c in clips),
                                     clip_labels=clab, norm_mode=pca_hip.NORM_WIN, seed=4, jitter=40,
                                     gain_db=6.0, win_lengths=wins, draw=7, want_meta=True)
    assert torch.equal(_bits(pts), _bits(want[0])) and torch.equal(lab, want[1]) and torch.equal(meta, want[2])
    assert bool(torch.isfinite(pts).all()) and float(pts[:, :, -1].min()) >= 0.0   # bias^r is the floor
    # the band dataset: the same draws, another value column
    band._draw = 6
    bpts, blab, bmeta = band.batch(idx, want_meta=True)
    assert torch.equal(meta, bmeta) and torch.equal(lab, blab)
    assert torch.equal(_bits(pts[:, :, :-1]), _bits(bpts[:, :, :-1]))
    assert not torch.equal(_bits(pts[:, :, -1]), _bits(bpts[:, :, -1]))
    # with_pcen(None) is it, bit for bit, on the same resident waveforms
    back = ds.with_pcen(None)
    assert back._draw == 7 and back._store is ds._store and back.bands is bank
    back._draw = 6
    a = back.batch(idx, want_meta=True)
    assert torch.equal(_bits(a[0]), _bits(bpts)) and torch.equal(a[1], blab) and torch.equal(a[2], bmeta)
    # buffers passed in, as the Trainer passes them; plain() keeps the spec and drops the draws
    o2, l2 = torch.full_like(pts, 3.0), torch.zeros(7, dtype=torch.int64, device=dev)
    ds._draw = 6
    ds.batch(idx, out=o2, labels_out=l2)
    assert torch.equal(_bits(o2), _bits(pts)) and torch.equal(l2, lab)
    p = ds.plain()
    assert p.pcen is spec and not p.stochastic
    q1, q2 = p.batch(idx), p.batch(idx)
    assert torch.equal(_bits(q1[0]), _bits(q2[0]))
    item, lbl = p[5]
    assert torch.equal(item, q1[0][2].cpu()) and int(lbl) == int(q1[1][2])


@pytest.mark.parametrize("graph", [True, False], ids=["hipgraph", "eager"])
def test_trainer_steps_on_a_pcen_set_and_resumes(dev, tmp_path, graph):
    import dataset
    import pca_hip
    from pca_hip import _lib, trainer
    B, N = 4, 256
    lengths, y = [10000, 20300, 8000], [1, 8, 3]                          # 4 + 9 + 3 = 16 sets of 16 frames
    clips = [orc.synth_clip(90 + i, 2 * i, seconds=n / FS + 0.01)[:n] for i, n in enumerate(lengths)]

    def make():
        d = dataset.ESC_wave_pc_temp(clips, y, FS, 256, 16, jitter=64, gain_db=6.0, seed=9, device=dev,
                                     bands=pca_hip.mel_bank(FS, 256, 16),
                                     pcen=pca_hip.Pcen(context=8, time_constant=0.03))
        assert len(d) == 16 and d.num_points == N and d.F == 16 and d.stochastic   # 4 steps per epoch
        return _net(dev, 3, seed=4), d, dict(seed=5, batch_size=B, mode=_lib.MODE_BF16)

    net, ds, kw = make()
    tr = trainer.Trainer(net, ds, use_graph=graph, **kw)
    assert tr.lengths is None and tr.N == N
    losses, batches = [], []
    for _ in range(3):
        tr.step()
        torch.cuda.synchronize()
        losses.append(float(tr.eng.loss))
        batches.append(tr.X.clone())
    assert all(np.isfinite(losses)) and len(set(losses)) == 3, losses
    assert torch.isfinite(_state(tr)[0]).all()
    assert not torch.equal(batches[0], batches[1])                        # fresh draws per step / replay
    # the batches are the dataset's: step s by hand
    net, ds2, _ = make()
    X = torch.empty((B, N, 3), device=dev)
    lab = torch.zeros(B, dtype=torch.int64, device=dev)
    step_count = torch.zeros(2, dtype=torch.int32, device=dev)
    stream = trainer.ShardedIndexStream(len(ds2), B, 0, 1, 5, True, dev)
    for s in range(3):
        if graph:                  # a captured step froze the host draw number of its recorded call, the 2nd
            ds2._draw = 1
        step_count[0] = s
        ds2.batch(stream.next().clone(), out=X, labels_out=lab, draw_dev=step_count)
        assert torch.equal(_bits(X), _bits(batches[s])), s
    # 6 steps straight = 3 steps + checkpoint + a fresh Trainer + 3 steps, bitwise
    _resume_case(make, 3, tmp_path, graph=graph)
    r = trainer.Evaluator(net, ds.plain(), 8, _lib.MODE_BF16).run()
    assert r["n"] == 16 and np.isfinite(r["loss"])


def test_pcen_sweep(corpus, dev, tmp_path):
    import dataset
    import evalsweep
    import models
    import pca_hip
    clips, y = corpus
    clips = [torch.from_numpy(c).to(dev) for c in clips]
    torch.manual_seed(11)
    net = models.ST(dim_input=3, num_outputs=1, dim_output=10, num_inds=4, dim_hidden=16,
                    num_heads=4).to(dev).eval()
    bank = pca_hip.mel_bank(FS, 256, 16)
    specs = {"fast": pca_hip.Pcen(context=4, time_constant=0.01), "slow": pca_hip.Pcen(context=12, s=0.05)}
    path = str(tmp_path / "pcen.json")
    out = evalsweep.pcen_sweep(net, clips, y, FS, 256, bank, specs, Ntemp=4, batch_size=8, json_file=path,
                               sets_per_call=6)
    assert sorted(out) == ["bank", "data", "list_specs", "specs"]
    assert list(out["data"]) == out["list_specs"] == ["log", "fast", "slow"]
    assert out["specs"] == [None, specs["fast"].summary(), specs["slow"].summary()]
    assert out["bank"] == bank.summary()
    assert json.load(open(path)) == json.loads(json.dumps(out))
    acc = lambda d: evalsweep._dataset_accuracy(net, d, None, 3, 8, evalsweep._lib.MODE_F32, 6)  # noqa: E731
    for name, spec in [("log", None)] + list(specs.items()):
        ds = dataset.ESC_wave_pc_temp(clips, y, FS, 256, 4, device=dev, bands=bank, pcen=spec)
        assert len(ds) >= 8
        assert out["data"][name] == [acc(ds), 0]
    assert all(np.isfinite(v[0]) and 0.0 <= v[0] <= 1.0 for v in out["data"].values())
    # a list of specs, 2-D sets
    net2 = models.ST(dim_input=2, num_outputs=1, dim_output=10, num_inds=4, dim_hidden=16,
                     num_heads=4).to(dev).eval()
    out = evalsweep.pcen_sweep(net2, clips, y, FS, 256, bank, [specs["slow"]], batch_size=8, sets_per_call=6)
    assert out["list_specs"] == ["log", "pcen0"] and len(out["data"]) == 2
