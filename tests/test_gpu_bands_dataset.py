"""Band point sets through the datasets, the Trainer and the sweep on the device: ESC_wave_pc[_temp](bands=)
is the pca_hip.frame_points_bands call, with_bands(None) is the grid dataset bit for bit, PeakPoints picks its
peaks on the band grid, a d = 128 model trains on the 512-point mel set through the set-resident forward and
resumes bit for bit, and evalsweep.band_sweep is one _dataset_accuracy pass per bank."""
import json

import numpy as np
import pytest
import torch

from dispatch import launches
from oracle import st_oracle as orc
from test_gpu_trainer_eval import _net, _resume_case, _state

pytestmark = pytest.mark.gpu

FS = 44100


@pytest.fixture(scope="module")
def dev():
    return torch.device("cuda", 0)


@pytest.fixture(scope="module")
def corpus():
    """test_gpu_frame_points_multires.py's five clips."""
    secs = (0.05, 0.11, 0.2, 0.3667, 0.5)
    clips = [orc.synth_clip(40 + i, 3 * i + 1, seconds=s) for i, s in enumerate(secs)]
    clips[2] = clips[2].copy()
    clips[2][3000:5200] = 0.0
    return clips, np.array([4, 9, 2, 7, 5])


def _bits(t):
    return t.contiguous().view(torch.int32)


@pytest.mark.parametrize("ntemp", [1, 4], ids=["2d", "3d"])
def test_dataset_batch_is_the_ops_call(ntemp, corpus, dev):
    import dataset
    import pca_hip
    clips, y = corpus
    bank = pca_hip.mel_bank(FS, 256, 16)
    kw = dict(jitter=40, gain_db=6.0, win_lengths=(256, 200), norm="win", seed=4, device=dev, bands=bank)
    ds = (dataset.ESC_wave_pc(clips, y, FS, 256, **kw) if ntemp == 1
          else dataset.ESC_wave_pc_temp(clips, y, FS, 256, ntemp, **kw))
    din = 2 if ntemp == 1 else 3
    assert ds.stochastic and ds.F == 16 and ds.num_points == 16 * ntemp
    n = len(ds)
    idx = torch.tensor([0, n - 1, 5, 5, 9, 2, n // 2], device=dev)
    ds._draw = 6
    pts, lab, meta = ds.batch(idx, want_meta=True)
    assert ds._draw == 7 and tuple(pts.shape) == (7, 16 * ntemp, din) and tuple(meta.shape) == (7, 4)
    waves, woff, soff, _, t32, clab = ds._resident()
    f32 = torch.as_tensor(bank.centres / FS).float().to(dev)
    call = dict(max_len=max(len(c) for c in clips), min_len=min(len(c) for c in clips), clip_labels=clab,
                norm_mode=pca_hip.NORM_WIN, seed=4)
    wins = torch.tensor([256, 200], dtype=torch.int32, device=dev)
    want = pca_hip.frame_points_bands(waves, woff, soff, idx, 256, 128, bank, f32, t32, ntemp, jitter=40,
                                      gain_db=6.0, win_lengths=wins, draw=7, want_meta=True, **call)
    assert torch.equal(_bits(pts), _bits(want[0])) and torch.equal(lab, want[1]) and torch.equal(meta, want[2])
    assert torch.equal(pts[0, :16, 0], f32)
    assert torch.equal(lab.cpu(), torch.from_numpy(ds.labels)[idx.cpu()])
    # buffers passed in, as the Trainer passes them
    o2, l2 = torch.full_like(pts, 3.0), torch.zeros(7, dtype=torch.int64, device=dev)
    ds._draw = 6
    ds.batch(idx, out=o2, labels_out=l2)
    assert torch.equal(_bits(o2), _bits(pts)) and torch.equal(l2, lab)
    # plain() keeps the bank and drops the draws
    p = ds.plain()
    assert p.bands is bank and not p.stochastic and p._resident()[0].data_ptr() == waves.data_ptr()
    q1, q2 = p.batch(idx, want_meta=True), p.batch(idx, want_meta=True)
    assert torch.equal(_bits(q1[0]), _bits(q2[0])) and torch.equal(q1[2], q2[2])
    m = q1[2].cpu().numpy()
    assert (m[:, 2] == 256).all() and (m[:, 3] == np.array([1.0], dtype=np.float32).view(np.int32)[0]).all()
    want = pca_hip.frame_points_bands(waves, woff, soff, idx, 256, 128, bank, f32, t32, ntemp,
                                      win_lengths=wins[:1].contiguous(), **call)
    assert torch.equal(_bits(q1[0]), _bits(want[0]))
    # one item goes through batch, to the host
    item, lbl = p[5]
    assert item.device.type == "cpu" and tuple(item.shape) == (16 * ntemp, din)
    assert torch.equal(item, q1[0][2].cpu()) and int(lbl) == int(q1[1][2])


@pytest.mark.parametrize("ntemp", [1, 4], ids=["2d", "3d"])
def test_with_bands_none_is_the_grid_dataset(ntemp, corpus, dev):
    import dataset
    import pca_hip
    clips, y = corpus
    kw = dict(jitter=40, gain_db=6.0, win_lengths=(256, 200), seed=4, device=dev)
    make = (lambda **k: dataset.ESC_wave_pc(clips, y, FS, 256, **kw, **k)) if ntemp == 1 else \
        (lambda **k: dataset.ESC_wave_pc_temp(clips, y, FS, 256, ntemp, **kw, **k))
    grid = make()
    band = make(bands=pca_hip.mel_bank(FS, 256, 16))
    idx = torch.arange(0, len(grid), 3, device=dev)
    band._draw = 2
    band.batch(idx)                       # the band view is the first to touch the shared store
    back = band.with_bands(None)
    assert back._draw == 3 and back._store is band._store
    grid._draw = 3
    a, b = back.batch(idx, want_meta=True), grid.batch(idx, want_meta=True)
    assert a[0].shape == b[0].shape == (idx.numel(), grid.num_points, 2 if ntemp == 1 else 3)
    assert torch.equal(_bits(a[0]), _bits(b[0])) and torch.equal(a[1], b[1]) and torch.equal(a[2], b[2])
    # and back again: two banks over one resident corpus
    again = back.with_bands(pca_hip.mel_bank(FS, 256, 8))
    assert again.batch(idx)[0].shape[1] == 8 * ntemp and band.batch(idx)[0].shape[1] == 16 * ntemp


def test_peak_points_over_a_band_dataset(corpus, dev):
    import dataset
    import pca_hip
    clips, y = corpus
    bank = pca_hip.mel_bank(FS, 256, 24, htk=True)
    ds = dataset.ESC_wave_pc_temp(clips, y, FS, 256, 4, jitter=20, gain_db=3.0, seed=2, device=dev, bands=bank)
    peaks = dataset.PeakPoints(ds, 12, radius_f=1, radius_t=1, rel_floor=8.0)
    assert (peaks.F, peaks.Nt, peaks.din) == (24, 4, 3) and peaks.num_points == 12 and peaks.stochastic
    idx = torch.arange(0, len(ds), 2, device=dev)
    ds._draw = 4
    got = peaks.batch(idx)
    ds._draw = 4
    dense, lab = ds.batch(idx)
    want = pca_hip.peak_points(dense, 24, 4, 12, radius_f=1, radius_t=1, rel_floor=8.0)
    assert torch.equal(_bits(got[0]), _bits(want[0])) and torch.equal(got[-1], want[1])
    assert torch.equal(got[1], lab) and int(got[-1].min()) >= 1 and int(got[-1].max()) <= 12
    assert peaks.plain().inner.bands is bank


# ---- through the Trainer: the 512-point mel set on the set-resident forward -------------------------------
@pytest.mark.parametrize("graph", [True, False], ids=["hipgraph", "eager"])
def test_trainer_steps_on_the_mel_set_and_resumes(dev, tmp_path, graph):
    import dataset
    import pca_hip
    from pca_hip import _lib, trainer
    B, N = 8, 512
    lengths, y = [10000, 20300, 16200, 22300], [1, 8, 3, 6]               # 5 + 10 + 8 + 11 = 34 sets
    clips = [orc.synth_clip(90 + i, 2 * i, seconds=n / FS + 0.01)[:n] for i, n in enumerate(lengths)]
    assert [len(c) for c in clips] == lengths

    def make():
        d = dataset.ESC_wave_pc_temp(clips, y, FS, 512, 8, jitter=64, gain_db=6.0, seed=9, device=dev,
                                     bands=pca_hip.mel_bank(FS, 512, 64))
        assert len(d) == 34 and d.num_points == N and d.F == 64 and d.stochastic   # 4 steps per epoch
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
    want = _state(tr)
    assert torch.isfinite(want[0]).all() and all(np.isfinite(losses)) and len(set(losses)) == 3, losses
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
    # the step on this set runs the set-resident forward: one k_set128_fwd launch
    eng = trainer.STEngine(net, B, N, _lib.MODE_BF16, training=True)
    assert launches(lambda: eng.fwd_bwd(X, lab), ("set_fwd",))["set_fwd"] == 1
    # 6 steps straight = 3 steps + checkpoint + a fresh Trainer + 3 steps, bitwise
    _resume_case(make, 3, tmp_path, graph=graph)
    r = trainer.Evaluator(net, ds.plain(), 16, _lib.MODE_BF16).run()
    assert r["n"] == 34 and np.isfinite(r["loss"])


# ---- the sweep --------------------------------------------------------------------------------------------
def test_band_sweep(corpus, dev, tmp_path):
    import dataset
    import evalsweep
    import models
    import pca_hip
    clips, y = corpus
    clips = [torch.from_numpy(c).to(dev) for c in clips[:3]]
    y = y[:3]
    torch.manual_seed(11)
    net = models.ST(dim_input=3, num_outputs=1, dim_output=10, num_inds=4, dim_hidden=16,
                    num_heads=4).to(dev).eval()
    path = str(tmp_path / "bands.json")
    out = evalsweep.band_sweep(net, clips, y, FS, 256, [8, 16, 24], Ntemp=4, batch_size=8, json_file=path,
                               sets_per_call=6, htk=True)
    assert sorted(out) == ["banks", "data", "list_banks"]
    assert list(out["data"]) == out["list_banks"] == ["8", "16", "24"]
    banks = [pca_hip.mel_bank(FS, 256, n, htk=True) for n in (8, 16, 24)]
    assert out["banks"] == [dict(n_bands=b.n_bands, power=2, amin=1e-8, nnz=b.nnz) for b in banks]
    back = json.load(open(path))
    assert back == json.loads(json.dumps(out))
    acc = lambda d: evalsweep._dataset_accuracy(net, d, None, 3, 8, evalsweep._lib.MODE_F32, 6)  # noqa: E731
    for name, b in zip(out["list_banks"], banks):
        ds = dataset.ESC_wave_pc_temp(clips, y, FS, 256, 4, device=dev, bands=b)
        assert len(ds) >= 8
        assert out["data"][name] == [acc(ds), 0]
    assert all(0.0 <= v[0] <= 1.0 for v in out["data"].values())
    # banks of the caller's own, by name; 2-D sets
    net2 = models.ST(dim_input=2, num_outputs=1, dim_output=10, num_inds=4, dim_hidden=16,
                     num_heads=4).to(dev).eval()
    own = {"mel16": banks[1], "flat": pca_hip.FilterBank(np.eye(129)[:64], np.arange(64) * 100.0, power=1)}
    out = evalsweep.band_sweep(net2, clips, y, FS, 256, own, batch_size=8, sets_per_call=6)
    assert out["list_banks"] == ["mel16", "flat"] and out["banks"][1]["n_bands"] == 64
    ds = dataset.ESC_wave_pc(clips, y, FS, 256, device=dev, bands=own["flat"])
    assert out["data"]["flat"] == [evalsweep._dataset_accuracy(net2, ds, None, 2, 8, evalsweep._lib.MODE_F32, 6), 0]
