"""The ``reassign`` switch of dataset.ESC_wave_pc / ESC_wave_pc_temp on the device: batches are the
binding's output, the Trainer steps and resumes on them, PeakPoints picks from them, and
evalsweep.reassign_sweep slides from the grid to the reassigned sets."""
import json

import numpy as np
import pytest
import torch

from oracle import st_oracle as orc
from test_gpu_trainer_eval import _net, _resume_case

pytestmark = pytest.mark.gpu

FS, N_FFT = 44100, 128
LABELS = np.array([3, 8, 5])
AUG = dict(jitter=20, gain_db=6.0, win_lengths=(128, 96), seed=4)


@pytest.fixture(scope="module")
def dev():
    return torch.device("cuda", 0)


def _clips():
    return [orc.synth_clip(70 + i, 3 * i + 1, seconds=n / FS)[:n] for i, n in enumerate((2000, 2100, 1950))]


def _bits(t):
    return t.contiguous().view(torch.int32)


def _binding(ds, idx, draw, **spec):
    """pca_hip.frame_points_reassigned with the dataset's own resident tensors and settings."""
    import pca_hip
    waves, woff, soff, f32, t32, lab = ds._resident()
    return pca_hip.frame_points_reassigned(
        waves, woff, soff, idx, ds.n_fft, ds.hop, ds.F, f32, t32, ds._ntemp, max_len=ds._max_len,
        min_len=ds._min_len, clip_labels=lab, jitter=ds.jitter, gain_db=ds.gain_db,
        win_lengths=torch.tensor(ds.win_lengths, dtype=torch.int32, device=waves.device),
        norm_mode=pca_hip.NORM_WIN if ds.norm == "win" else pca_hip.NORM_NFFT, seed=ds.seed, draw=draw,
        want_meta=True, **spec)


@pytest.mark.parametrize("ntemp", [1, 4], ids=["din2", "din3"])
def test_batches_are_the_binding(ntemp, dev):
    import dataset
    if ntemp == 1:
        ds = dataset.ESC_wave_pc(_clips(), LABELS, FS, N_FFT, device=dev, reassign=True, **AUG)
        spec = dict(axes="f")
    else:
        spec = dict(axes="ft", rel_floor=5.0, max_df=1.5, max_dt=0.75, strength=0.5)
        ds = dataset.ESC_wave_pc_temp(_clips(), LABELS, FS, N_FFT, ntemp, norm="win", device=dev,
                                      reassign=dict(spec), **AUG)
    assert ds.stochastic and not ds.variable_length and ds.batch_seq is None
    n = len(ds)
    idx = torch.tensor([0, n - 1, 5, 5, 9, 2, n // 2], device=dev)
    ds._draw = 6
    pts, lab, meta = ds.batch(idx, want_meta=True)
    assert ds._draw == 7 and tuple(pts.shape) == (7, ds.num_points, 2 if ntemp == 1 else 3)
    want = _binding(ds, idx, 7, **spec)
    assert torch.equal(_bits(pts), _bits(want[0])) and torch.equal(lab, want[1]) and torch.equal(meta, want[2])
    # the grid view: bit for bit the dataset without the switch
    grid = ds.with_reassign(None)
    assert grid.reassign is None and grid._resident()[0].data_ptr() == ds._resident()[0].data_ptr()
    other = (dataset.ESC_wave_pc(_clips(), LABELS, FS, N_FFT, device=dev, **AUG) if ntemp == 1 else
             dataset.ESC_wave_pc_temp(_clips(), LABELS, FS, N_FFT, ntemp, norm="win", device=dev, **AUG))
    grid._draw = other._draw = 6
    a, b = grid.batch(idx), other.batch(idx)
    assert torch.equal(_bits(a[0]), _bits(b[0])) and torch.equal(a[1], b[1])
    assert torch.equal(_bits(a[0][:, :, -1]), _bits(pts[:, :, -1]))             # the same values
    assert not torch.equal(_bits(a[0][:, :, 0]), _bits(pts[:, :, 0]))           # other coordinates
    # plain(): augmentations off, the representation kept
    p = ds.plain()
    assert p.reassign == ds.reassign and not p.stochastic
    q1, q2 = p.batch(idx), p.batch(idx)
    assert torch.equal(_bits(q1[0]), _bits(q2[0]))
    assert not torch.equal(_bits(q1[0][:, :, 0]), _bits(grid.plain().batch(idx)[0][:, :, 0]))
    # buffers passed in, as the Trainer passes them; one item goes through batch
    o2 = torch.full_like(pts, 3.0)
    l2 = torch.zeros(7, dtype=torch.int64, device=dev)
    ds._draw = 6
    ds.batch(idx, out=o2, labels_out=l2)
    assert torch.equal(_bits(o2), _bits(pts)) and torch.equal(l2, lab)
    item, lbl = p[5]
    assert torch.equal(item, q1[0][2].cpu()) and int(lbl) == int(q1[1][2])
    # what the switch does not combine with
    for kw in (dict(speeds=(1.0, 1.1)), dict(mix_clips="self", mix_prob=0.5),
               dict(freq_masks=1, freq_mask_width=4)):
        with pytest.raises(ValueError, match="reassign"):
            dataset.ESC_wave_pc(_clips(), LABELS, FS, N_FFT, device=dev, reassign=True, **kw)


@pytest.mark.parametrize("graph", [True, False], ids=["hipgraph", "eager"])
def test_trainer_steps_and_resumes(dev, tmp_path, graph):
    """The corpus, batch and net of tests/test_gpu_frame_points.py's Trainer test (n_fft 512: N = 256, B = 16,
    bf16, d = 128) with the points reassigned."""
    import dataset
    from pca_hip import _lib, trainer
    lengths, y = [3000, 5200, 4100, 6000], [1, 8, 3, 6]
    clips = [orc.synth_clip(90 + i, 2 * i, seconds=n / FS)[:n] for i, n in enumerate(lengths)]

    def make(reassign=True):
        d = dataset.ESC_wave_pc(clips, y, FS, 512, drop_nyquist=True, jitter=64, gain_db=6.0, seed=9,
                                device=dev, reassign=reassign)
        assert len(d) == 74 and d.num_points == 256                       # 4 steps per epoch
        return _net(dev, 2, seed=4), d, dict(seed=5, batch_size=16, mode=_lib.MODE_BF16)

    net, ds, kw = make()
    tr = trainer.Trainer(net, ds, use_graph=graph, **kw)
    losses, batches = [], []
    for _ in range(3):
        tr.step()
        torch.cuda.synchronize()
        losses.append(float(tr.eng.loss))
        batches.append(tr.X.clone())
    assert all(np.isfinite(losses)) and len(set(losses)) == 3, losses
    assert torch.isfinite(tr.eng.flat).all()
    F = ds.F
    farr = ds._resident()[3]
    assert not torch.equal(batches[0][:, :, 0], farr.expand(16, F))       # the step saw moved points
    # the grid dataset takes another path through the same steps
    net, grid, kw = make(reassign=None)
    tg = trainer.Trainer(net, grid, use_graph=graph, **kw)
    tg.step()
    torch.cuda.synchronize()
    assert torch.equal(tg.X[:, :, 0], farr.expand(16, F)) and float(tg.eng.loss) != losses[0]
    assert torch.equal(_bits(tg.X[:, :, 1]), _bits(batches[0][:, :, 1]))  # the same draws, the same values

    _resume_case(make, 3, tmp_path, graph=graph)
    r = trainer.Evaluator(net, ds.plain(), 16, _lib.MODE_BF16).run()
    assert r["n"] == 74 and np.isfinite(r["loss"])


@pytest.mark.parametrize("ntemp", [1, 4], ids=["din2", "din3"])
def test_peaks_over_a_reassigned_dataset(ntemp, dev):
    import dataset
    mk = (lambda: dataset.ESC_wave_pc(_clips(), LABELS, FS, N_FFT, device=dev, reassign=True, **AUG)) \
        if ntemp == 1 else \
        (lambda: dataset.ESC_wave_pc_temp(_clips(), LABELS, FS, N_FFT, ntemp, device=dev, reassign=True, **AUG))
    inner, other = mk(), mk()
    K = 12
    view = dataset.PeakPoints(inner, K, radius_f=2, rel_floor=9.0, refine=False)
    idx = torch.tensor([0, len(inner) - 1, 5, 5, 9, 2], device=dev)
    view._draw = other._draw = 6
    out, lab, sel, lens = view.batch(idx, want_sel=True)
    rows, want_lab = other.batch(idx)
    assert torch.equal(lab, want_lab) and int(lens.min()) >= 1
    grid_f = other._resident()[3]
    moved_rows = 0
    for b in range(idx.numel()):
        n = int(lens[b])
        s = sel[b, :n].long()
        assert torch.equal(_bits(out[b, :n]), _bits(rows[b, s]))          # the reassigned rows at sel
        assert not out[b, n:].any() and (sel[b, n:] == -1).all()
        moved_rows += int((out[b, :n, 0] != grid_f[s % inner.F]).sum())
    assert moved_rows > 0                                                 # peaks carry energy: they moved


@pytest.mark.parametrize("ntemp", [None, 4], ids=["fst", "tst"])
def test_reassign_sweep(ntemp, dev, tmp_path):
    import dataset
    import evalsweep
    import models
    clips = [torch.from_numpy(c).to(dev) for c in _clips()]
    din = 2 if ntemp is None else 3
    torch.manual_seed(11)
    net = models.ST(dim_input=din, num_outputs=1, dim_output=10, num_inds=4, dim_hidden=16,
                    num_heads=4).to(dev).eval()
    path = str(tmp_path / "reassign.json")
    strengths = (0, 0.5, 1)
    out = evalsweep.reassign_sweep(net, clips, LABELS, FS, N_FFT, Ntemp=ntemp, list_strength=strengths,
                                   batch_size=8, json_file=path, sets_per_call=6, max_df=1.5)
    assert out["list_strength"] == [0.0, 0.5, 1.0] and sorted(out["data"]) == [0.0, 0.5, 1.0]
    assert out["spec"]["max_df"] == 1.5 and out["spec"]["axes"] == ("f" if ntemp is None else "ft")
    back = json.load(open(path))
    assert len(back["data"]) == 3
    assert {float(k): v for k, v in back["data"].items()} == {k: list(v) for k, v in out["data"].items()}
    # strength 0 is the grid dataset, exactly; every entry is one _dataset_accuracy pass over a view
    grid = (dataset.ESC_wave_pc(clips, LABELS, FS, N_FFT, device=dev) if ntemp is None else
            dataset.ESC_wave_pc_temp(clips, LABELS, FS, N_FFT, ntemp, device=dev))
    assert len(grid) >= 8
    acc = lambda d: evalsweep._dataset_accuracy(net, d, None, din, 8, evalsweep._lib.MODE_F32, 6)  # noqa: E731
    assert out["data"][0.0] == [acc(grid), 0]
    for s in (0.5, 1.0):
        assert out["data"][s] == [acc(grid.with_reassign(dict(max_df=1.5, strength=s))), 0]
    assert all(0.0 <= v[0] <= 1.0 for v in out["data"].values())
    with pytest.raises(ValueError):
        evalsweep.reassign_sweep(net, clips, LABELS, FS, N_FFT, Ntemp=ntemp, strength=0.5)
