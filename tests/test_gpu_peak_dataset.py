"""dataset.PeakPoints, the engine and the Trainer on peak sets, and evalsweep.peak_sweep, on the device.

The view is checked as a composition: its batch is pca_hip.peak_points of the inner dataset's batch of the
same draw, bit for bit.  The engine on a padded peak batch is held to the bar of tests/test_gpu_varlen.py
(mask == truncation) against the forward of each set's own rows.  Trainer steps over the view are compared
with the same steps issued by hand, bitwise, at the bf16 d = 128 step that tests/test_gpu_trainer_eval.py
holds to bitwise resume."""
import numpy as np
import pytest
import torch

from oracle import st_oracle as orc
from test_gpu_trainer_eval import _net, _same_bits, _state
from util import close

pytestmark = pytest.mark.gpu

FS, N_FFT = 44100, 128


@pytest.fixture(scope="module")
def dev():
    return torch.device("cuda", 0)


def _clips():
    return [orc.synth_clip(70 + i, 3 * i + 1, seconds=n / FS)[:n] for i, n in enumerate((2000, 2100, 1950))]


LABELS = np.array([3, 8, 5])
AUG = dict(jitter=20, gain_db=6.0, win_lengths=(128, 96), freq_masks=1, freq_mask_width=6, mask_mode="floor")


def _wave(dev, ntemp=1, **kw):
    import dataset
    if ntemp == 1:
        return dataset.ESC_wave_pc(_clips(), LABELS, FS, N_FFT, seed=4, device=dev, **kw)
    return dataset.ESC_wave_pc_temp(_clips(), LABELS, FS, N_FFT, ntemp, seed=4, device=dev, **kw)


def _spectra(dev, ntemp):
    """(x, labels, farr, tarr): the log-magnitude spectra of the clips, [F, T] frames or [F, Nt, S] chunks."""
    w = _wave(dev, ntemp)
    X, lab = w.batch(torch.arange(len(w), device=dev))[:2]
    v = X[:, :, -1].cpu().numpy()
    if ntemp == 1:
        return v.T.copy(), lab.cpu().numpy(), w.farr, None
    return v.reshape(len(w), ntemp, w.F).transpose(2, 1, 0).copy(), lab.cpu().numpy(), w.farr, w.tarr


def _inner(kind, dev):
    """A fresh inner dataset of ``kind`` and the peak radii the view is built with."""
    import dataset
    if kind == "pc":
        x, y, farr, _ = _spectra(dev, 1)
        return dataset.ESC_pc(x, y, farr, device=dev), (2, 0)
    if kind == "pc_temp":
        x, y, farr, tarr = _spectra(dev, 4)
        ntv = np.random.default_rng(3).integers(1, 5, size=x.shape[2]).astype(np.int32)
        ntv[:2] = (4, 1)
        return dataset.ESC_pc_temp(x, y, farr, tarr, device=dev, nt_valid=ntv), (2, 1)
    if kind == "wave":
        return _wave(dev, 1, **AUG), (1, 0)
    return _wave(dev, 4, time_masks=1, time_mask_width=1, **AUG), (1, 1)


def _bits(t):
    return t.contiguous().view(torch.int32)


@pytest.mark.parametrize("kind", ["pc", "pc_temp", "wave", "wave_temp"])
def test_view_is_peak_points_of_the_inner_batch(kind, dev):
    import dataset
    import pca_hip
    inner, (rf, rt) = _inner(kind, dev)
    K = 12
    view = dataset.PeakPoints(inner, K, radius_f=rf, radius_t=rt, rel_floor=9.0)
    assert view.variable_length and view.num_points == K and view.batch_seq is None
    assert len(view) == len(inner) and view.stochastic == bool(getattr(inner, "stochastic", False))
    assert not view.soft_targets
    idx = torch.tensor([0, len(inner) - 1, 5, 5, 9, 2, 17], device=dev)
    if view.stochastic:
        view._draw = 6
        assert inner._draw == 6
    out, lab, sel, count, lens = view.batch(idx, want_sel=True, want_count=True)
    assert tuple(out.shape) == (7, K, view.din) and lens.dtype == torch.int32
    other, _ = _inner(kind, dev)
    if view.stochastic:
        assert view._draw == 7
        other._draw = 6
    res = other.batch(idx)
    ln_in = res[2] if getattr(other, "variable_length", False) else None
    want = pca_hip.peak_points(res[0], view.F, view.Nt, K, rf, rt, rel_floor=9.0, lengths=ln_in,
                               want_sel=True, want_count=True)
    assert torch.equal(_bits(out), _bits(want[0])) and torch.equal(lens, want[1])
    assert torch.equal(sel, want[2]) and torch.equal(count, want[3]) and torch.equal(lab, res[1])
    assert int(lens.min()) >= 1 and int(count.max()) > 0
    beyond = torch.arange(K, device=dev)[None, :] >= lens[:, None]
    assert (_bits(out)[beyond] == 0).all()
    if kind == "pc_temp":                       # nothing beyond a chunk's own frames is a peak
        assert (sel.max(1).values < ln_in).all()
    # buffers passed in, as the Trainer and the Evaluator pass them
    if view.stochastic:
        view._draw = 6
    o2 = torch.full((7, K, view.din), 3.0, device=dev)
    l2 = torch.zeros(7, dtype=torch.int64, device=dev)
    n2 = torch.zeros(7, dtype=torch.int32, device=dev)
    view.batch(idx, out=o2, labels_out=l2, lengths_out=n2)
    assert torch.equal(_bits(o2), _bits(out)) and torch.equal(l2, lab) and torch.equal(n2, lens)
    # the plain view is deterministic
    p = view.plain()
    assert not p.stochastic and p.num_points == K and p.variable_length
    a, b = p.batch(idx), p.batch(idx)
    assert torch.equal(_bits(a[0]), _bits(b[0])) and torch.equal(a[-1], b[-1])
    if view.stochastic:
        assert not torch.equal(_bits(a[0]), _bits(out))
    # one item: the un-padded rows
    pts, lbl = p[5]
    assert tuple(pts.shape) == (int(a[-1][2]), view.din) and int(lbl) == int(a[1][2])
    assert torch.equal(pts, a[0][2, :pts.shape[0]].cpu())


def test_view_refuses_what_has_no_grid(dev):
    import dataset
    with pytest.raises(ValueError, match="drop"):
        dataset.PeakPoints(_wave(dev, 1, freq_masks=1, freq_mask_width=4, mask_mode="drop"), 8)
    dataset.PeakPoints(_wave(dev, 1, freq_masks=1, freq_mask_width=4, mask_mode="floor"), 8)
    x, y, farr, tarr = _spectra(dev, 4)
    with pytest.raises(TypeError):
        dataset.PeakPoints(dataset.ESC_pc_temp_maxKSS(x, y, farr, tarr, 10, device=dev), 8)
    inner = dataset.ESC_pc_temp(x, y, farr, tarr, device=dev)
    with pytest.raises(ValueError):
        dataset.PeakPoints(inner, 8, radius_f=0)
    with pytest.raises(ValueError):
        dataset.PeakPoints(inner, 64 * 4 + 1)


def test_engine_on_a_peak_batch_equals_the_sets_alone(dev):
    """tests/test_gpu_varlen.py's tiny_f32 architecture and its fp32 bar, 2e-4."""
    import dataset
    import models
    from pca_hip import _lib
    from pca_hip.trainer import STEngine
    inner, _ = _inner("pc", dev)
    K = 24
    view = dataset.PeakPoints(inner, K, radius_f=2)
    torch.manual_seed(5)
    net = models.ST(dim_input=2, num_outputs=1, dim_output=10, num_inds=4, dim_hidden=16, num_heads=4).to(dev)
    idx = torch.tensor([1, 30, 50, 95], device=dev)
    X, _, lens = view.batch(idx)
    n = lens.cpu().tolist()
    assert min(n) < K and len(set(n)) > 1, n
    got = STEngine(net, 4, K, _lib.MODE_F32, training=False).forward(X, lens).clone()
    for b in range(4):
        alone = STEngine(net, 1, n[b], _lib.MODE_F32, training=False).forward(X[b:b + 1, :n[b]].contiguous())
        close(got[b:b + 1], alone, 2e-4, f"set {b} of {n[b]} peaks")


@pytest.mark.parametrize("graph", [True, False], ids=["hipgraph", "eager"])
def test_trainer_steps_are_the_steps_issued_by_hand(dev, graph):
    import dataset
    from pca_hip import _lib, trainer
    # the corpus, batch and model of tests/test_gpu_point_mask.py's Trainer test (n_fft 128, Ntemp 4: 256 points
    # a set, 70 sets), reduced to the 100 strongest peaks of each set: B = 16, N = 100, bf16, d = 128
    B, K = 16, 100
    opts = dict(batch_size=B, mode=_lib.MODE_BF16, seed=5)
    clips = [orc.synth_clip(90 + i, 2 * i, seconds=n / FS)[:n] for i, n in enumerate((3000, 5200, 4100, 6000))]

    def make():
        inner = dataset.ESC_wave_pc_temp(clips, [1, 8, 3, 6], FS, N_FFT, 4, seed=9, device=dev,
                                         time_masks=1, time_mask_width=1, **AUG)
        ds = dataset.PeakPoints(inner, K, radius_f=1)
        assert ds.stochastic and len(ds) == 70                            # 4 steps per epoch
        return _net(dev, 3, seed=4), ds

    net, ds = make()
    tr = trainer.Trainer(net, ds, use_graph=graph, **opts)
    assert tr.lengths is not None and tr.N == K and not tr._cursor_mode
    losses, sizes = [], []
    for _ in range(3):
        tr.step()
        torch.cuda.synchronize()
        losses.append(float(tr.eng.loss))
        sizes.append(tr.lengths.clone())
    want = _state(tr)
    assert torch.isfinite(want[0]).all() and all(np.isfinite(losses))
    assert not torch.equal(sizes[0], sizes[1])                            # other sets, other counts

    # by hand: ds.batch -> STEngine.fwd_bwd(lengths=) -> Adam
    net, ds = make()
    eng = trainer.STEngine(net, B, K, _lib.MODE_BF16, training=True)
    n = eng.flat.numel()
    m, v = torch.zeros(n, device=dev), torch.zeros(n, device=dev)
    step_count = torch.zeros(2, dtype=torch.int32, device=dev)
    X = torch.empty((B, K, 3), device=dev)
    lab = torch.zeros(B, dtype=torch.int64, device=dev)
    lens = torch.zeros(B, dtype=torch.int32, device=dev)
    stream = trainer.ShardedIndexStream(len(ds), B, 0, 1, 5, True, dev)
    for s in range(3):
        if graph:                  # a captured step froze the host draw number of its recorded call, the 2nd
            ds._draw = 1
        ds.batch(stream.next().clone(), out=X, labels_out=lab, lengths_out=lens, draw_dev=step_count)
        eng.fwd_bwd(X, lab, lengths=lens)
        _lib.check(_lib.lib().pca_adam_step(eng.flat.data_ptr(), eng.grads.data_ptr(), m.data_ptr(),
                                            v.data_ptr(), n, 1e-3, 0.9, 0.999, 1e-8, 1e-3, 1.0,
                                            step_count.data_ptr(), 1, eng._stream()), "pca_adam_step")
        torch.cuda.synchronize()
        assert float(eng.loss) == losses[s], (s, float(eng.loss), losses[s])
        assert torch.equal(lens, sizes[s])
    _same_bits((eng.flat, m, v, step_count), want)

    # save after step 1, resume in a new Trainer on a new model and dataset: the uninterrupted run
    net, ds = make()
    first = trainer.Trainer(net, ds, use_graph=graph, **opts)
    first.step()
    state = first.state_dict()
    assert state["draw"] == ds._draw == ds.inner._draw
    del first
    net, ds = make()
    with torch.no_grad():
        for p in net.parameters():
            p.add_(1.0)
    second = trainer.Trainer(net, ds, use_graph=graph, **opts)
    second.load_state_dict(state)
    for _ in range(2):
        second.step()
    _same_bits(_state(second), want)
    # the held-out pass takes the plain view
    r = trainer.Evaluator(net, ds.plain(), 32, _lib.MODE_BF16).run()
    assert r["n"] == 70 and np.isfinite(r["loss"])


@pytest.mark.parametrize("tag", ["fst", "tst"])
def test_peak_sweep_is_the_composition(dev, tag, tmp_path):
    import json

    import evalsweep
    import models
    import pca_hip
    from pca_hip import _lib
    from pca_hip.trainer import STEngine
    x, y, farr, tarr = _spectra(dev, 1 if tag == "fst" else 4)
    x, y = x[..., :19], y[:19]                                  # 16 of them count at batch_size 8
    F, Nt, din = x.shape[0], (1 if tarr is None else x.shape[1]), (2 if tarr is None else 3)
    torch.manual_seed(11)
    net = models.ST(dim_input=din, num_outputs=1, dim_output=10, num_inds=4, dim_hidden=16,
                    num_heads=4).to(dev).eval()
    list_K, cap, spec = [1, 7, 40], 6, dict(radius_f=2, radius_t=0 if tarr is None else 1, rel_floor=12.0)
    path = str(tmp_path / "peaks.json")
    out = evalsweep.peak_sweep(net, x, y, farr, tarr, list_K=list_K, sets_per_call=cap, json_file=path,
                               **spec)
    assert out["list_K"] == list_K and sorted(out["data"]) == sorted(out["mean_points"]) == list_K
    back = json.load(open(path))
    assert {int(k): v for k, v in back["data"].items()} == {k: list(v) for k, v in out["data"].items()}
    assert {int(k): v for k, v in back["mean_points"].items()} == out["mean_points"]
    xs, lab, f32, t32 = evalsweep._resident_sets(x, y, farr, tarr, dev)
    full = 16
    for K in list_K:
        correct = points = 0
        for p0 in range(0, full, cap):
            b = min(cap, full - p0)
            Xf = torch.empty((b, F * Nt, din), dtype=torch.float32, device=dev)
            evalsweep._pack_sets(xs, f32, t32, torch.arange(p0, p0 + b, device=dev), Xf)
            sub, lens = pca_hip.peak_points(Xf, F, Nt, K, **spec)
            logits = STEngine(net, b, K, _lib.MODE_F32, training=False).forward(sub, lens)
            correct += int((logits.argmax(1) == lab[p0:p0 + b]).sum())
            points += int(lens.sum())
        assert out["data"][K] == [correct / full, 0], (tag, K, out["data"][K], correct)
        assert out["mean_points"][K] == points / full
    mp = out["mean_points"]
    assert mp[1] == 1.0 and 1.0 < mp[7] <= 7.0 and mp[7] <= mp[40] <= 40.0
    # the default grid ends at the most peaks a set can hold
    assert evalsweep.most_peaks(F, Nt) == (F - 1) // 2 * Nt
    assert evalsweep.default_list_K(evalsweep.most_peaks(F, Nt))[-1] == (F - 1) // 2 * Nt
