"""pca_frame_points / dataset.ESC_wave_pc / ESC_wave_pc_temp on the device: with the augmentation off
the batches are those of the spectrogram pipeline bit for bit; with it on every frame is the numpy
restatement (tests/frame_ref.py) of what ``meta`` says was cut; the draws are uniform, reproducible and
advance per replay of a captured training step."""
import numpy as np
import pytest
import torch

from frame_ref import frame_ref
from oracle import st_oracle as orc
from test_gpu_trainer_eval import _net, _resume_case, _state

pytestmark = pytest.mark.gpu

FS = 44100
TOL = 5e-5          # test_stft_logmag_vs_oracle's bar: the same fp64 arithmetic on both sides


@pytest.fixture(scope="module")
def dev():
    return torch.device("cuda", 0)


@pytest.fixture(scope="module")
def corpus():
    """Five clips of 0.05 .. 0.5 s, one with a stretch of exact zeros; one label per clip."""
    secs = (0.05, 0.11, 0.2, 0.3667, 0.5)
    clips = [orc.synth_clip(40 + i, 3 * i + 1, seconds=s) for i, s in enumerate(secs)]
    clips[2] = clips[2].copy()
    clips[2][3000:5200] = 0.0
    assert len({len(c) for c in clips}) == 5
    return clips, np.array([4, 9, 2, 7, 5])


def _shuffled_with_repeats(n, seed, dev):
    rng = np.random.Generator(np.random.PCG64(seed))
    idx = np.concatenate([rng.permutation(n), rng.integers(0, n, size=max(8, n // 10))])
    return torch.from_numpy(idx).to(dev)


def _spectrogram_2d(clips, y, n_fft, win, drop, dev):
    """The existing pipeline: one STFT pre-pass, then ESC_pc over the resident spectrogram."""
    import dataset
    import pca_hip
    waves = [torch.from_numpy(c).to(dev) for c in clips]
    spec, foff = pca_hip.stft_logmag_batch(waves, n_fft, win, n_fft // 2, drop_nyquist=drop,
                                           frame_major=True)
    F = spec.shape[1]
    lab = torch.from_numpy(np.repeat(y, np.diff(foff))).to(dev)
    return dataset.ESC_pc.from_device(spec, lab, np.linspace(0, FS / 2, F) / FS), spec, foff


def _spectrogram_3d(clips, y, n_fft, win, ntemp, dev):
    import dataset
    _, spec, foff = _spectrogram_2d(clips, y, n_fft, win, True, dev)
    spec = spec.cpu().numpy()
    chunks = [orc.chunk_frames(spec[foff[c]:foff[c + 1]].T, ntemp) for c in range(len(clips))]
    per = [c.shape[2] for c in chunks]
    assert any((foff[c + 1] - foff[c]) % ntemp for c in range(len(clips)))      # a dropped tail
    F = n_fft // 2
    return dataset.ESC_pc_temp(np.concatenate(chunks, axis=2), np.repeat(y, per),
                               np.linspace(0, FS / 2, F) / FS,
                               np.linspace(0, (n_fft // 2 / FS) * ntemp, ntemp), device=dev)


# ---- 1. augmentation off = the existing pipeline, bit for bit -------------------------------------------
@pytest.mark.parametrize("n_fft,win,drop", [(64, 64, False), (256, 200, False), (1024, 1024, True)])
def test_off_equals_spectrogram_pipeline_2d(n_fft, win, drop, corpus, dev):
    import dataset
    clips, y = corpus
    ds = dataset.ESC_wave_pc(clips, y, FS, n_fft, drop_nyquist=drop, win_lengths=(win,), device=dev)
    ref, _, _ = _spectrogram_2d(clips, y, n_fft, win, drop, dev)
    assert len(ds) == len(ref) and ds.num_points == ref.num_points and not ds.stochastic
    idx = _shuffled_with_repeats(len(ds), 1, dev)
    pts, lab = ds.batch(idx)
    want, want_lab = ref.batch(idx)
    assert pts.shape == want.shape == (idx.numel(), ds.num_points, 2)
    assert torch.equal(pts.view(torch.int32), want.view(torch.int32))
    assert torch.equal(lab, want_lab)
    # __getitem__ goes through batch
    p0, l0 = ds[len(ds) - 1]
    w0, wl0 = ref[len(ds) - 1]
    assert torch.equal(p0, w0) and int(l0) == int(wl0)


@pytest.mark.parametrize("n_fft,win", [(64, 64), (256, 200), (1024, 1024)])
def test_off_equals_spectrogram_pipeline_3d(n_fft, win, corpus, dev):
    import dataset
    clips, y = corpus
    ntemp = 4
    ds = dataset.ESC_wave_pc_temp(clips, y, FS, n_fft, ntemp, win_lengths=(win,), device=dev)
    ref = _spectrogram_3d(clips, y, n_fft, win, ntemp, dev)
    assert len(ds) == len(ref) > 0 and ds.num_points == ref.num_points == ntemp * (n_fft // 2)
    idx = _shuffled_with_repeats(len(ds), 2, dev)
    pts, lab = ds.batch(idx)
    want, want_lab = ref.batch(idx)
    assert pts.shape == want.shape == (idx.numel(), ds.num_points, 3)
    assert torch.equal(pts.view(torch.int32), want.view(torch.int32))
    assert torch.equal(lab, want_lab)


def test_off_equals_spectrogram_pipeline_n_fft_4096(corpus, dev):
    """96 KiB of dynamic LDS: the opt-in above 64 KiB."""
    import dataset
    clips, y = corpus
    clips, y = clips[4:], y[4:]                                          # the 0.5 s clip: 11 frames
    ds = dataset.ESC_wave_pc(clips, y, FS, 4096, device=dev)
    ref, _, _ = _spectrogram_2d(clips, y, 4096, 4096, False, dev)
    assert len(ds) == len(ref) == 11
    idx = torch.tensor([3, 10], device=dev)
    pts, lab = ds.batch(idx)
    want, want_lab = ref.batch(idx)
    assert torch.equal(pts.view(torch.int32), want.view(torch.int32)) and torch.equal(lab, want_lab)


# ---- 2. off the grid, against the CPU restatement -------------------------------------------------------
def _gain(meta_row):
    return np.array([meta_row[3]], dtype=np.int32).view(np.float32)[0]


def _check_against_frame_ref(ds, clips, idx, pts, meta, jitter):
    """Every frame of every slot rebuilt from what ``meta`` reports; returns max |delta|."""
    n_fft, hop, F, Nt = ds.n_fft, ds.hop, ds.F, ds._ntemp
    worst = 0.0
    for b, i in enumerate(idx):
        c, centre0, win, _ = (int(v) for v in meta[b])
        g = _gain(meta[b])
        assert ds.set_off[c] <= i < ds.set_off[c + 1]
        wave, L = clips[c], len(clips[c])
        s = i - ds.set_off[c]
        nominal = s * Nt * hop
        assert max(0, nominal - jitter) <= centre0 <= min(L, nominal + jitter), (b, centre0, nominal)
        assert win in ds.win_lengths
        norm = n_fft if ds.norm == "n_fft" else win
        got = pts[b].reshape(Nt, F, -1)[:, :, -1]

        def err(delta):
            e = 0.0
            for j in range(Nt):
                cj = min(max(nominal + j * hop + delta, 0), L)         # frames hop apart, each clamped
                e = max(e, float(np.abs(got[j] - frame_ref(wave, cj, n_fft, win, g, norm, F)).max()))
            return e

        if centre0 > 0 or nominal > 0 or Nt == 1:
            e = err(centre0 - nominal)
        else:
            # frame 0 sits at the clip's start: the shift it was clamped from is any of [-jitter, 0];
            # one of them must explain the chunk's other frames
            e = min(err(d) for d in range(-jitter, 1))
        worst = max(worst, e)
    return worst


@pytest.mark.parametrize("norm", ["n_fft", "win"])
@pytest.mark.parametrize("ntemp", [1, 3], ids=["din2", "din3"])
def test_augmented_frames_against_numpy(ntemp, norm, corpus, dev):
    import dataset
    clips, y = corpus
    kw = dict(jitter=37, gain_db=6.0, win_lengths=(128, 200, 256), norm=norm, seed=11, device=dev)
    ds = (dataset.ESC_wave_pc(clips, y, FS, 256, **kw) if ntemp == 1
          else dataset.ESC_wave_pc_temp(clips, y, FS, 256, ntemp, **kw))
    assert ds.stochastic
    rng = np.random.Generator(np.random.PCG64(5))
    # sets whose frames, shifted by up to 37 samples, lie wholly inside the zeros [3000, 5200) of clip 2
    zero_sets = [ds.set_off[2] + 3000 // (128 * ntemp) + 2 + k for k in range(4)]
    idx = np.concatenate([ds.set_off[:-1], np.asarray(ds.set_off[1:]) - 1, zero_sets,
                          rng.integers(0, len(ds), size=64 - 14)])         # first and last set of each clip
    assert idx.size == 64
    pts, lab, meta = ds.batch(torch.from_numpy(idx).to(dev), want_meta=True)
    pts, lab, meta = pts.cpu().numpy(), lab.cpu().numpy(), meta.cpu().numpy()
    din = 2 if ntemp == 1 else 3
    assert pts.shape == (64, ntemp * ds.F, din) and np.isfinite(pts).all()
    # coordinates: exactly farr / tarr, point p = t * F + f
    farr = np.asarray(ds.farr, dtype=np.float64).astype(np.float32)
    assert np.array_equal(pts[:, :, 0], np.broadcast_to(np.tile(farr, ntemp), (64, ntemp * ds.F)))
    if ntemp > 1:
        tarr = np.asarray(ds.tarr, dtype=np.float64).astype(np.float32)
        assert np.array_equal(pts[:, :, 1], np.broadcast_to(np.repeat(tarr, ds.F), (64, ntemp * ds.F)))
    assert np.array_equal(lab, y[meta[:, 0]])
    worst = _check_against_frame_ref(ds, clips, idx, pts, meta, 37)
    print(f"frame_points vs numpy, din {din}, norm {norm}: max |delta| {worst:.3e}")
    assert worst < TOL
    # the augmentation did something: shifts, gains and windows all vary over the batch
    assert len({int(m[2]) for m in meta}) == 3 and len({int(m[3]) for m in meta}) > 32
    # and the silent stretch is the floor, scaled by nothing
    silent = pts[2 * len(clips) + 1].reshape(ntemp, ds.F, din)[:, :, -1]
    assert np.abs(silent - np.float32(np.log(np.float32(1e-8)))).max() < TOL


# ---- 3. the draws ---------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def long_clip():
    return [orc.synth_clip(77, 6, seconds=0.5)], np.array([6])


def _draw_ds(long_clip, dev, **kw):
    import dataset
    clips, y = long_clip
    args = dict(jitter=8, gain_db=6.0, win_lengths=(32, 48, 64), seed=21, device=dev)
    args.update(kw)
    return dataset.ESC_wave_pc(clips, y, FS, 64, **args)


def _batch_at(ds, idx, draw, **kw):
    ds._draw = draw - 1                                                  # batch() advances it first
    return ds.batch(idx, want_meta=True, **kw)


def test_draws_are_uniform_and_reproducible(long_clip, dev):
    ds = _draw_ds(long_clip, dev)
    n = len(ds)
    assert n == 690
    slots = 4096
    idx = torch.arange(slots, device=dev) % n
    pts, _, meta = _batch_at(ds, idx, 3)
    m = meta.cpu().numpy()
    nominal = (np.arange(slots) % n) * ds.hop
    delta = m[:, 1] - nominal
    counts = np.bincount(delta + 8, minlength=17)
    print("offset counts", counts.tolist())
    assert counts.size == 17 and counts.min() >= 150 and counts.max() <= 330       # 241 +- 15
    wins = [int((m[:, 2] == w).sum()) for w in (32, 48, 64)]
    print("window counts", wins)
    assert sum(wins) == slots and min(wins) >= 1180 and max(wins) <= 1550          # 1365 +- 30
    gains = m[:, 3].copy().view(np.float32)
    assert gains.min() >= 10 ** -0.3 and gains.max() <= 10 ** 0.3
    below = float((gains < 1).mean())
    print(f"gains below 1: {below:.3f}")
    assert 0.4 <= below <= 0.6
    # the same set in two slots of one call: independent draws
    assert gains[0] != gains[n] and gains[1] != gains[n + 1]
    assert not np.array_equal(m[:n, 1:], m[n:2 * n, 1:])

    bits = lambda t: t.view(torch.int32)                                  # noqa: E731
    again, _, meta2 = _batch_at(ds, idx, 3)
    assert torch.equal(bits(again), bits(pts)) and torch.equal(meta2, meta)
    other, _, meta3 = _batch_at(ds, idx, 4)
    assert not torch.equal(meta3, meta) and not torch.equal(bits(other), bits(pts))
    seeded, _, meta4 = _batch_at(_draw_ds(long_clip, dev, seed=22), idx, 3)
    assert not torch.equal(meta4, meta) and not torch.equal(bits(seeded), bits(pts))
    # the device half of the draw number
    two = torch.tensor([2, 0], dtype=torch.int32, device=dev)
    a, _, ma = _batch_at(ds, idx, 5, draw_dev=two)
    b, _, mb = _batch_at(ds, idx, 7)
    assert torch.equal(bits(a), bits(b)) and torch.equal(ma, mb)


# ---- 4. each field on its own ---------------------------------------------------------------------------
def test_each_field_alone_and_plain(long_clip, corpus, dev):
    import dataset
    n = 690
    idx = torch.arange(1024, device=dev) % n
    nominal = (np.arange(1024) % n) * 32
    one = np.array([1.0], dtype=np.float32).view(np.int32)[0]

    _, _, meta = _draw_ds(long_clip, dev, gain_db=0.0, win_lengths=None).batch(idx, want_meta=True)
    m = meta.cpu().numpy()
    assert (m[:, 3] == one).all() and (m[:, 2] == 64).all()
    assert len(set((m[:, 1] - nominal).tolist())) == 17

    _, _, meta = _draw_ds(long_clip, dev, jitter=0, win_lengths=None).batch(idx, want_meta=True)
    m = meta.cpu().numpy()
    assert np.array_equal(m[:, 1], nominal) and (m[:, 2] == 64).all() and (m[:, 3] != one).any()

    _, _, meta = _draw_ds(long_clip, dev, jitter=0, gain_db=0.0).batch(idx, want_meta=True)
    m = meta.cpu().numpy()
    assert np.array_equal(m[:, 1], nominal) and (m[:, 3] == one).all()
    assert set(m[:, 2].tolist()) == {32, 48, 64}

    off = _draw_ds(long_clip, dev, jitter=0, gain_db=0.0, win_lengths=None)
    assert not off.stochastic
    _, _, meta = off.batch(idx, want_meta=True)
    m = meta.cpu().numpy()
    assert np.array_equal(m[:, 1], nominal) and (m[:, 2] == 64).all() and (m[:, 3] == one).all()

    # plain() of an augmented dataset: the spectrogram pipeline at the nominal window, bit for bit
    clips, y = corpus
    aug = dataset.ESC_wave_pc(clips, y, FS, 256, jitter=37, gain_db=6.0, win_lengths=(200, 128, 256),
                              seed=3, device=dev)
    plain = aug.plain()
    assert aug.stochastic and not plain.stochastic
    assert plain._resident()[0].data_ptr() == aug._resident()[0].data_ptr()          # one resident store
    ref, _, _ = _spectrogram_2d(clips, y, 256, 200, False, dev)
    ids = _shuffled_with_repeats(len(aug), 4, dev)
    pts, lab = plain.batch(ids)
    want, want_lab = ref.batch(ids)
    assert torch.equal(pts.view(torch.int32), want.view(torch.int32)) and torch.equal(lab, want_lab)
    assert not torch.equal(aug.batch(ids)[0], want)


# ---- 5. through the Trainer -----------------------------------------------------------------------------
def _train_clips(lengths):
    return [orc.synth_clip(90 + i, 2 * i, seconds=n / FS)[:n] for i, n in enumerate(lengths)]


@pytest.mark.parametrize("graph", [True, False], ids=["hipgraph", "eager"])
def test_trainer_draws_afresh_resumes_and_evaluates(dev, tmp_path, graph):
    import dataset
    from pca_hip import _lib, trainer
    kw_ds = dict(drop_nyquist=True, jitter=64, gain_db=6.0, device=dev)      # n_fft 512: N = 256
    kw_tr = dict(batch_size=16, mode=_lib.MODE_BF16)

    # (a) one batch of 16 sets, the same indices every step: the packed batch still changes
    clips = _train_clips([4000])
    assert len(clips[0]) == 4000
    ds = dataset.ESC_wave_pc(clips, [3], FS, 512, seed=9, **kw_ds)
    assert len(ds) == 16 and ds.num_points == 256 and ds.stochastic
    tr = trainer.Trainer(_net(dev, 2, seed=4), ds, use_graph=graph, shuffle=False, seed=5, **kw_tr)
    seen = []
    for _ in range(3):
        tr.step()
        torch.cuda.synchronize()
        seen.append((tr.X.clone(), tr.idx.clone()))
    assert torch.equal(seen[0][1], seen[1][1]) and torch.equal(seen[1][1], seen[2][1])
    assert not torch.equal(seen[0][0], seen[1][0]) and not torch.equal(seen[1][0], seen[2][0])
    assert torch.isfinite(tr.eng.flat).all()

    # (b) 6 steps straight = 3 steps + checkpoint + a fresh Trainer + 3 steps, bitwise
    lengths = [3000, 5200, 4100, 6000]                                   # 12 + 21 + 17 + 24 = 74 sets
    y = [1, 8, 3, 6]

    def make(seed=9):
        d = dataset.ESC_wave_pc(_train_clips(lengths), y, FS, 512, seed=seed, **kw_ds)
        assert len(d) == 74                                              # 4 steps per epoch
        return _net(dev, 2, seed=4), d, dict(seed=5, **kw_tr)

    _resume_case(make, 3, tmp_path, graph=graph)

    # (c) the draws matter: another dataset seed ends elsewhere
    net, d, kw = make()
    a = trainer.Trainer(net, d, use_graph=graph, **kw)
    net, d, kw = make(seed=10)
    b = trainer.Trainer(net, d, use_graph=graph, **kw)
    for _ in range(2):
        a.step(); b.step()
    assert not torch.equal(_state(a)[0], _state(b)[0])

    # (d) the held-out pass takes the plain view and is deterministic
    ev = trainer.Evaluator(a.eng.model, d.plain(), 16, _lib.MODE_BF16)
    r1, r2 = ev.run(), ev.run()
    assert r1["n"] == 74 and r1["loss"] == r2["loss"] and r1["acc"] == r2["acc"]
    assert torch.equal(r1["confusion"], r2["confusion"]) and np.isfinite(r1["loss"])
