"""pca_frame_points_reassigned on the device: every coordinate against the numpy restatement
(tests/reassign_ref.py) of what ``meta`` says was cut, the bit identities with pca_frame_points, the
invariants with the floors off, and the device half of the draw number under a captured graph."""
import numpy as np
import pytest
import torch

import reassign_ref
from oracle import st_oracle as orc

pytestmark = pytest.mark.gpu

FS = 44100
SPEC = dict(rel_floor=float(np.log(1e3)), max_df=2.0, max_dt=1.0, strength=1.0)
AUG = dict(jitter=37, gain_db=6.0, seed=11)
CASES = [(64, 64, False), (256, 200, False), (1024, 1024, True), (4096, 4096, False)]


@pytest.fixture(scope="module")
def dev():
    return torch.device("cuda", 0)


@pytest.fixture(scope="module")
def corpus():
    """tests/test_gpu_frame_points.py's: five clips of 0.05 .. 0.5 s, one with a stretch of exact zeros."""
    secs = (0.05, 0.11, 0.2, 0.3667, 0.5)
    clips = [orc.synth_clip(40 + i, 3 * i + 1, seconds=s) for i, s in enumerate(secs)]
    clips[2] = clips[2].copy()
    clips[2][3000:5200] = 0.0
    return clips, np.array([4, 9, 2, 7, 5])


def _shuffled_with_repeats(n, seed):
    rng = np.random.Generator(np.random.PCG64(seed))
    return np.concatenate([rng.permutation(n), rng.integers(0, n, size=max(8, n // 10))])


def _bits(t):
    return t.contiguous().view(torch.int32)


class _Launch:
    """The resident corpus of a waveform dataset and the two launches over it with the same arguments."""

    def __init__(self, corpus, n_fft, win, drop, ntemp, dev, **aug):
        import dataset
        clips, y = corpus
        self.clips = clips
        kw = dict(win_lengths=(win,), device=dev)
        self.ds = (dataset.ESC_wave_pc(clips, y, FS, n_fft, drop_nyquist=drop, **kw) if ntemp == 1
                   else dataset.ESC_wave_pc_temp(clips, y, FS, n_fft, ntemp, **kw))
        self.res = self.ds._resident()
        self.win = torch.tensor([win], dtype=torch.int32, device=dev)
        self.n_fft, self.Nt, self.F, self.hop, self.dev = n_fft, ntemp, self.ds.F, self.ds.hop, dev
        self.aug = aug

    def _args(self, idx, kw):
        waves, woff, soff, f32, t32, lab = self.res
        a = dict(max_len=self.ds._max_len, min_len=self.ds._min_len, clip_labels=lab,
                 win_lengths=self.win, draw=3, **self.aug)
        a.update(kw)
        return (waves, woff, soff, idx, self.n_fft, self.hop, self.F, f32, t32, self.Nt), a

    def plain(self, idx, **kw):
        import pca_hip
        pos, a = self._args(idx, kw)
        return pca_hip.frame_points(*pos, **a)

    def moved(self, idx, **kw):
        import pca_hip
        pos, a = self._args(idx, kw)
        return pca_hip.frame_points_reassigned(*pos, **a)

    def axes32(self):
        f = np.asarray(self.ds.farr, dtype=np.float64).astype(np.float32)
        t = None if self.ds.tarr is None else np.asarray(self.ds.tarr, dtype=np.float64).astype(np.float32)
        return f, t


def _idx_for(L, n_fft):
    n = len(L.ds)
    if n_fft == 4096:                             # B = 4: the 96 KiB LDS path, 9 bins per thread
        return np.array([n - 1, 0, n // 2, n - 1] if L.Nt > 1 else [n - 2, 1, n // 2, n - 2])
    return _shuffled_with_repeats(n, 1 + L.Nt)


# ---- 1. parity with the restatement, 2. the bit identities that hold in every case ---------------------
@pytest.mark.parametrize("ntemp", [1, 4], ids=["din2-f", "din3-ft"])
@pytest.mark.parametrize("n_fft,win,drop", CASES)
def test_every_point_against_numpy(n_fft, win, drop, ntemp, corpus, dev):
    """Bar per coordinate column: 4 np.spacing(float32(max |reference coordinate|)) - both sides compute in
    fp64 from the same fp32 inputs and round once; what differs is the order of the butterflies and of the
    products, ~1e-13 relative at bins within log(1e3) of the frame's maximum."""
    L = _Launch(corpus, n_fft, win, drop, ntemp, dev, **AUG)
    axes = "f" if ntemp == 1 else "ft"
    idx = _idx_for(L, n_fft)
    ids = torch.from_numpy(idx).to(dev)
    B, F, Nt = idx.size, L.F, ntemp
    grid, glab, gmeta = L.plain(ids, want_meta=True)
    got, lab, meta = L.moved(ids, want_meta=True, axes=axes, **SPEC)
    assert got.shape == grid.shape == (B, Nt * F, 2 if ntemp == 1 else 3)
    # value column, labels and meta are the plain launch's bits
    assert torch.equal(_bits(got[:, :, -1]), _bits(grid[:, :, -1]))
    assert torch.equal(lab, glab) and torch.equal(meta, gmeta)
    again = L.moved(ids, axes=axes, **SPEC)[0]
    assert torch.equal(_bits(again), _bits(got))

    g, m = got.cpu().numpy(), meta.cpu().numpy()
    values = g[:, :, -1]
    farr, tarr = L.axes32()
    first = reassign_ref.first_centres(L.clips, L.ds.set_off, idx, m, values, n_fft, L.hop, Nt, AUG["jitter"])
    f_ref, t_ref, moved, sdb = reassign_ref.reassign_batch(L.clips, first, m, values, n_fft, L.hop, Nt, farr,
                                                           tarr, axes=axes, **SPEC)
    bar_f = 4 * np.spacing(np.float32(np.abs(f_ref).max()))
    err_f = np.abs(g[:, :, 0].astype(np.float64) - f_ref).max()
    clamped = int((np.abs(sdb) == 2.0).sum())
    print(f"n_fft {n_fft} win {win} {axes}: {B} sets, moved {moved.mean():.1%}, clamped {clamped}, "
          f"frequency |delta| {err_f:.3e} (bar {bar_f:.3e})")
    assert err_f <= bar_f
    if ntemp > 1:
        bar_t = 4 * np.spacing(np.float32(np.abs(t_ref).max()))
        err_t = np.abs(g[:, :, 1].astype(np.float64) - t_ref).max()
        print(f"    time |delta| {err_t:.3e} (bar {bar_t:.3e})")
        assert err_t <= bar_t
    # not vacuous
    assert moved.mean() >= 0.25 and clamped >= 1
    # a row that did not move is the grid row
    assert np.array_equal(g[~moved].view(np.int32), grid.cpu().numpy()[~moved].view(np.int32))


# ---- 2. the other bit identities ------------------------------------------------------------------------
@pytest.mark.parametrize("ntemp", [1, 3], ids=["din2", "din3"])
def test_bit_identities_with_the_plain_launch(ntemp, corpus, dev):
    L = _Launch(corpus, 256, 200, False, ntemp, dev, **AUG)
    ids = torch.from_numpy(_shuffled_with_repeats(len(L.ds), 5)).to(dev)
    axes = "f" if ntemp == 1 else "ft"
    grid, glab, gmeta = L.plain(ids, want_meta=True)
    # strength 0: the whole output
    zero, lab, meta = L.moved(ids, want_meta=True, axes=axes, **dict(SPEC, strength=0.0))
    assert torch.equal(_bits(zero), _bits(grid)) and torch.equal(lab, glab) and torch.equal(meta, gmeta)
    # buffers passed in, no labels
    out = torch.full_like(grid, 3.0)
    res = L.moved(ids, axes=axes, out=out, clip_labels=None, **SPEC)
    assert res[0] is out and res[1] is None
    full = L.moved(ids, axes=axes, **SPEC)[0]
    assert torch.equal(_bits(out), _bits(full)) and not torch.equal(_bits(full), _bits(grid))
    if ntemp > 1:
        only_f = L.moved(ids, axes="f", **SPEC)[0]
        assert torch.equal(_bits(only_f[:, :, 1]), _bits(grid[:, :, 1]))           # time untouched
        assert torch.equal(_bits(only_f[:, :, 0]), _bits(full[:, :, 0]))
        only_t = L.moved(ids, axes="t", **SPEC)[0]
        assert torch.equal(_bits(only_t[:, :, 0]), _bits(grid[:, :, 0]))
        assert torch.equal(_bits(only_t[:, :, 1]), _bits(full[:, :, 1]))
        assert not torch.equal(_bits(only_t[:, :, 1]), _bits(grid[:, :, 1]))
    # frames inside the zeros [3000, 5200) of clip 2, shifted by up to 37 samples: p = 0, the grid rows
    zs = torch.tensor([L.ds.set_off[2] + 3000 // (128 * ntemp) + 2 + k for k in range(3)], device=dev)
    zg = L.plain(zs)[0]
    zm = L.moved(zs, axes=axes, **SPEC)[0]
    assert ((zg[:, :, -1] - float(np.log(np.float32(1e-8)))).abs() < 5e-5).all()           # silent frames
    assert torch.equal(_bits(zm), _bits(zg))
    # NORM_WIN: the same coordinates, the plain launch's values
    import pca_hip
    nw = L.moved(ids, axes=axes, norm_mode=pca_hip.NORM_WIN, **SPEC)[0]
    assert torch.equal(_bits(nw[:, :, -1]), _bits(L.plain(ids, norm_mode=pca_hip.NORM_WIN)[0][:, :, -1]))


# ---- 3. floors off: invariants --------------------------------------------------------------------------
@pytest.mark.parametrize("n_fft,ntemp", [(256, 1), (1024, 4)])
def test_floors_off_invariants(n_fft, ntemp, corpus, dev):
    L = _Launch(corpus, n_fft, n_fft, ntemp > 1, ntemp, dev, **AUG)
    ids = torch.from_numpy(_shuffled_with_repeats(len(L.ds), 7)).to(dev)
    axes = "f" if ntemp == 1 else "ft"
    farr, tarr = L.axes32()
    grid = L.plain(ids)[0].cpu().numpy()
    df = float(farr[1]) - float(farr[0])
    spread = {}
    for max_df in (2.0, 0.25):
        g = L.moved(ids, axes=axes, rel_floor=float("inf"), max_df=max_df, max_dt=0.5)[0].cpu().numpy()
        assert np.isfinite(g).all()
        assert g[:, :, 0].min() >= farr[0] and g[:, :, 0].max() <= farr[-1]
        shift = np.abs(g[:, :, 0].astype(np.float64) - grid[:, :, 0]) / df
        spread[max_df] = shift.max()
        assert shift.max() <= max_df + 1e-3, (max_df, shift.max())             # 1e-3 bin: fp32 rounding of f
        assert (shift > 0).mean() > 0.5
        if ntemp > 1:
            dt = float(tarr[1]) - float(tarr[0])
            ts = np.abs(g[:, :, 1].astype(np.float64) - grid[:, :, 1]) / dt
            assert 0.49 < ts.max() <= 0.5 + 1e-3
    assert spread[2.0] > 1.9 and 0.24 < spread[0.25]                            # the smaller clamp binds


# ---- 4. the device half of the draw number, under a captured graph -------------------------------------
def test_captured_launch_draws_afresh_on_replay(corpus, dev):
    L = _Launch(corpus, 256, 200, False, 1, dev, **AUG)
    ids = torch.from_numpy(_shuffled_with_repeats(len(L.ds), 9)[:64]).to(dev)
    out = torch.zeros((64, L.F, 2), device=dev)
    lab = torch.zeros(64, dtype=torch.int64, device=dev)
    step = torch.zeros(2, dtype=torch.int32, device=dev)
    kw = dict(out=out, labels_out=lab, draw_dev=step, **SPEC)
    s = torch.cuda.Stream(dev)
    s.wait_stream(torch.cuda.current_stream(dev))
    with torch.cuda.stream(s):
        L.moved(ids, **kw)                                                       # warm-up
    torch.cuda.current_stream(dev).wait_stream(s)
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        L.moved(ids, **kw)
    seen = []
    for k in range(3):
        step[0] = k
        out.zero_()
        g.replay()
        torch.cuda.synchronize()
        seen.append(out.clone())
        want = L.moved(ids, draw=3 + k, **SPEC)[0]                               # the host draw number
        assert torch.equal(_bits(seen[-1]), _bits(want)), k
    assert not torch.equal(_bits(seen[0]), _bits(seen[1])) and not torch.equal(_bits(seen[1]), _bits(seen[2]))
