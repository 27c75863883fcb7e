"""pca_frame_points_pcen on the device: every row against the numpy restatement (tests/pcen_ref.py) of what
``meta`` says was drawn, under a bar the test sizes on the CPU for its own inputs; meta and labels are the
band launch's bits; a smoother without memory ignores the context; with the normalisation switched off the
value is the band launch's energy; which workgroup arrives last does not matter, the tickets come back zero
and a captured launch replays; a stationary tone sits at the closed-form steady state."""
import numpy as np
import pytest
import torch

import pcen_ref
from oracle import st_oracle as orc

pytestmark = pytest.mark.gpu

FS = 44100
JITTER = 20


@pytest.fixture(scope="module")
def dev():
    return torch.device("cuda", 0)


@pytest.fixture(scope="module")
def corpus():
    """Three clips of a few thousand samples, the last one a tone that repeats exactly every 32 samples (so
    every frame of it away from the ends holds the same samples at hop 32 and 64); one label per clip."""
    clips = [orc.synth_clip(70 + i, 2 * i + 3, seconds=s) for i, s in enumerate((0.06, 0.085))]
    one = 0.3 * np.sin(2 * np.pi * (5.0 / 32.0) * np.arange(32)) + 0.1 * np.sin(2 * np.pi * (11.0 / 32.0) *
                                                                               np.arange(32) + 0.7)
    clips.append(np.tile(one.astype(np.float32), 120))
    return clips, np.array([6, 1, 8])


def _bits(t):
    return t.contiguous().view(torch.int32)


def _f32(a, dev):
    return torch.as_tensor(np.asarray(a, dtype=np.float64)).float().to(dev)


def _random_bank(n_fft, n_bands, power, seed):
    """Overlapping bands of 1 .. 9 bins with random weights, spread over all n_fft/2 + 1 bins."""
    import pca_hip
    rng = np.random.Generator(np.random.PCG64(seed))
    nb = n_fft // 2 + 1
    W = np.zeros((n_bands, nb))
    for m in range(n_bands):
        width = int(rng.integers(1, 10))
        lo = int(round(m * (nb - width) / max(n_bands - 1, 1)))
        W[m, lo:lo + width] = rng.uniform(0.1, 1.0, width)
    return pca_hip.FilterBank(W, np.linspace(0.0, FS / 2, n_bands), power=power)


class _Case:
    """The resident corpus and the axes of one (n_fft, Nt) framing, as the datasets lay them out."""

    def __init__(self, clips, y, n_fft, Nt, dev):
        import dataset
        self.clips, self.n_fft, self.hop, self.Nt = clips, n_fft, n_fft // 2, Nt
        lens = [len(c) for c in clips]
        self.set_off = dataset.wave_set_offsets(lens, self.hop, Nt)
        i64 = lambda a: torch.as_tensor(np.asarray(a, dtype=np.int64)).to(dev)   # noqa: E731
        self.waves = torch.cat([torch.from_numpy(c).to(dev) for c in clips])
        self.woff, self.soff, self.lab = i64([0] + list(np.cumsum(lens))), i64(self.set_off), i64(y)
        self.kw = dict(max_len=max(lens), min_len=min(lens), clip_labels=self.lab)
        self.tarr = np.linspace(0, self.hop / FS * Nt, Nt) if Nt > 1 else None
        self.t32 = _f32(self.tarr, dev) if Nt > 1 else None
        self.wins = (n_fft, n_fft * 3 // 4)
        self.win_dev = torch.tensor(self.wins, dtype=torch.int32, device=dev)
        self.one_win = torch.tensor([n_fft], dtype=torch.int32, device=dev)
        self.dev = dev

    def idx(self, B):
        """B = 1: the last set of clip 1.  B = 5: a clip's first and last set (clamped centres: the context
        before the first lies before the clip), mid-clip, and the corpus' last."""
        so = self.set_off
        if B == 1:
            return np.array([so[2] - 1], dtype=np.int64)
        return np.array([so[0], so[1] - 1, (so[1] + so[2]) // 2, so[1], so[3] - 1], dtype=np.int64)

    def pcen(self, idx, bank, spec, wins=None, **kw):
        import pca_hip
        return pca_hip.frame_points_pcen(self.waves, self.woff, self.soff, torch.from_numpy(idx).to(self.dev),
                                         self.n_fft, self.hop, bank, _f32(bank.centres / FS, self.dev), self.t32,
                                         self.Nt, pcen=spec, fs=FS, win_lengths=self.win_dev if wins is None
                                         else wins, **self.kw, **kw)

    def bands(self, idx, bank, wins=None, **kw):
        import pca_hip
        return pca_hip.frame_points_bands(self.waves, self.woff, self.soff, torch.from_numpy(idx).to(self.dev),
                                          self.n_fft, self.hop, bank, _f32(bank.centres / FS, self.dev), self.t32,
                                          self.Nt, win_lengths=self.win_dev if wins is None else wins,
                                          **self.kw, **kw)

    def workspace(self, B, T, n_bands):
        return (torch.full((B, T, n_bands), float("nan"), dtype=torch.float64, device=self.dev),
                torch.zeros(B, dtype=torch.int32, device=self.dev))


AUG = dict(jitter=JITTER, gain_db=6.0, norm_mode=1, seed=11, draw=5)


def _gain(meta_row):
    return np.array([meta_row[3]], dtype=np.int32).view(np.float32)[0]


def _ref_struct(spec, hop):
    """The fp32 parameters the launch gets from a pca_hip.Pcen."""
    return pcen_ref.spec(spec.context, spec.coefficient(FS, hop), spec.gain, spec.bias, spec.power, spec.eps,
                         spec.scale)


def _against_ref(case, idx, pts, meta, bank, spec, norm_mode):
    """Every row of every slot rebuilt from what ``meta`` reports.  Returns (|got - float64 restatement| per
    value, one fp32 step of every value, D): D is the largest distance between the float64 restatement and the
    one with the kernel's fp32 magnitudes, over the same rows - what the bar is made of."""
    n_fft, hop, Nt = case.n_fft, case.hop, case.Nt
    W, p = bank.dense(), _ref_struct(spec, hop)
    farr = bank.centres / FS
    diffs, ulps, D = [], [], 0.0
    for b, i in enumerate(idx):
        c, centre0, win, _ = (int(v) for v in meta[b])
        assert case.set_off[c] <= i < case.set_off[c + 1] and win in case.wins
        wave, L, s = case.clips[c], len(case.clips[c]), int(i) - case.set_off[c]
        nominal = s * Nt * hop
        # the shifts that explain frame 0's centre: one, unless the clamp to [0, L] took hold of it
        deltas = [d for d in range(-JITTER, JITTER + 1) if min(max(nominal + d, 0), L) == centre0]
        assert deltas and (len(deltas) == 1 or centre0 in (0, L)), (b, centre0, nominal)
        best = None
        for d in deltas:
            args = (wave, s, d, Nt, hop, n_fft, win, _gain(meta[b]), n_fft if norm_mode == 0 else win, W,
                    bank.power, p)
            y64 = pcen_ref.slot_values(*args)
            y32 = pcen_ref.slot_values(*args, fp32_mag=True)
            want = pcen_ref.rows(y64, farr, case.tarr)
            assert want.shape == pts[b].shape
            assert np.array_equal(pts[b][:, :-1], want[:, :-1]), b        # coordinates: exactly
            ulp = np.spacing(np.abs(want[:, -1])).astype(np.float64)
            diff = np.abs(pts[b][:, -1].astype(np.float64) - y64.reshape(-1))
            if best is None or diff.max() < best[0].max():
                best = (diff, ulp, float(np.abs(y64 - y32).max()))
        diffs.append(best[0])
        ulps.append(best[1])
        D = max(D, best[2])
    return np.concatenate(diffs), np.concatenate(ulps), D


CASES = {   # n_fft, n_bands, bank power, Nt, W, B, the spec's other fields
    "64-5b-Nt1-W0-B1": (64, 5, 2, 1, 0, 1, dict(s=0.3)),
    "64-37b-Nt3-W1-B5": (64, 37, 2, 3, 1, 5, dict(time_constant=0.01)),
    "128-37b-Nt3-W7-B5": (128, 37, 1, 3, 7, 5, dict(s=0.2, gain=0.8, bias=10.0, power=0.25, scale=100.0)),
    "128-5b-Nt1-W7-B5": (128, 5, 2, 1, 7, 5, dict(s=0.05, eps=1e-3)),
    "64-37b-Nt1-W7-B1": (64, 37, 1, 1, 7, 1, dict(s=0.5, gain=1.0, bias=0.0, power=1.0)),
    "1024-513b-Nt1-W1-B1": (1024, 513, 1, 1, 1, 1, dict(s=0.4)),       # more than 256 bands: the m loop
}


def _bank(n_fft, n_bands, power, seed=3):
    import pca_hip
    if n_bands == n_fft // 2 + 1:                                     # identity-like
        return pca_hip.FilterBank(np.eye(n_bands) * 0.5, np.linspace(0.0, FS / 2, n_bands), power=power)
    return _random_bank(n_fft, n_bands, power, seed)


# ---- 1. + 2. against the restatement; meta and labels are the band launch's -----------------------------
@pytest.mark.parametrize("name", list(CASES))
def test_against_numpy_and_the_band_launch(name, corpus, dev):
    """The bar of a value is 4 D + one fp32 step of it, D from the CPU alone (_against_ref); the worst
    difference and the bar are printed, DESIGN section 7 records what an MI355X gave."""
    import pca_hip
    n_fft, n_bands, power, Nt, W, B, kw = CASES[name]
    clips, y = corpus
    case = _Case(clips, y, n_fft, Nt, dev)
    bank = _bank(n_fft, n_bands, power)
    spec = pca_hip.Pcen(context=W, **kw)
    idx = case.idx(B)
    norm_mode = 1 if Nt == 3 else 0
    aug = dict(AUG, norm_mode=norm_mode)
    ws = case.workspace(B, W + Nt, n_bands)
    pts, lab, meta = case.pcen(idx, bank, spec, want_meta=True, workspace=ws, **aug)
    _, band_lab, band_meta = case.bands(idx, bank, want_meta=True, **aug)
    assert torch.equal(meta, band_meta) and torch.equal(lab, band_lab)
    assert int(ws[1].abs().sum()) == 0                                  # the tickets are zero again
    pts, lab, meta = pts.cpu().numpy(), lab.cpu().numpy(), meta.cpu().numpy()
    assert pts.shape == (B, Nt * n_bands, 3 if Nt > 1 else 2) and np.isfinite(pts).all()
    assert np.array_equal(lab, y[meta[:, 0]])
    diff, ulp, D = _against_ref(case, idx, pts, meta, bank, spec, norm_mode)
    w = int(np.argmax(diff - ulp))
    print(f"frame_points_pcen {name}: worst |delta| {diff.max():.3e}, nearest the bar {diff[w]:.3e} under "
          f"4 D + ulp = {4 * D:.3e} + {ulp[w]:.3e}, largest |y| {np.abs(pts[:, :, -1]).max():.3e}, {B} slots, "
          f"all rows")
    assert D > 0.0 and (diff <= 4 * D + ulp).all()


# ---- 3. no memory: the context cannot matter ------------------------------------------------------------
def test_without_memory_the_context_does_not_matter(corpus, dev):
    import pca_hip
    clips, y = corpus
    case = _Case(clips, y, 64, 3, dev)
    bank = _bank(64, 37, 2)
    idx = case.idx(5)
    a, _, ma = case.pcen(idx, bank, pca_hip.Pcen(context=0, s=1.0), want_meta=True, **AUG)
    b, _, mb = case.pcen(idx, bank, pca_hip.Pcen(context=7, s=1.0), want_meta=True, **AUG)
    assert torch.equal(_bits(a), _bits(b)) and torch.equal(ma, mb)
    c, _ = case.pcen(idx, bank, pca_hip.Pcen(context=7, s=0.25), **AUG)
    assert not torch.equal(_bits(a), _bits(c))                          # with memory it does


# ---- 4. normalisation off: the band launch's energy -----------------------------------------------------
@pytest.mark.parametrize("power", [1, 2])
def test_normalisation_off_is_the_band_energy(power, corpus, dev):
    """y is (float)E, so logf(amin + y) is the band launch's value: the logarithm is taken where the band
    launch takes it, on the device in fp32 (torch.log of a float32 tensor).  A host logarithm is another
    function: on an MI355X the band launch's values sit up to 2 fp32 steps from the correctly rounded
    logarithm of the same argument (float64, rounded once) and from numpy's float32 log, whatever y is; that
    distance is printed beside the one asserted."""
    import pca_hip
    clips, y = corpus
    case = _Case(clips, y, 128, 3, dev)
    bank = _bank(128, 37, power)
    idx = case.idx(5)
    off = pca_hip.Pcen(context=1, s=0.3, gain=0.0, bias=0.0, power=1.0, scale=1.0)
    e, _ = case.pcen(idx, bank, off, **AUG)
    want, _ = case.bands(idx, bank, **AUG)
    got = torch.log(torch.tensor(bank.amin, dtype=torch.float32, device=dev) + e[:, :, -1]).cpu().numpy()
    e, want = e.cpu().numpy(), want.cpu().numpy()
    assert np.array_equal(e[:, :, :-1], want[:, :, :-1])
    step = np.spacing(np.abs(want[:, :, -1])).astype(np.float64)
    steps = np.abs(got.astype(np.float64) - want[:, :, -1]) / step
    host = np.log((np.float32(bank.amin) + e[:, :, -1]).astype(np.float64)).astype(np.float32)
    print(f"frame_points_pcen off, power {power}: logf(amin + y) within {steps.max():.2f} fp32 steps of the "
          f"band launch, {int((steps == 0).sum())} of {steps.size} rows bit-equal; the correctly rounded host "
          f"logarithm within {(np.abs(host.astype(np.float64) - want[:, :, -1]) / step).max():.2f}")
    assert steps.max() <= 1.0


# ---- 5. last-arrival independence and replay ------------------------------------------------------------
def test_last_arrival_independence_and_replay(corpus, dev):
    import pca_hip
    clips, y = corpus
    case = _Case(clips, y, 128, 3, dev)
    bank = _bank(128, 37, 2)
    spec = pca_hip.Pcen(context=7, s=0.1)
    B, T = 5, 10
    same = np.full(B, (case.set_off[1] + case.set_off[2]) // 2, dtype=np.int64)
    ws = case.workspace(B, T, 37)
    off = dict(wins=case.one_win, seed=3, draw=1)
    a, _ = case.pcen(same, bank, spec, workspace=ws, **off)
    assert int(ws[1].abs().sum()) == 0 and bool(torch.isfinite(ws[0]).all())
    for b in range(1, B):
        assert torch.equal(_bits(a[b]), _bits(a[0])), b                   # five slots, one set
    ws[0].fill_(float("nan"))                                             # nothing stale is read
    a2, _ = case.pcen(same, bank, spec, workspace=ws, **off)
    assert torch.equal(_bits(a2), _bits(a)) and int(ws[1].abs().sum()) == 0

    # captured: the tickets need no memset node, every replay finds them zero
    idx = case.idx(5)
    eager, eager_lab = case.pcen(idx, bank, spec, workspace=ws, **AUG)
    out = torch.zeros_like(eager)
    lab = torch.zeros(B, dtype=torch.int64, device=dev)
    idx_dev = torch.from_numpy(idx).to(dev)
    f32 = _f32(bank.centres / FS, dev)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        pca_hip.frame_points_pcen(case.waves, case.woff, case.soff, idx_dev, 128, 64, bank, f32, case.t32, 3,
                                  pcen=spec, fs=FS, win_lengths=case.win_dev, out=out, labels_out=lab,
                                  workspace=ws, **case.kw, **AUG)
    for k in range(3):
        out.zero_()
        ws[0].fill_(float("nan"))
        g.replay()
        torch.cuda.synchronize()
        assert torch.equal(_bits(out), _bits(eager)) and torch.equal(lab, eager_lab), k
        assert int(ws[1].abs().sum()) == 0, k


# ---- 6. a stationary tone sits at the steady state --------------------------------------------------------
@pytest.mark.parametrize("n_fft", [64, 128])
def test_stationary_tone_is_at_the_steady_state(n_fft, corpus, dev):
    import pca_hip
    clips, y = corpus
    Nt, W, hop = 3, 7, n_fft // 2
    case = _Case(clips, y, n_fft, Nt, dev)
    bank = _bank(n_fft, 37, 2)
    spec = pca_hip.Pcen(context=W, s=0.2, gain=0.9, bias=1.0, power=0.5, scale=50.0)
    tone = clips[2]
    s_set = len(tone) // (2 * Nt * hop)                                    # mid-clip
    centres = pcen_ref.slot_centres(len(tone), s_set, 0, Nt, hop, W)
    assert min(centres) >= n_fft and max(centres) <= len(tone) - n_fft     # no frame reaches the ends
    idx = np.array([case.set_off[2] + s_set], dtype=np.int64)
    pts, _ = case.pcen(idx, bank, spec, wins=case.one_win)
    got = pts.cpu().numpy()[0, :, -1].astype(np.float64).reshape(Nt, 37)
    p = _ref_struct(spec, hop)
    E64 = pcen_ref.energies(tone, centres[:1], n_fft, n_fft, 1.0, n_fft, bank.dense(), 2)[0]
    E32 = pcen_ref.energies(tone, centres[:1], n_fft, n_fft, 1.0, n_fft, bank.dense(), 2, fp32_mag=True)[0]
    want = pcen_ref.steady_state(p["scale"] * E64, p)
    D = float(np.abs(want - pcen_ref.steady_state(p["scale"] * E32, p)).max())
    ulp = np.spacing(np.abs(want.astype(np.float32))).astype(np.float64)
    diff = np.abs(got - want[None, :])
    print(f"frame_points_pcen tone n_fft {n_fft}: worst |delta| {diff.max():.3e}, bar 4 D + ulp = {4 * D:.3e} + "
          f"{ulp.max():.3e} at most")
    assert want.max() > 0.1 and D > 0.0 and (diff <= 4 * D + ulp[None, :]).all()
