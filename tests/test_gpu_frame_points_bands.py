"""pca_frame_points_bands on the device: the identity bank is pca_frame_points bit for bit; mel banks and a
hand-made bank against the numpy restatement (tests/bands_ref.py) of what ``meta`` says was drawn, every row
of every slot; bands outside the frame's bins are clipped on the device; the draws are reproducible and
advance per replay of a captured launch."""
import numpy as np
import pytest
import torch

import bands_ref
from oracle import st_oracle as orc

pytestmark = pytest.mark.gpu

FS = 44100
TOL = 5e-5          # test_gpu_frame_points.py's bar: the same fp64 transform on both sides
JITTER = 37


@pytest.fixture(scope="module")
def dev():
    return torch.device("cuda", 0)


@pytest.fixture(scope="module")
def corpus():
    """Five clips of 0.05 .. 0.5 s, one with a stretch of exact zeros; one label per clip
    (test_gpu_frame_points_multires.py's corpus)."""
    secs = (0.05, 0.11, 0.2, 0.3667, 0.5)
    clips = [orc.synth_clip(40 + i, 3 * i + 1, seconds=s) for i, s in enumerate(secs)]
    clips[2] = clips[2].copy()
    clips[2][3000:5200] = 0.0
    return clips, np.array([4, 9, 2, 7, 5])


def _bits(t):
    return t.contiguous().view(torch.int32)


def _f32(a, dev):
    return torch.as_tensor(np.asarray(a, dtype=np.float64)).float().to(dev)


class _Case:
    """The resident corpus and the axes of one (n_fft, Nt) framing, as the datasets lay them out."""

    def __init__(self, clips, y, n_fft, Nt, dev, three=None):
        import dataset
        self.clips, self.n_fft, self.hop, self.Nt = clips, n_fft, n_fft // 2, Nt
        lens = [len(c) for c in clips]
        self.set_off = dataset.wave_set_offsets(lens, self.hop, Nt)
        i64 = lambda a: torch.as_tensor(np.asarray(a, dtype=np.int64)).to(dev)   # noqa: E731
        self.waves = torch.cat([torch.from_numpy(c).to(dev) for c in clips])
        self.woff, self.soff, self.lab = i64([0] + list(np.cumsum(lens))), i64(self.set_off), i64(y)
        self.kw = dict(max_len=max(lens), min_len=min(lens), clip_labels=self.lab)
        self.three = Nt > 1 if three is None else three
        self.tarr = np.linspace(0, self.hop / FS * Nt, Nt) if self.three else None
        self.t32 = _f32(self.tarr, dev) if self.three else None
        self.wins = (n_fft, n_fft * 3 // 4)
        self.win_dev = torch.tensor(self.wins, dtype=torch.int32, device=dev)
        self.dev = dev

    def idx(self, seed, clamp=True, zero_sets=()):
        """First and last set of every clip, the sets inside the zero stretch, a shuffle with repeats and
        two ids out of range (clamped on the device)."""
        n = self.set_off[-1]
        rng = np.random.Generator(np.random.PCG64(seed))
        parts = [self.set_off[:-1], np.asarray(self.set_off[1:]) - 1, list(zero_sets),
                 rng.permutation(n)[:24], rng.integers(0, n, size=8)]
        if clamp:
            parts.append([-3, n + 5])
        return np.concatenate([np.asarray(p, dtype=np.int64) for p in parts])

    def bands(self, idx, bank, farr, **kw):
        import pca_hip
        return pca_hip.frame_points_bands(self.waves, self.woff, self.soff, torch.from_numpy(idx).to(self.dev),
                                          self.n_fft, self.hop, bank, _f32(farr, self.dev), self.t32, self.Nt,
                                          win_lengths=self.win_dev, **self.kw, **kw)

    def plain(self, idx, n_bins, farr, **kw):
        import pca_hip
        return pca_hip.frame_points(self.waves, self.woff, self.soff, torch.from_numpy(idx).to(self.dev),
                                    self.n_fft, self.hop, n_bins, _f32(farr, self.dev), self.t32, self.Nt,
                                    win_lengths=self.win_dev, **self.kw, **kw)


AUG = dict(jitter=JITTER, gain_db=6.0, norm_mode=1, seed=11, draw=5)


# ---- 1. the identity bank is the plain launch -------------------------------------------------------------
@pytest.mark.parametrize("n_fft,Nt,n_bins", [(64, 1, 33), (256, 4, 128)], ids=["64-2d-33", "256-Nt4-128"])
def test_identity_bank_is_the_plain_launch(n_fft, Nt, n_bins, corpus, dev):
    import pca_hip
    clips, y = corpus
    case = _Case(clips, y, n_fft, Nt, dev)
    bank = pca_hip.FilterBank(np.eye(n_fft // 2 + 1)[:n_bins], np.arange(n_bins), power=1, amin=1e-8)
    assert bank.nnz == bank.n_bands == n_bins and bank.band_lo.tolist() == list(range(n_bins))
    farr = np.linspace(0, FS / 2, n_bins) / FS
    idx = case.idx(1)
    pts, lab, meta = case.bands(idx, bank, farr, want_meta=True, **AUG)
    want, want_lab, want_meta = case.plain(idx, n_bins, farr, want_meta=True, **AUG)
    assert pts.shape == want.shape == (idx.size, Nt * n_bins, 3 if Nt > 1 else 2)
    assert torch.equal(_bits(pts), _bits(want))
    assert torch.equal(lab, want_lab) and torch.equal(meta, want_meta)
    m = meta.cpu().numpy()
    assert set(m[:, 2].tolist()) == set(case.wins) and len(set(m[:, 3].tolist())) > 16   # the augmentation is on


# ---- 2. + 3. against the numpy restatement ----------------------------------------------------------------
def _gain(meta_row):
    return np.array([meta_row[3]], dtype=np.int32).view(np.float32)[0]


def _against_ref(case, idx, pts, meta, bank, farr, norm_mode):
    """Every row of every slot rebuilt from what ``meta`` reports; returns max |delta| of the values."""
    n_fft, hop, Nt = case.n_fft, case.hop, case.Nt
    W = bank.dense()                              # the fp32 weights the device applies, in fp64
    total, worst = case.set_off[-1], 0.0
    for b, i in enumerate(idx):
        i = min(max(int(i), 0), total - 1)
        c, centre0, win, _ = (int(v) for v in meta[b])
        assert case.set_off[c] <= i < case.set_off[c + 1] and win in case.wins
        wave, L, s = case.clips[c], len(case.clips[c]), i - case.set_off[c]
        nominal = s * Nt * hop
        assert max(0, nominal - JITTER) <= centre0 <= min(L, nominal + JITTER), (b, centre0, nominal)

        def err(delta):
            want = bands_ref.slot_rows(wave, s, delta, Nt, hop, n_fft, win, _gain(meta[b]),
                                       n_fft if norm_mode == 0 else win, W, bank.power, bank.amin, farr,
                                       case.tarr)
            assert want.shape == pts[b].shape
            assert np.array_equal(pts[b][:, :-1], want[:, :-1]), b        # coordinates: exactly
            return float(np.abs(pts[b][:, -1] - want[:, -1]).max())

        if centre0 > 0 or nominal > 0 or Nt == 1:
            e = err(centre0 - nominal)
        else:     # frame 0 clamped at the clip's start: one shift of [-jitter, 0] explains the other frames
            e = min(err(d) for d in range(-JITTER, 1))
        worst = max(worst, e)
    return worst


def _floor_rows(pts, slots, amin):
    """Largest distance of the slots' values from logf(amin), in units of one fp32 step at that value."""
    floor = np.float32(np.log(np.float64(np.float32(amin))))
    return float(np.abs(pts[slots][:, :, -1] - floor).max() / np.spacing(np.abs(floor)))


MEL_CASES = {      # n_fft, n_mels, mel_bank keywords, Nt, sets of clip 2 whose frames lie inside its zeros
    "256-16-slaney-p2-2d": (256, 16, dict(power=2), 1, (28, 30, 36)),
    "1024-64-slaney-p1-Nt2": (1024, 64, dict(power=1), 2, (4,)),
    "256-24-htk-flat-p2-Nt4": (256, 24, dict(htk=True, norm=None, power=2, amin=1e-6), 4, (7,)),
}


@pytest.mark.parametrize("name", list(MEL_CASES))
def test_mel_bank_against_numpy(name, corpus, dev):
    import pca_hip
    n_fft, n_mels, mel_kw, Nt, zero = MEL_CASES[name]
    clips, y = corpus
    case = _Case(clips, y, n_fft, Nt, dev)
    bank = pca_hip.mel_bank(FS, n_fft, n_mels, **mel_kw)
    farr = bank.centres / FS
    zero_sets = [case.set_off[2] + s for s in zero]
    idx = case.idx(2, zero_sets=zero_sets)
    norm_mode = 1 if Nt == 2 else 0
    pts, lab, meta = case.bands(idx, bank, farr, want_meta=True, **dict(AUG, norm_mode=norm_mode))
    pts, lab, meta = pts.cpu().numpy(), lab.cpu().numpy(), meta.cpu().numpy()
    assert pts.shape == (idx.size, Nt * n_mels, 3 if Nt > 1 else 2) and np.isfinite(pts).all()
    assert np.array_equal(lab, y[meta[:, 0]])
    worst = _against_ref(case, idx, pts, meta, bank, farr, norm_mode)
    print(f"frame_points_bands {name}: max |delta| {worst:.3e} over {idx.size} slots, all rows")
    assert worst <= TOL
    assert set(meta[:, 2].tolist()) == set(case.wins) and len(set(meta[:, 3].tolist())) > 16
    # inside the stretch of exact zeros every band is empty of energy: logf(amin), to one fp32 step of logf
    slots = np.arange(10, 10 + len(zero))
    assert np.array_equal(idx[slots], zero_sets)
    steps = _floor_rows(pts, slots, bank.amin)
    print(f"frame_points_bands {name}: silent rows within {steps:.2f} fp32 steps of logf(amin)")
    assert steps <= 1.0


@pytest.mark.parametrize("power", [1, 2])
def test_hand_made_bank_against_numpy(power, corpus, dev):
    import pca_hip
    clips, y = corpus
    case = _Case(clips, y, 64, 1, dev)
    W = np.zeros((4, 33))
    W[0, :] = 1.0                                               # every bin: 33 terms on four lanes
    W[1, 32] = 1.0                                              # Nyquist alone
    W[2, 3:12] = [0.5, 0.0, 0.0, 1.5, 0.25, 0.0, 2.0, 0.0, 1.0]   # zeros inside the span
    W[3, 8:15] = [1.0, 0.0, 3.0, 0.0, 0.0, 0.125, 0.75]         # overlaps band 2
    bank = pca_hip.FilterBank(W, [0.0, 22050.0, 5000.0, 7500.0], power=power, amin=1e-8)
    assert bank.band_off.tolist() == [0, 33, 34, 43, 50]
    farr = bank.centres / FS
    idx = case.idx(3)
    pts, lab, meta = case.bands(idx, bank, farr, want_meta=True, **AUG)
    pts, meta = pts.cpu().numpy(), meta.cpu().numpy()
    assert pts.shape == (idx.size, 4, 2)
    worst = _against_ref(case, idx, pts, meta, bank, farr, 1)
    print(f"frame_points_bands hand-made bank, power {power}: max |delta| {worst:.3e}")
    assert worst <= TOL


# ---- 4. the bank is clipped on the device -----------------------------------------------------------------
def test_bands_are_clipped_on_the_device(corpus, dev):
    import pca_hip
    clips, y = corpus
    case = _Case(clips, y, 64, 2, dev)
    w = np.linspace(0.25, 3.0, 24).astype(np.float32)
    #            starts below 0   inside    wholly above   wholly below   runs past Nyquist, and past nnz
    lo = [-2, 5, 40, -5, 30]
    off = [0, 6, 9, 11, 14, 24 + 7]
    raw = pca_hip.FilterBank.from_packed(lo, off, w, 33, centres=np.arange(5) * 1000.0, power=2, amin=1e-7)
    D = raw.dense()
    assert np.flatnonzero(D[0]).tolist() == [0, 1, 2, 3] and np.flatnonzero(D[4]).tolist() == [30, 31, 32]
    assert not D[2].any() and not D[3].any()
    farr = raw.centres / FS
    idx = case.idx(4)
    pts, _, meta = case.bands(idx, raw, farr, want_meta=True, **AUG)
    # the clipped bank, built from the dense rows that are left
    keep = [0, 1, 4]
    clipped = pca_hip.FilterBank(D[keep], raw.centres[keep], power=2, amin=1e-7)
    assert clipped.band_lo.tolist() == [0, 5, 30] and clipped.band_off.tolist() == [0, 4, 7, 10]
    want, _, want_meta = case.bands(idx, clipped, farr[keep], want_meta=True, **AUG)
    assert torch.equal(meta, want_meta)
    got = pts.reshape(idx.size, 2, 5, 3)
    assert torch.equal(_bits(got[:, :, keep]), _bits(want.reshape(idx.size, 2, 3, 3)))
    # a band that is empty after the clip: logf(amin), whatever the frame holds
    floor = np.float32(np.log(np.float64(np.float32(1e-7))))
    empty = got[:, :, [2, 3], 2].cpu().numpy()
    assert np.abs(empty - floor).max() <= np.spacing(np.abs(floor))
    assert len(np.unique(empty)) == 1
    worst = _against_ref(case, idx, pts.cpu().numpy(), meta.cpu().numpy(), raw, farr, 1)
    print(f"frame_points_bands clipped bank: max |delta| {worst:.3e}")
    assert worst <= TOL


# ---- 5. the draws -----------------------------------------------------------------------------------------
def test_draws_reproduce_and_advance_per_replay(corpus, dev):
    import pca_hip
    clips, y = corpus
    case = _Case(clips, y, 256, 4, dev)
    bank = pca_hip.mel_bank(FS, 256, 16)
    farr = bank.centres / FS
    idx = case.idx(5, clamp=False)[:32].copy()
    aug = dict(jitter=100, gain_db=6.0, seed=5)
    a, _, ma = case.bands(idx, bank, farr, draw=4, want_meta=True, **aug)
    b, _, mb = case.bands(idx, bank, farr, draw=4, want_meta=True, **aug)
    assert torch.equal(_bits(a), _bits(b)) and torch.equal(ma, mb)
    c, _, mc = case.bands(idx, bank, farr, draw=5, want_meta=True, **aug)
    assert not torch.equal(_bits(a), _bits(c)) and not torch.equal(ma[:, 3], mc[:, 3])
    assert torch.equal(ma[:, 0], mc[:, 0])                                # the same clips
    # the device half of the draw number, captured
    out = torch.zeros_like(a)
    lab = torch.zeros(idx.size, dtype=torch.int64, device=dev)
    cnt = torch.zeros(2, dtype=torch.int32, device=dev)
    side = torch.cuda.Stream(dev)
    side.wait_stream(torch.cuda.current_stream(dev))
    with torch.cuda.stream(side):                                         # uploads the bank outside the capture
        case.bands(idx, bank, farr, draw=4, out=out, labels_out=lab, draw_dev=cnt, **aug)
    torch.cuda.current_stream(dev).wait_stream(side)
    torch.cuda.synchronize()
    assert torch.equal(_bits(out), _bits(a))
    idx_dev = torch.from_numpy(idx).to(dev)
    f32 = _f32(farr, dev)
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        pca_hip.frame_points_bands(case.waves, case.woff, case.soff, idx_dev, 256, 128, bank, f32, case.t32, 4,
                                   win_lengths=case.win_dev, draw=4, out=out, labels_out=lab, draw_dev=cnt,
                                   **case.kw, **aug)
    seen = []
    for k in (1, 2):
        cnt[0] = k
        g.replay()
        torch.cuda.synchronize()
        seen.append(out.clone())
        eager, eager_lab = case.bands(idx, bank, farr, draw=4 + k, **aug)
        assert torch.equal(_bits(seen[-1]), _bits(eager)) and torch.equal(lab, eager_lab), k
    assert not torch.equal(_bits(seen[0]), _bits(seen[1]))
    assert torch.equal(_bits(seen[0]), _bits(c))
