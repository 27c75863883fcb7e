"""pca_frame_points_delta on the device: coordinates, value column, labels and meta are the grid or the band
launch's bits; the workspace holds the value column and the context frames, each against the numpy
restatement at the centre ``meta`` gives; the delta columns are tests/delta_ref.py of the workspace, bit for
bit; sets in a stretch of exact zeros have +0.0 deltas; the launch replays, its tickets come back zero, and
a slot does not depend on how many workgroups the launch has."""
import numpy as np
import pytest
import torch

import bands_ref
import delta_ref
import frame_ref
from oracle import st_oracle as orc

pytestmark = pytest.mark.gpu

FS = 44100
TOL = 5e-5          # the bar of test_gpu_frame_points.py and test_gpu_frame_points_bands.py: the same fp64
#                     transform on both sides
JITTER = 37
ZERO = (3000, 5200)   # clip 2's stretch of exact zeros
AUG = dict(jitter=JITTER, gain_db=6.0, norm_mode=1, seed=11, draw=5)


@pytest.fixture(scope="module")
def dev():
    return torch.device("cuda", 0)


@pytest.fixture(scope="module")
def corpus():
    """test_gpu_frame_points_bands.py's corpus: five clips of 0.05 .. 0.5 s, one with a stretch of exact zeros;
    one label per clip."""
    secs = (0.05, 0.11, 0.2, 0.3667, 0.5)
    clips = [orc.synth_clip(40 + i, 3 * i + 1, seconds=s) for i, s in enumerate(secs)]
    clips[2] = clips[2].copy()
    clips[2][ZERO[0]:ZERO[1]] = 0.0
    return clips, np.array([4, 9, 2, 7, 5])


def _bits(t):
    return t.contiguous().view(torch.int32)


def _f32(a, dev):
    return torch.as_tensor(np.asarray(a, dtype=np.float64)).float().to(dev)


CASES = {   # n_fft, Nt, 3-D rows, bank (None: grid) as (n_mels, power), grid bins, axes, W
    "a-64-2d-grid33-tf-W2": (64, 1, False, None, 33, "tf", 2),
    "b-256-Nt4-grid128-t-W1": (256, 4, True, None, 128, "t", 1),
    "c-1024-Nt2-mel128-t-W4": (1024, 2, True, (128, 1), None, "t", 4),
    "d-256-2d-mel16-f-W3": (256, 1, False, (16, 2), None, "f", 3),
    "e-1024-2d-grid513-t-W1": (1024, 1, False, None, 513, "t", 1),
}


class _Case:
    """The resident corpus, the axes and the spec of one case, as the datasets lay them out."""

    def __init__(self, name, clips, y, dev):
        import dataset
        import pca_hip
        n_fft, Nt, three, bank, n_bins, axes, W = CASES[name]
        self.name, self.clips, self.y, self.dev = name, clips, y, dev
        self.n_fft, self.hop, self.Nt = n_fft, n_fft // 2, Nt
        self.spec = pca_hip.Deltas(axes, W)
        self.Wt, self.T = self.spec.context, Nt + 2 * self.spec.context
        self.bank = None if bank is None else pca_hip.mel_bank(FS, n_fft, bank[0], power=bank[1])
        self.F = n_bins if bank is None else bank[0]
        self.W = None if bank is None else self.bank.dense()    # the fp32 weights the device applies, fp64
        self.farr = np.linspace(0, FS / 2, self.F) / FS if bank is None else self.bank.centres / FS
        self.f32 = _f32(self.farr, dev)
        self.din0 = 3 if three else 2
        self.din = self.din0 + len(axes)
        lens = [len(c) for c in clips]
        self.set_off = dataset.wave_set_offsets(lens, self.hop, Nt)
        i64 = lambda a: torch.as_tensor(np.asarray(a, dtype=np.int64)).to(dev)   # noqa: E731
        self.waves = torch.cat([torch.from_numpy(c).to(dev) for c in clips])
        self.woff, self.soff, self.lab = i64([0] + list(np.cumsum(lens))), i64(self.set_off), i64(y)
        self.kw = dict(max_len=max(lens), min_len=min(lens), clip_labels=self.lab)
        self.tarr = np.linspace(0, self.hop / FS * Nt, Nt) if three else None
        self.t32 = _f32(self.tarr, dev) if three else None
        self.wins = (n_fft, n_fft * 3 // 4)
        self.win_dev = torch.tensor(self.wins, dtype=torch.int32, device=dev)

    def zero_sets(self):
        """The sets of clip 2 (as corpus ids) whose T frames, whatever the shift, read zeros only."""
        out = []
        for s in range(self.set_off[3] - self.set_off[2]):
            lo = (s * self.Nt - self.Wt) * self.hop - self.n_fft // 2 - JITTER
            hi = (s * self.Nt + self.Nt - 1 + self.Wt) * self.hop + self.n_fft // 2 + JITTER   # one past the last
            if lo >= ZERO[0] and hi <= ZERO[1]:
                out.append(self.set_off[2] + s)
        return out

    def idx(self, seed):
        """First and last set of every clip, (up to three of) the sets inside the zero stretch, a shuffle with
        repeats and two ids out of range (clamped on the device)."""
        n = self.set_off[-1]
        rng = np.random.Generator(np.random.PCG64(seed))
        parts = [self.set_off[:-1], np.asarray(self.set_off[1:]) - 1, self.zero_sets()[:3],
                 rng.permutation(n)[:12], rng.integers(0, n, size=6), [-3, n + 5]]
        return np.concatenate([np.asarray(p, dtype=np.int64) for p in parts])

    def workspace(self, B):
        return (torch.full((B, self.T, self.F), float("nan"), dtype=torch.float32, device=self.dev),
                torch.zeros(B, dtype=torch.int32, device=self.dev))

    def delta(self, idx, ws, **kw):
        import pca_hip
        return pca_hip.frame_points_delta(self.waves, self.woff, self.soff, torch.from_numpy(idx).to(self.dev),
                                          self.n_fft, self.hop, self.F, self.f32, self.t32, self.Nt,
                                          deltas=self.spec, bank=self.bank, win_lengths=self.win_dev,
                                          workspace=ws, **self.kw, **kw)

    def base(self, idx, **kw):
        """The launch whose rows the deltas ride on."""
        import pca_hip
        i = torch.from_numpy(idx).to(self.dev)
        if self.bank is None:
            return pca_hip.frame_points(self.waves, self.woff, self.soff, i, self.n_fft, self.hop, self.F,
                                        self.f32, self.t32, self.Nt, win_lengths=self.win_dev, **self.kw, **kw)
        return pca_hip.frame_points_bands(self.waves, self.woff, self.soff, i, self.n_fft, self.hop, self.bank,
                                          self.f32, self.t32, self.Nt, win_lengths=self.win_dev, **self.kw, **kw)

    def ref_values(self, wave, centres, win, gain):
        """float32 [len(centres), F]: the restated value column of the frames at ``centres`` (norm_mode 1)."""
        if self.bank is None:
            return np.stack([frame_ref.frame_ref(wave, c, self.n_fft, win, gain, win, self.F) for c in centres])
        return bands_ref.band_values(wave, centres, self.n_fft, win, gain, win, self.W,
                                     self.bank.power, self.bank.amin)


_RUNS = {}


@pytest.fixture
def run(request, corpus, dev):
    """One launch per case, shared by the checks: (case, idx, points, labels, meta, workspace), on the host."""
    name = request.param
    if name not in _RUNS:
        clips, y = corpus
        case = _Case(name, clips, y, dev)
        idx = case.idx(1)
        ws = case.workspace(idx.size)
        pts, lab, meta = case.delta(idx, ws, want_meta=True, **AUG)
        torch.cuda.synchronize()
        assert int(ws[1].abs().sum()) == 0                              # the tickets are zero again
        _RUNS[name] = (case, idx, pts, lab, meta, ws[0].cpu().numpy())
    return _RUNS[name]


def _gain(meta_row):
    return np.array([meta_row[3]], dtype=np.int32).view(np.float32)[0]


# ---- 1. coordinates, value, labels and meta are the base launch's -----------------------------------------
@pytest.mark.parametrize("run", list(CASES), indirect=True)
def test_base_columns_labels_and_meta_are_the_base_launch(run):
    case, idx, pts, lab, meta, _ = run
    want, want_lab, want_meta = case.base(idx, want_meta=True, **AUG)
    assert tuple(pts.shape) == (idx.size, case.Nt * case.F, case.din)
    assert tuple(want.shape) == (idx.size, case.Nt * case.F, case.din0)
    assert torch.equal(_bits(pts[:, :, :case.din0]), _bits(want))
    assert torch.equal(lab, want_lab) and torch.equal(meta, want_meta)
    assert bool(torch.isfinite(pts).all())
    m = meta.cpu().numpy()
    assert np.array_equal(lab.cpu().numpy(), case.y[m[:, 0]])
    assert set(m[:, 2].tolist()) == set(case.wins) and len(set(m[:, 3].tolist())) > 16   # the augmentation is on


# ---- 2. the workspace: the value column, and every frame against the restatement --------------------------
@pytest.mark.parametrize("run", list(CASES), indirect=True)
def test_workspace_rows_against_numpy(run):
    case, idx, pts, _, meta, ws = run
    pts, meta = pts.cpu().numpy(), meta.cpu().numpy()
    Nt, F, Wt, T, hop = case.Nt, case.F, case.Wt, case.T, case.hop
    assert ws.shape == (idx.size, T, F) and np.isfinite(ws).all()
    own = ws[:, Wt:Wt + Nt].reshape(idx.size, Nt * F)
    assert np.array_equal(own.view(np.int32), pts[:, :, case.din0 - 1].view(np.int32))
    total, worst, both_ends = case.set_off[-1], 0.0, 0
    for b, i in enumerate(idx):
        i = min(max(int(i), 0), total - 1)
        c, centre0, win, _ = (int(v) for v in meta[b])
        assert case.set_off[c] <= i < case.set_off[c + 1] and win in case.wins
        wave, L, s = case.clips[c], len(case.clips[c]), i - case.set_off[c]
        nominal = s * Nt * hop
        # the shifts that explain frame 0's centre: one, unless the clamp to [0, L] took hold of it
        shifts = [d for d in range(-JITTER, JITTER + 1) if min(max(nominal + d, 0), L) == centre0]
        assert shifts and (len(shifts) == 1 or centre0 in (0, L)), (b, centre0, nominal)
        errs = []
        for d in shifts:
            centres = delta_ref.slot_centres(L, s, d, Nt, hop, Wt)
            assert centres[Wt] == centre0 and len(centres) == T
            want = case.ref_values(wave, centres, win, _gain(meta[b]))
            errs.append(float(np.abs(ws[b].astype(np.float64) - want).max()))
            if d == shifts[0] and centres[0] == 0 and centres[-1] == L and T > 1:
                both_ends += 1
        worst = max(worst, min(errs))
    print(f"frame_points_delta {case.name}: max |delta| of the workspace {worst:.3e} over {idx.size} slots x {T} "
          f"frames, {both_ends} slots with context clamped at both ends")
    assert worst <= TOL
    if Wt > 0:        # the first and the last set of the 0.05 s clip are in the batch: clamped context
        L0, last = len(case.clips[0]), case.set_off[1] - 1
        assert idx[0] == 0 and idx[5] == last
        ends = [delta_ref.slot_centres(L0, s, 0, Nt, hop, Wt) for s in (0, last)]
        assert ends[0][0] == 0 and ends[0][Wt] == 0                         # context before the clip's start
        if case.name.startswith("c-"):                                      # context longer than the set: both ends
            assert all(cs[0] == 0 and cs[-1] == L0 for cs in ends) and both_ends >= 2


# ---- 3. the delta columns are the restatement of the workspace, bit for bit -------------------------------
@pytest.mark.parametrize("run", list(CASES), indirect=True)
def test_delta_columns_are_the_restatement_bit_for_bit(run):
    case, idx, pts, _, _, ws = run
    pts = pts.cpu().numpy()
    k = len(case.spec.axes)
    for b in range(idx.size):
        want = delta_ref.deltas(ws[b], case.Nt, case.spec.axes, case.spec.width).reshape(case.Nt * case.F, k)
        got = pts[b][:, case.din0:]
        assert got.shape == want.shape
        assert np.array_equal(got.view(np.int32), want.view(np.int32)), (case.name, b)
    d = pts[:, :, case.din0:]
    assert np.abs(d).max() > 1e-3                                       # the deltas are not all small


# ---- 4. sets inside the zero stretch: +0.0 ----------------------------------------------------------------
@pytest.mark.parametrize("run", list(CASES), indirect=True)
def test_sets_in_the_zero_stretch_have_zero_deltas(run):
    case, idx, pts, _, meta, ws = run
    zero = case.zero_sets()
    if case.name.startswith("c-"):
        # 10 frames of n_fft 1024, 512 apart, span 5632 samples: no set fits into 2200 zeros
        assert zero == [] and (case.T + 1) * case.hop > ZERO[1] - ZERO[0]
        return
    assert len(zero) >= 1, case.name
    slots = np.arange(10, 10 + min(len(zero), 3))
    assert np.array_equal(idx[slots], zero[:3])
    m = meta.cpu().numpy()
    assert (m[slots, 0] == 2).all()
    d = pts[torch.from_numpy(slots).to(pts.device)][:, :, case.din0:]
    assert not bool(_bits(d).any())                                     # +0.0: no bit set
    assert len(np.unique(ws[slots])) == 1                               # every frame of the slot is silent


# ---- 5. replay ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["b-256-Nt4-grid128-t-W1", "c-1024-Nt2-mel128-t-W4"])
def test_replay(name, corpus, dev):
    import pca_hip
    clips, y = corpus
    case = _Case(name, clips, y, dev)
    idx = case.idx(5)[:32].copy()
    B = idx.size
    ws = case.workspace(B)
    aug = dict(jitter=100, gain_db=6.0, seed=5)
    a, _, ma = case.delta(idx, ws, draw=4, want_meta=True, **aug)
    assert int(ws[1].abs().sum()) == 0 and bool(torch.isfinite(ws[0]).all())
    ws[0].fill_(float("nan"))                                           # nothing stale is read
    b, _, mb = case.delta(idx, ws, draw=4, want_meta=True, **aug)
    assert torch.equal(_bits(a), _bits(b)) and torch.equal(ma, mb) and int(ws[1].abs().sum()) == 0
    c, _, mc = case.delta(idx, ws, draw=5, want_meta=True, **aug)
    assert int(ws[1].abs().sum()) == 0
    assert not torch.equal(_bits(a), _bits(c)) and not torch.equal(ma[:, 3], mc[:, 3])
    assert torch.equal(ma[:, 0], mc[:, 0])                              # the same clips
    # the device half of the draw number, captured: the tickets need no memset node
    eager = [case.delta(idx, ws, draw=4 + k, **aug) for k in (1, 2, 3)]
    eager = [(p.clone(), l.clone()) for p, l in eager]
    out = torch.zeros_like(a)
    lab = torch.zeros(B, dtype=torch.int64, device=dev)
    cnt = torch.zeros(2, dtype=torch.int32, device=dev)
    idx_dev = torch.from_numpy(idx).to(dev)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        pca_hip.frame_points_delta(case.waves, case.woff, case.soff, idx_dev, case.n_fft, case.hop, case.F,
                                   case.f32, case.t32, case.Nt, deltas=case.spec, bank=case.bank,
                                   win_lengths=case.win_dev, workspace=ws, draw=4, out=out, labels_out=lab,
                                   draw_dev=cnt, **case.kw, **aug)
    for k in (1, 2, 3):
        cnt[0] = k
        out.zero_()
        ws[0].fill_(float("nan"))
        g.replay()
        torch.cuda.synchronize()
        assert torch.equal(_bits(out), _bits(eager[k - 1][0])) and torch.equal(lab, eager[k - 1][1]), k
        assert int(ws[1].abs().sum()) == 0, k
    assert torch.equal(_bits(eager[0][0]), _bits(c)) and not torch.equal(_bits(eager[0][0]), _bits(eager[1][0]))


# ---- 6. far more workgroups than can be resident ------------------------------------------------------------
def test_slots_do_not_depend_on_the_size_of_the_launch(corpus, dev):
    """Case a with B = 600: 3000 workgroups.  The first 40 slots are a B = 40 launch of the same ids, bit for
    bit: a slot depends neither on which workgroups are resident nor on the order they arrive in."""
    clips, y = corpus
    case = _Case("a-64-2d-grid33-tf-W2", clips, y, dev)
    base = case.idx(7)
    idx = np.concatenate([base] * (600 // base.size + 1))[:600].copy()
    assert idx.size == 600 and case.T * idx.size == 3000
    big_ws, small_ws = case.workspace(600), case.workspace(40)
    big, big_lab, big_meta = case.delta(idx, big_ws, want_meta=True, **AUG)
    small, small_lab, small_meta = case.delta(idx[:40].copy(), small_ws, want_meta=True, **AUG)
    assert int(big_ws[1].abs().sum()) == 0 and int(small_ws[1].abs().sum()) == 0
    assert bool(torch.isfinite(big).all()) and bool(torch.isfinite(big_ws[0]).all())
    assert torch.equal(_bits(big[:40]), _bits(small))
    assert torch.equal(big_lab[:40], small_lab) and torch.equal(big_meta[:40], small_meta)
    assert torch.equal(_bits(big_ws[0][:40]), _bits(small_ws[0]))
    # and every slot of the big launch is the restatement of its own workspace
    ws, pts = big_ws[0].cpu().numpy(), big.cpu().numpy()
    for b in range(0, 600, 7):
        want = delta_ref.deltas(ws[b], 1, "tf", 2).reshape(case.F, 2)
        assert np.array_equal(pts[b][:, 2:].view(np.int32), want.view(np.int32)), b
