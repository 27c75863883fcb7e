"""pca_frame_points_ex / pca_clip_rms and the speed / mix options of dataset.ESC_wave_pc[_temp] on the
device: with both off the call is pca_frame_points bit for bit; with either on the samples every frame
was built from (``want_samples``) are the resampled clip (pca_hip.resample) plus the scaled background that
``meta`` reports, and the points are the numpy frame of those samples; the draws are uniform, reproducible
and advance per replay of a captured training step."""
import numpy as np
import pytest
import torch

from frame_aug_ref import aug_samples, frame_of_samples
from oracle import st_oracle as orc
from test_gpu_trainer_eval import _net, _resume_case, _state

pytestmark = pytest.mark.gpu

FS = 44100
TOL = 5e-5          # test_stft_logmag_vs_oracle's bar: the same fp64 arithmetic on both sides
JIT = 37


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


@pytest.fixture(scope="module")
def backgrounds():
    """Three separate short clips, one shorter than n_fft = 256: its wrap-around runs twice per frame."""
    rng = np.random.Generator(np.random.PCG64(8))
    return [orc.synth_clip(60, 2, seconds=0.03), (0.3 * rng.standard_normal(100)).astype(np.float32),
            orc.synth_clip(61, 8, seconds=0.08)]


def _dataset(clips, y, dev, ntemp, n_fft=256, **kw):
    import dataset
    if ntemp == 1:
        return dataset.ESC_wave_pc(clips, y, FS, n_fft, device=dev, **kw)
    return dataset.ESC_wave_pc_temp(clips, y, FS, n_fft, ntemp, device=dev, **kw)


def _ends_and_random(ds, seed, n=64):
    """First and last set of every clip (where the clamp and both reflections act), then random ones."""
    rng = np.random.Generator(np.random.PCG64(seed))
    ends = np.concatenate([ds.set_off[:-1], np.asarray(ds.set_off[1:]) - 1])
    return np.concatenate([ends, rng.integers(0, len(ds), size=n - ends.size)])


def _f32(bits):
    return np.array([bits], dtype=np.int32).view(np.float32)[0]


def _bits(t):
    return t.view(torch.int32)


# ---- 1. off is pca_frame_points, bit for bit ------------------------------------------------------------
@pytest.mark.parametrize("n_fft,ntemp", [(256, 1), (256, 3), (64, 1), (4096, 1)],
                         ids=["256-din2", "256-din3", "64", "4096-lds-opt-in"])
def test_off_is_frame_points_bit_for_bit(n_fft, ntemp, corpus, dev):
    import pca_hip
    clips, y = corpus
    if n_fft == 4096:
        clips, y = clips[4:], y[4:]                                      # the 0.5 s clip: 11 frames
    ds = _dataset(clips, y, dev, ntemp, n_fft)
    waves, woff, soff, f32, t32, lab = ds._resident()
    idx = (torch.tensor([3, 10], device=dev) if n_fft == 4096
           else torch.from_numpy(_ends_and_random(ds, 1)).to(dev))
    wins = torch.tensor([n_fft // 2, 200 * n_fft // 256, n_fft], dtype=torch.int32, device=dev)
    kw = dict(max_len=ds._max_len, min_len=ds._min_len, clip_labels=lab, jitter=JIT, gain_db=6.0,
              win_lengths=wins, seed=11, draw=4, want_meta=True)
    args = (waves, woff, soff, idx, n_fft, ds.hop, ds.F, f32, t32, ntemp)
    want, want_lab, want_meta = pca_hip.frame_points(*args, **kw)
    got, got_lab, meta = pca_hip.frame_points_ex(*args, ratios=(1.0,), **kw)
    assert meta.shape == (idx.numel(), 8) and got.shape == want.shape
    assert torch.equal(_bits(got), _bits(want)) and torch.equal(got_lab, want_lab)
    assert torch.equal(meta[:, :4], want_meta)
    assert (meta[:, 4] == 0).all() and (meta[:, 5] == -1).all()
    assert idx.numel() == 2 or len(set(want_meta[:, 2].tolist())) == 3    # the draws were on
    # ... and so is the loop that also hands the samples out
    again, _, _, samples = pca_hip.frame_points_ex(*args, ratios=(1.0,), want_samples=True, **kw)
    assert torch.equal(_bits(again), _bits(want)) and samples.shape == (idx.numel(), ntemp, n_fft)


# ---- 2. clip_rms ----------------------------------------------------------------------------------------
def test_clip_rms(corpus, dev):
    import pca_hip
    clips, _ = corpus
    clips = list(clips) + [np.zeros(777, dtype=np.float32), clips[0][:1], clips[1][:255], clips[1][:257]]
    lens = [len(c) for c in clips]
    waves = torch.from_numpy(np.concatenate(clips)).to(dev)
    woff = torch.from_numpy(np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)).to(dev)
    got = pca_hip.clip_rms(waves, woff, max(lens))
    assert got.dtype == torch.float64 and got.shape == (len(clips),)
    assert torch.equal(got, pca_hip.clip_rms(waves, woff, max(lens)))
    got = got.cpu().numpy()
    want = np.array([np.sqrt(np.mean(c.astype(np.float64) ** 2)) for c in clips])
    rel = np.abs(got - want) / np.where(want > 0, want, 1.0)
    print("clip_rms relative error", rel.tolist())
    assert got[5] == 0.0                                                  # the all-zero clip: exactly
    assert rel.max() <= 1e-10


# ---- the check shared by 3, 4 and 5 -----------------------------------------------------------------------
class _Resampled:
    """pca_hip.resample(clip, fs_old=speed, fs_new=1.0, scale=False)[:int(L * ratio)], once per pair."""

    def __init__(self, ds, clips, dev):
        self.ds, self.clips, self.dev, self.cache = ds, clips, dev, {}

    def __call__(self, c, si):
        import pca_hip
        if (c, si) not in self.cache:
            speed, ratio = self.ds.speeds[si], self.ds.ratios[si]
            y = pca_hip.resample(torch.from_numpy(self.clips[c]).to(self.dev), speed, 1.0, scale=False)
            if ratio == 1.0:
                assert np.array_equal(y.cpu().numpy(), self.clips[c])
            self.cache[c, si] = y.cpu().numpy()[:int(len(self.clips[c]) * ratio)]
        return self.cache[c, si]


def _check_slots(ds, clips, bgs, idx, pts, meta, samples, jitter, dev):
    """Every frame of every slot against what ``meta`` reports: (a) the centre, (b) the samples, (c) the
    points.  Returns (worst sample error in ulps of the frame's peak, all samples bit-equal, worst point
    error)."""
    n_fft, hop, F, Nt = ds.n_fft, ds.hop, ds.F, ds._ntemp
    resampled = _Resampled(ds, clips, dev)
    worst_ulp, bit_equal, worst_pt = 0.0, True, 0.0
    for b, i in enumerate(idx):
        c, centre0, win, _, si, c2, p, _ = (int(v) for v in meta[b])
        g, alpha = _f32(meta[b, 3]), _f32(meta[b, 7])
        assert ds.set_off[c] <= i < ds.set_off[c + 1] and win in ds.win_lengths
        assert 0 <= si < len(ds.speeds)
        ratio, L = ds.ratios[si], len(clips[c])
        y = resampled(c, si)
        Ly = len(y)
        assert Ly == int(L * ratio)
        nominal = (i - ds.set_off[c]) * Nt * hop

        def q0(d):                                                        # frame 0's centre before the clamp
            return nominal + d if ratio == 1.0 else int(np.floor((nominal + d) * ratio + 0.5))

        # (a) within 1 of clamp(round((s Nt hop + d) ratio), 0, Ly) for some |d| <= jitter
        cands = sorted({q0(d) for d in range(-jitter, jitter + 1)})
        assert min(abs(centre0 - min(max(q, 0), Ly)) for q in cands) <= 1, (b, centre0, cands[0], cands[-1])
        # frame 0 clamped at the clip's start hides the shift the chunk's other frames still carry: one of
        # the shifts that clamp there must explain them
        firsts = [centre0] if (centre0 > 0 or Nt == 1) else [q for q in cands if q <= 0]
        bg = None if c2 < 0 else bgs[c2]
        if c2 < 0:
            assert alpha == 0 and p == 0
        else:
            assert 0 <= p < len(bg)
        norm = n_fft if ds.norm == "n_fft" else win
        got_pts = pts[b].reshape(Nt, F, -1)[:, :, -1]
        best = None
        for first in firsts:
            ulps, same = 0.0, True
            for j in range(Nt):
                cj = min(max(first + j * hop, 0), Ly)
                want = aug_samples(y, cj, n_fft, bg, p + j * hop, alpha)
                peak = max(float(np.abs(want).max()), float(np.finfo(np.float32).tiny))
                err = float(np.abs(samples[b, j].astype(np.float64) - want.astype(np.float64)).max())
                ulps = max(ulps, err / float(np.spacing(np.float32(peak))))
                same = same and np.array_equal(samples[b, j].view(np.int32), want.view(np.int32))
            if best is None or ulps < best[0]:
                best = (ulps, same)
        worst_ulp, bit_equal = max(worst_ulp, best[0]), bit_equal and best[1]
        # (c) the points are the frame of those samples: the same fp64 arithmetic on the same fp32 samples
        for j in range(Nt):
            ref = frame_of_samples(samples[b, j], win, g, norm, F)
            worst_pt = max(worst_pt, float(np.abs(got_pts[j] - ref).max()))
    return worst_ulp, bit_equal, worst_pt


def _run(ds, idx, dev):
    pts, lab, meta, samples = ds.batch(torch.from_numpy(idx).to(dev), want_meta=True, want_samples=True)
    assert meta.shape == (idx.size, 8) and samples.shape == (idx.size, ds._ntemp, ds.n_fft)
    pts, meta, samples = pts.cpu().numpy(), meta.cpu().numpy(), samples.cpu().numpy()
    assert np.isfinite(pts).all()
    assert np.array_equal(lab.cpu().numpy(), ds.clip_labels[meta[:, 0]])
    return pts, meta, samples


# ---- 3. speed alone -------------------------------------------------------------------------------------
@pytest.mark.parametrize("ntemp", [1, 3], ids=["din2", "din3"])
def test_speed_against_resample_and_numpy(ntemp, corpus, dev):
    clips, y = corpus
    ds = _dataset(clips, y, dev, ntemp, speeds=(1.0, 0.8, 1.25), jitter=JIT, seed=11)
    assert ds.stochastic
    idx = _ends_and_random(ds, 5)
    pts, meta, samples = _run(ds, idx, dev)
    assert set(meta[:, 4].tolist()) == {0, 1, 2}                           # all three speeds occur
    assert (meta[:, 5] == -1).all() and (meta[:, 7] == 0).all()
    # both ends of every clip at a ratio other than 1
    assert (meta[:10, 4] != 0).sum() >= 3
    ulps, same, worst = _check_slots(ds, clips, None, idx, pts, meta, samples, JIT, dev)
    print(f"speed, din {2 if ntemp == 1 else 3}: samples vs pca_hip.resample {ulps:.3f} ulp of the peak "
          f"(bit-equal: {same}); points vs numpy max |delta| {worst:.3e}")
    assert ulps <= 1.0
    assert worst < TOL


# ---- 4. mix alone ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("ntemp", [1, 3], ids=["din2", "din3"])
def test_mix_against_numpy(ntemp, corpus, backgrounds, dev):
    clips, y = corpus
    ds = _dataset(clips, y, dev, ntemp, mix_clips=backgrounds, mix_prob=0.5, mix_snr_db=(0.0, 20.0), seed=12)
    assert ds.stochastic and min(len(b) for b in backgrounds) < ds.n_fft
    idx = _ends_and_random(ds, 6)
    pts, meta, samples = _run(ds, idx, dev)
    rms, _, _, bg_rms, _ = ds._mix_resident()
    rms, bg_rms = rms.cpu().numpy(), bg_rms.cpu().numpy()
    mixed = meta[:, 5] >= 0
    assert 16 <= mixed.sum() <= 48 and set(meta[mixed, 5].tolist()) == {0, 1, 2}
    assert (meta[:, 4] == 0).all()
    for b in np.nonzero(mixed)[0]:
        c, c2, alpha = meta[b, 0], meta[b, 5], _f32(meta[b, 7])
        assert alpha > 0
        snr = -20.0 * np.log10(float(alpha) * bg_rms[c2] / rms[c])        # the SNR the reported scale implies
        assert -1e-5 <= snr <= 20.0 + 1e-5, (b, snr)                      # fp32 rounding of alpha: 5e-7 dB
    ulps, same, worst = _check_slots(ds, clips, backgrounds, idx, pts, meta, samples, 0, dev)
    print(f"mix, din {2 if ntemp == 1 else 3}: samples vs numpy {ulps:.3f} ulp of the peak (bit-equal: {same}); "
          f"points vs numpy max |delta| {worst:.3e}")
    assert ulps <= 1.0
    assert worst < TOL
    # a slot that does not mix is the unmixed frame, bit for bit
    plain = ds.plain().batch(torch.from_numpy(idx).to(dev))[0].cpu().numpy()
    assert np.array_equal(pts[~mixed].view(np.int32), plain[~mixed].view(np.int32))
    assert all(not np.array_equal(pts[b], plain[b]) for b in np.nonzero(mixed)[0])


def test_mix_self_with_a_silent_clip(corpus, dev):
    clips, y = corpus
    clips = [clips[0], np.zeros(3000, dtype=np.float32), clips[1]]
    ds = _dataset(clips, y[:3], dev, 1, mix_clips="self", mix_prob=1.0, mix_snr_db=(3.0, 3.0), seed=2)
    idx = np.arange(len(ds))
    pts, meta, samples = _run(ds, idx, dev)
    assert (meta[:, 5] >= 0).all()                                        # every slot mixes
    silent = (meta[:, 0] == 1) | (meta[:, 5] == 1)                        # either RMS is 0
    assert (meta[:, 0] == 1).sum() >= 10 and (meta[:, 5] == 1).sum() >= 10 and (~silent).sum() >= 10
    assert (meta[silent, 7] == 0).all() and (meta[~silent, 7] != 0).all()
    plain = ds.plain().batch(torch.from_numpy(idx).to(dev))[0].cpu().numpy()
    assert np.array_equal(pts[silent].view(np.int32), plain[silent].view(np.int32))
    assert all(not np.array_equal(pts[b], plain[b]) for b in np.nonzero(~silent)[0])
    rms = ds._mix_resident()[0].cpu().numpy()
    assert rms[1] == 0.0
    for b in np.nonzero(~silent)[0]:                                      # SNR 3 dB exactly
        want = np.float32(rms[meta[b, 0]] / rms[meta[b, 5]] * 10.0 ** (-3.0 / 20.0))
        assert abs(float(_f32(meta[b, 7])) / float(want) - 1.0) < 1e-6


# ---- 5. both, with shift, gain and window draws too -------------------------------------------------------
def test_speed_and_mix_with_every_draw_on(corpus, backgrounds, dev):
    clips, y = corpus
    ds = _dataset(clips, y, dev, 3, speeds=(1.0, 0.8, 1.25), mix_clips=backgrounds, mix_prob=0.5,
                  mix_snr_db=(0.0, 20.0), jitter=JIT, gain_db=6.0, win_lengths=(128, 200, 256), norm="win",
                  seed=13)
    idx = _ends_and_random(ds, 7)
    pts, meta, samples = _run(ds, idx, dev)
    both = (meta[:, 4] != 0) & (meta[:, 5] >= 0)
    assert both.sum() >= 8 and len(set(meta[:, 2].tolist())) == 3 and len(set(meta[:, 3].tolist())) > 32
    ulps, same, worst = _check_slots(ds, clips, backgrounds, idx, pts, meta, samples, JIT, dev)
    print(f"speed + mix, din 3: samples {ulps:.3f} ulp of the peak (bit-equal: {same}); "
          f"points vs numpy max |delta| {worst:.3e}")
    assert ulps <= 1.0
    assert worst < TOL


# ---- 6. the draws ---------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def long_clip():
    return [orc.synth_clip(77, 6, seconds=0.5)], np.array([6])


def _draw_ds(long_clip, backgrounds, dev, **kw):
    clips, y = long_clip
    args = dict(jitter=8, gain_db=6.0, win_lengths=(32, 48, 64), seed=21, speeds=(1.0, 0.8, 1.25),
                mix_clips=backgrounds, mix_prob=0.5)
    args.update(kw)
    return _dataset(clips, y, dev, 1, 64, **args)


def _batch_at(ds, idx, draw, **kw):
    ds._draw = draw - 1                                                   # batch() advances it first
    return ds.batch(idx, want_meta=True, **kw)


def _within_5_sigma(count, n, p, what):
    bound = 5.0 * np.sqrt(n * p * (1.0 - p))
    print(f"{what}: {count} of {n}, expected {n * p:.1f} +- {bound:.1f}")
    assert abs(count - n * p) <= bound, what


def test_draws_are_uniform_and_reproducible(long_clip, backgrounds, dev):
    ds = _draw_ds(long_clip, backgrounds, dev)
    n = len(ds)
    assert n == 690
    slots = 4096
    idx = torch.arange(slots, device=dev) % n
    pts, _, meta = _batch_at(ds, idx, 3)
    m = meta.cpu().numpy()
    for k in range(3):
        _within_5_sigma(int((m[:, 4] == k).sum()), slots, 1.0 / 3.0, f"speed index {k}")
    mixed = m[:, 5] >= 0
    n_mixed = int(mixed.sum())
    _within_5_sigma(n_mixed, slots, 0.5, "mix decision")
    for k in range(3):
        sel = mixed & (m[:, 5] == k)
        _within_5_sigma(int(sel.sum()), n_mixed, 1.0 / 3.0, f"background clip {k}")
        bucket = (m[sel, 6].astype(np.int64) * 8) // len(backgrounds[k])
        assert bucket.min() >= 0 and bucket.max() <= 7
        for q in range(8):
            lo, hi = -(-q * len(backgrounds[k]) // 8), -(-(q + 1) * len(backgrounds[k]) // 8)
            _within_5_sigma(int((bucket == q).sum()), int(sel.sum()), (hi - lo) / len(backgrounds[k]),
                            f"start bucket {q} of background {k}")
    assert (m[~mixed, 6] == 0).all() and (m[~mixed, 7] == 0).all()
    # the same set in two slots of one call: independent draws
    assert not np.array_equal(m[:n, 4:], m[n:2 * n, 4:])

    again, _, meta2 = _batch_at(ds, idx, 3)
    assert torch.equal(_bits(again), _bits(pts)) and torch.equal(meta2, meta)
    other, _, meta3 = _batch_at(ds, idx, 4)
    assert not torch.equal(meta3[:, 4:], meta[:, 4:]) and not torch.equal(_bits(other), _bits(pts))
    seeded, _, meta4 = _batch_at(_draw_ds(long_clip, backgrounds, dev, seed=22), idx, 3)
    assert not torch.equal(meta4[:, 4:], meta[:, 4:]) and not torch.equal(_bits(seeded), _bits(pts))
    # the device half of the draw number
    two = torch.tensor([2, 0], dtype=torch.int32, device=dev)
    a, _, ma = _batch_at(ds, idx, 5, draw_dev=two)
    b, _, mb = _batch_at(ds, idx, 7)
    assert torch.equal(_bits(a), _bits(b)) and torch.equal(ma, mb)

    # draws 0 - 2 do not move when speed or mix is switched on
    _, _, base = _batch_at(_draw_ds(long_clip, backgrounds, dev, speeds=None, mix_prob=0.0), idx, 3)
    assert base.shape == (slots, 4)                                       # today's call
    _, _, mix_only = _batch_at(_draw_ds(long_clip, backgrounds, dev, speeds=(1.0,)), idx, 3)
    assert mix_only.shape == (slots, 8) and torch.equal(mix_only[:, 1:4], base[:, 1:4])
    assert torch.equal(mix_only[:, 5:], meta[:, 5:])                      # nor do draws 4 - 7 depend on speed
    # with speed on, window and gain stay; the centre is the same shift seen through the slot's ratio
    assert torch.equal(meta[:, 2:4], base[:, 2:4])
    at_one = (m[:, 4] == 0)
    assert np.array_equal(m[at_one, 1], base.cpu().numpy()[at_one, 1])


# ---- 7. through the Trainer -----------------------------------------------------------------------------
def _train_clips(lengths):
    return [orc.synth_clip(90 + i, 2 * i, seconds=n / FS)[:n] for i, n in enumerate(lengths)]


@pytest.mark.parametrize("graph", [True, False], ids=["hipgraph", "eager"])
def test_trainer_draws_afresh_resumes_and_evaluates(dev, tmp_path, graph):
    import dataset
    from pca_hip import _lib, trainer
    new = dict(speeds=(1.0, 0.9, 1.1), mix_clips="self", mix_prob=0.5)
    kw_ds = dict(drop_nyquist=True, device=dev)                           # n_fft 512: N = 256
    kw_tr = dict(batch_size=16, mode=_lib.MODE_BF16)

    # (a) one batch of 16 sets, the same indices every step: the packed batch still changes
    clips = _train_clips([4000])
    ds = dataset.ESC_wave_pc(clips, [3], FS, 512, seed=9, **new, **kw_ds)
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
    lengths = [3000, 5200, 4100, 6000]                                    # 12 + 21 + 17 + 24 = 74 sets
    y = [1, 8, 3, 6]

    def make(**opts):
        d = dataset.ESC_wave_pc(_train_clips(lengths), y, FS, 512, seed=9, **opts, **kw_ds)
        assert len(d) == 74                                               # 4 steps per epoch
        return _net(dev, 2, seed=4), d, dict(seed=5, **kw_tr)

    _resume_case(lambda: make(**new), 3, tmp_path, graph=graph)

    # (c) the held-out pass takes the plain view: deterministic, and the plain view of a dataset built
    # without the new options, bit for bit
    net, d, kw = make(**new)
    a = trainer.Trainer(net, d, use_graph=graph, **kw)
    for _ in range(2):
        a.step()
    assert torch.isfinite(_state(a)[0]).all()
    ev = trainer.Evaluator(a.eng.model, d.plain(), 16, _lib.MODE_BF16)
    r1, r2 = ev.run(), ev.run()
    _, d0, _ = make()
    assert not d0.stochastic
    r0 = trainer.Evaluator(a.eng.model, d0.plain(), 16, _lib.MODE_BF16).run()
    for r in (r2, r0):
        assert r["n"] == 74 and r["loss"] == r1["loss"] and r["acc"] == r1["acc"]
        assert torch.equal(r["confusion"], r1["confusion"])
    assert np.isfinite(r1["loss"])
