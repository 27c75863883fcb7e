"""pca_frame_points_masked and the mask options of dataset.ESC_wave_pc[_temp] on the device: the masked
batch is the dense batch of the same draw with the bands and stripes the mask meta reports removed
(tests/mask_ref.py), bit for bit, in drop and in floor mode; the mask draws are uniform, reproducible,
independent of the other augmentations' draws and advance per replay of a captured training step."""
import numpy as np
import pytest
import torch

from mask_ref import DROP, FLOOR, mask_rows, masked_axes
from oracle import st_oracle as orc
from test_gpu_trainer_eval import _net, _resume_case, _state

pytestmark = pytest.mark.gpu

FS = 44100
ZERO_CLIP = 5


@pytest.fixture(scope="module")
def dev():
    return torch.device("cuda", 0)


@pytest.fixture(scope="module")
def corpus():
    """Five clips of 0.05 .. 0.5 s and an all-zero one (what a silent bin's value is read from)."""
    secs = (0.05, 0.11, 0.2, 0.3667, 0.5)
    clips = [orc.synth_clip(40 + i, 3 * i + 1, seconds=s) for i, s in enumerate(secs)]
    clips.append(np.zeros(6000, dtype=np.float32))
    return clips, np.array([4, 9, 2, 7, 5, 1])


@pytest.fixture(scope="module")
def backgrounds():
    rng = np.random.Generator(np.random.PCG64(8))
    return [orc.synth_clip(60, 2, seconds=0.03), (0.3 * rng.standard_normal(100)).astype(np.float32),
            orc.synth_clip(61, 8, seconds=0.08)]


def _dataset(clips, y, dev, ntemp, n_fft, **kw):
    import dataset
    if ntemp == 1:
        return dataset.ESC_wave_pc(clips, y, FS, n_fft, device=dev, **kw)
    return dataset.ESC_wave_pc_temp(clips, y, FS, n_fft, ntemp, device=dev, **kw)


def _ends_and_random(ds, seed, n=64):
    """First and last set of every clip, then random ones."""
    rng = np.random.Generator(np.random.PCG64(seed))
    ends = np.concatenate([ds.set_off[:-1], np.asarray(ds.set_off[1:]) - 1])
    return np.concatenate([ends, rng.integers(0, len(ds), size=n - ends.size)])


def _batch_at(ds, idx, draw, **kw):
    ds._draw = draw - 1                                                   # batch() advances it first
    return ds.batch(idx, want_meta=True, **kw)


def _bits(a):
    return np.ascontiguousarray(a).view(np.int32)


def _same_ex_meta(meta, dense_meta):
    """Columns 0 - 7 of the masked launch's meta against the dense launch's: 8 columns from the ex launch,
    4 from pca_frame_points, whose other four are what the ex launch reports with speed and mix off."""
    if dense_meta.shape[1] == 8:
        assert np.array_equal(meta[:, :8], dense_meta)
    else:
        assert dense_meta.shape[1] == 4 and np.array_equal(meta[:, :4], dense_meta)
        assert (meta[:, 4] == 0).all() and (meta[:, 5] == -1).all() and (meta[:, 6:8] == 0).all()


SHAPES = {
    # (n_fft, Ntemp): n_bins, mask options, speeds (None: the dense batch is one pca_frame_points launch)
    (64, 1): (33, dict(freq_masks=3, freq_mask_width=10), None),
    (64, 4): (32, dict(freq_masks=2, freq_mask_width=8, time_masks=1, time_mask_width=2), (1.0, 0.9)),
    (256, 3): (128, dict(freq_masks=4, freq_mask_width=31, time_masks=2, time_mask_width=1), (1.0, 1.1)),
    (1024, 1): (513, dict(freq_masks=4, freq_mask_width=120), None),     # bins past one 256-thread pass
    (4096, 1): (2049, dict(freq_masks=4, freq_mask_width=500), None),    # 96 KiB of LDS
}


def _pair(shape, corpus, dev, mode):
    """(masked dataset, the same dataset with the masks off, indices)."""
    n_fft, ntemp = shape
    n_bins, mask, speeds = SHAPES[shape]
    clips, y = corpus
    if n_fft == 4096:
        clips, y = clips[4:], y[4:]                                       # the 0.5 s clip and the silent one
    aug = dict(jitter=37, gain_db=6.0, win_lengths=(n_fft // 2, 200 * n_fft // 256, n_fft), seed=11,
               speeds=speeds)
    on = _dataset(clips, y, dev, ntemp, n_fft, mask_mode=mode, **mask, **aug)
    off = _dataset(clips, y, dev, ntemp, n_fft, **aug)
    assert on.F == off.F == n_bins and on.stochastic and off.stochastic
    assert on.variable_length == (mode == "drop") and not off.variable_length
    idx = np.array([3, 10]) if n_fft == 4096 else _ends_and_random(on, 1)
    return on, off, idx


# ---- 1. drop against the dense launch, bit for bit ---------------------------------------------------------
@pytest.mark.parametrize("shape", list(SHAPES), ids=lambda s: f"{s[0]}x{s[1]}")
def test_drop_is_the_dense_batch_compacted(shape, corpus, dev):
    on, off, idx = _pair(shape, corpus, dev, "drop")
    n_bins, Nt = on.F, on._ntemp
    N, din, B = n_bins * Nt, 2 if Nt == 1 else 3, idx.size
    idx_t = torch.from_numpy(idx).to(dev)
    out = torch.full((B, N, din), float("nan"), device=dev)
    lengths_out = torch.full((B,), -7, dtype=torch.int32, device=dev)
    pts, lab, meta, lengths = _batch_at(on, idx_t, 4, out=out, lengths_out=lengths_out)
    assert pts.data_ptr() == out.data_ptr() and lengths.data_ptr() == lengths_out.data_ptr()
    assert meta.shape == (B, 24) and meta.dtype == torch.int32
    dense, dense_lab, dense_meta = _batch_at(off, idx_t, 4)
    assert dense.shape == (B, N, din) and torch.equal(lab, dense_lab)
    pts, meta, lengths = pts.cpu().numpy(), meta.cpu().numpy(), lengths.cpu().numpy()
    dense, dense_meta = dense.cpu().numpy(), dense_meta.cpu().numpy()
    assert not np.isnan(pts).any()                                        # every row was written
    _same_ex_meta(meta, dense_meta)                                       # the masks moved no earlier draw
    assert len(set(dense_meta[:, 2].tolist())) == 3 or B == 2             # ... which were on
    frames_gone = 0
    for b in range(B):
        want, n = mask_rows(dense[b], meta[b, 8:], n_bins, Nt, DROP)
        assert lengths[b] == n and 1 <= n <= N, (b, lengths[b], n)
        assert np.array_equal(_bits(pts[b]), _bits(want)), b
        assert (_bits(pts[b, n:]) == 0).all(), b                          # the tail: +0.0 in every column
        frames_gone += int(masked_axes(meta[b, 8:], n_bins, Nt)[1].sum())
    assert (lengths < N).sum() >= B // 2 and len(set(lengths.tolist())) >= min(B, 8) // 2
    assert Nt == 1 or frames_gone > 0
    # the same arguments, the same bits
    again = _batch_at(on, idx_t, 4)
    assert np.array_equal(_bits(again[0].cpu().numpy()), _bits(pts))
    assert np.array_equal(again[3].cpu().numpy(), lengths)


def test_masks_off_is_the_ex_launch_and_lengths_are_n(corpus, dev):
    """pca_frame_points_masked with both kinds off: pca_frame_points_ex's bits, lengths_out = N."""
    import pca_hip
    clips, y = corpus
    ds = _dataset(clips, y, dev, 3, 256, jitter=37, gain_db=6.0, seed=11)
    waves, woff, soff, f32, t32, lab = ds._resident()
    idx = torch.from_numpy(_ends_and_random(ds, 2)).to(dev)
    args = (waves, woff, soff, idx, 256, ds.hop, ds.F, f32, t32, 3)
    kw = dict(max_len=ds._max_len, min_len=ds._min_len, clip_labels=lab, jitter=37, gain_db=6.0, seed=11,
              draw=4, ratios=(1.0, 0.9), want_meta=True)
    want, want_lab, want_meta = pca_hip.frame_points_ex(*args, **kw)
    for mask in (dict(), dict(freq_masks=3), dict(time_mask_width=2)):
        got, got_lab, meta, lengths = pca_hip.frame_points_masked(*args, **mask, **kw)
        assert torch.equal(got.view(torch.int32), want.view(torch.int32)) and torch.equal(got_lab, want_lab)
        assert torch.equal(meta[:, :8], want_meta) and (meta[:, 8:] == 0).all()
        assert (lengths == 3 * ds.F).all() and lengths.dtype == torch.int32
    res = pca_hip.frame_points_masked(*args, mask_mode="floor", **kw)
    assert len(res) == 3 and torch.equal(res[0].view(torch.int32), want.view(torch.int32))


# ---- 2. floor -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", [(64, 4), (1024, 1)], ids=lambda s: f"{s[0]}x{s[1]}")
def test_floor_keeps_the_rows_and_silences_the_masked_points(shape, corpus, dev):
    on, off, idx = _pair(shape, corpus, dev, "floor")
    n_bins, Nt = on.F, on._ntemp
    idx_t = torch.from_numpy(idx).to(dev)
    out = torch.full((idx.size, n_bins * Nt, 2 if Nt == 1 else 3), float("nan"), device=dev)
    res = _batch_at(on, idx_t, 4, out=out)
    assert len(res) == 3                                                  # no lengths in this mode
    pts, meta = res[0].cpu().numpy(), res[2].cpu().numpy()
    dense, _, dense_meta = _batch_at(off, idx_t, 4)
    dense, dense_meta = dense.cpu().numpy(), dense_meta.cpu().numpy()
    _same_ex_meta(meta, dense_meta)
    # a silent bin's value, as the device computes it: the dense rows of the all-zero clip
    silent = np.nonzero(dense_meta[:, 0] == ZERO_CLIP)[0]
    assert silent.size >= 2
    quiet = dense[silent[0], 0, -1]
    assert (_bits(dense[silent][:, :, -1]) == _bits(quiet)).all() and abs(quiet - np.log(1e-8)) < 1e-5
    assert not np.isnan(pts).any()
    masked = 0
    for b in range(idx.size):
        want, n = mask_rows(dense[b], meta[b, 8:], n_bins, Nt, FLOOR, floor_value=quiet)
        assert n == n_bins * Nt
        assert np.array_equal(_bits(pts[b]), _bits(want)), b              # off the mask: the dense bits
        masked += int((_bits(want) != _bits(dense[b])).any())
    assert masked >= idx.size // 2
    with pytest.raises(ValueError):
        on.batch(idx_t, lengths_out=torch.zeros(idx.size, dtype=torch.int32, device=dev))


# ---- 3. the draws -------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def long_clip():
    return [orc.synth_clip(77, 6, seconds=0.5)], np.array([6])


MASK3 = dict(freq_masks=2, freq_mask_width=8, time_masks=1, time_mask_width=2)


def _draw_ds(long_clip, dev, **kw):
    clips, y = long_clip
    args = dict(jitter=8, gain_db=6.0, win_lengths=(32, 48, 64), seed=21, **MASK3)
    args.update(kw)
    return _dataset(clips, y, dev, 4, 64, **args)


def _within_5_sigma(count, n, p, what):
    bound = 5.0 * np.sqrt(n * p * (1.0 - p))
    print(f"{what}: {count} of {n}, expected {n * p:.1f} +- {bound:.1f}")
    assert abs(count - n * p) <= bound, what


def _uniform_starts(start, extent, what):
    """``start`` uniform over 0 .. extent - 1: four buckets (or every value of a short range)."""
    n = start.size
    assert start.min() >= 0 and start.max() < extent, what
    if extent <= 5:
        for v in range(extent):
            _within_5_sigma(int((start == v).sum()), n, 1.0 / extent, f"{what} = {v}")
        return
    bucket = (start.astype(np.int64) * 4) // extent
    for q in range(4):
        lo, hi = -(-q * extent // 4), -(-(q + 1) * extent // 4)
        _within_5_sigma(int((bucket == q).sum()), n, (hi - lo) / extent, f"{what}, bucket {q}")


def test_mask_draws_are_uniform_independent_and_reproducible(long_clip, backgrounds, dev):
    ds = _draw_ds(long_clip, dev)
    n_bins, Nt, slots = 32, 4, 4096
    n = len(ds)
    assert n == 172 and ds.F == n_bins
    idx = torch.arange(slots, device=dev) % n
    pts, _, meta, lengths = _batch_at(ds, idx, 3)
    m = meta.cpu().numpy().astype(np.int64)
    bands, stripes = m[:, 8:16].reshape(slots, 4, 2), m[:, 16:24].reshape(slots, 4, 2)
    assert (bands[:, 2:] == 0).all() and (stripes[:, 1:] == 0).all()      # unused entries
    # every draw inside its range, widths and starts uniform
    for k in range(2):
        f0, w = bands[:, k, 0], bands[:, k, 1]
        assert w.min() >= 0 and w.max() <= 8 and f0.min() >= 0 and (f0 + w <= n_bins).all()
        for v in range(9):
            _within_5_sigma(int((w == v).sum()), slots, 1.0 / 9.0, f"band {k} width {v}")
            _uniform_starts(f0[w == v], n_bins - v + 1, f"band {k} start at width {v}")
    t0, tw = stripes[:, 0, 0], stripes[:, 0, 1]
    assert tw.min() >= 0 and tw.max() <= 2 and t0.min() >= 0 and (t0 + tw <= Nt).all()
    for v in range(3):
        _within_5_sigma(int((tw == v).sum()), slots, 1.0 / 3.0, f"stripe width {v}")
        _uniform_starts(t0[tw == v], Nt - v + 1, f"stripe start at width {v}")
    # the two bands of a slot are drawn independently of each other
    _within_5_sigma(int((bands[:, 0, 1] == bands[:, 1, 1]).sum()), slots, 1.0 / 9.0, "equal band widths")
    # every kind of slot the compaction has to get right is in the batch
    w0, w1, a0, a1 = bands[:, 0, 1], bands[:, 1, 1], bands[:, 0, 0], bands[:, 1, 0]
    kinds = {
        "a width-0 band": (w0 == 0) | (w1 == 0),
        "a band at bin 0": ((a0 == 0) & (w0 > 0)) | ((a1 == 0) & (w1 > 0)),
        "a band ending at n_bins": ((a0 + w0 == n_bins) & (w0 > 0)) | ((a1 + w1 == n_bins) & (w1 > 0)),
        "two overlapping bands": (w0 > 0) & (w1 > 0) & (a0 < a1 + w1) & (a1 < a0 + w0),
        "a stripe at frame 0": (t0 == 0) & (tw > 0),
        "a stripe ending at Nt": (t0 + tw == Nt) & (tw > 0),
        "nothing masked": (w0 == 0) & (w1 == 0) & (tw == 0),
    }
    for what, sel in kinds.items():
        print(f"{what}: {int(sel.sum())} slots")
        assert sel.any(), what
    # ... and each of them is the dense batch compacted (the dense batch: the same draw with the masks off)
    dense = _batch_at(_draw_ds(long_clip, dev, freq_masks=0, time_masks=0), idx, 3)[0].cpu().numpy()
    got, ln = pts.cpu().numpy(), lengths.cpu().numpy()
    check = set()
    for sel in kinds.values():
        check.update(np.nonzero(sel)[0][:4].tolist())
    for b in sorted(check):
        want, cnt = mask_rows(dense[b], m[b, 8:], n_bins, Nt, DROP)
        assert ln[b] == cnt and np.array_equal(_bits(got[b]), _bits(want)), b
    axes = [masked_axes(m[b, 8:], n_bins, Nt) for b in range(slots)]
    assert np.array_equal(ln, [(~bins).sum() * (~frames).sum() for bins, frames in axes])
    assert (ln[kinds["nothing masked"]] == n_bins * Nt).all()
    # the same set in two slots of one call: independent draws
    assert not np.array_equal(m[:n, 8:], m[n:2 * n, 8:])

    again = _batch_at(ds, idx, 3)
    assert torch.equal(again[0].view(torch.int32), pts.view(torch.int32)) and torch.equal(again[2], meta)
    assert torch.equal(again[3], lengths)
    other = _batch_at(ds, idx, 4)
    assert not torch.equal(other[2][:, 8:], meta[:, 8:]) and not torch.equal(other[3], lengths)
    seeded = _batch_at(_draw_ds(long_clip, dev, seed=22), idx, 3)
    assert not torch.equal(seeded[2][:, 8:], meta[:, 8:]) and not torch.equal(seeded[3], lengths)
    # the device half of the draw number
    two = torch.tensor([2, 0], dtype=torch.int32, device=dev)
    a = _batch_at(ds, idx, 5, draw_dev=two)
    b = _batch_at(ds, idx, 7)
    assert torch.equal(a[0].view(torch.int32), b[0].view(torch.int32))
    assert torch.equal(a[2], b[2]) and torch.equal(a[3], b[3])

    # speed and mix do not move the mask draws, and the masks do not move theirs
    ex = dict(speeds=(1.0, 0.8, 1.25), mix_clips=backgrounds, mix_prob=0.5)
    both = _batch_at(_draw_ds(long_clip, dev, **ex), idx, 3)
    assert torch.equal(both[2][:, 8:], meta[:, 8:]) and torch.equal(both[3], lengths)
    assert torch.equal(both[2][:, 2:4], meta[:, 2:4])                     # window and gain
    ex_only = _batch_at(_draw_ds(long_clip, dev, freq_masks=0, time_masks=0, **ex), idx, 3)
    assert ex_only[2].shape == (slots, 8) and torch.equal(both[2][:, :8], ex_only[2])
    assert len(set(ex_only[2][:, 4].tolist())) == 3 and (ex_only[2][:, 5] >= 0).any()
    # one kind alone draws what it draws beside the other
    bands_only = _batch_at(_draw_ds(long_clip, dev, time_masks=0), idx, 3)[2]
    stripes_only = _batch_at(_draw_ds(long_clip, dev, freq_masks=0), idx, 3)[2]
    assert torch.equal(bands_only[:, 8:16], meta[:, 8:16]) and (bands_only[:, 16:] == 0).all()
    assert torch.equal(stripes_only[:, 16:], meta[:, 16:]) and (stripes_only[:, 8:16] == 0).all()


# ---- 4. with speed, mix and the soft targets on -------------------------------------------------------------
def test_masks_with_speed_mix_and_soft_targets(corpus, backgrounds, dev):
    clips, y = corpus
    ex = dict(speeds=(1.0, 0.8, 1.25), mix_clips=backgrounds, mix_prob=0.5, mix_snr_db=(-10.0, 20.0),
              mix_targets=True, mix_labels=[3, 0, 8], jitter=37, gain_db=6.0, win_lengths=(128, 200, 256),
              norm="win", seed=13)
    mask = dict(freq_masks=3, freq_mask_width=20, time_masks=1, time_mask_width=2)
    on = _dataset(clips, y, dev, 3, 256, **mask, **ex)
    off = _dataset(clips, y, dev, 3, 256, **ex)
    assert on.soft_targets and on.variable_length and off.soft_targets and not off.variable_length
    n_bins, Nt = on.F, 3
    idx = _ends_and_random(on, 7)
    idx_t = torch.from_numpy(idx).to(dev)
    pts, lab, meta, samples, lab2, wgt, lengths = _batch_at(on, idx_t, 6, want_samples=True)
    dense, dlab, dmeta, dsamples, dlab2, dwgt = _batch_at(off, idx_t, 6, want_samples=True)
    assert torch.equal(meta[:, :8], dmeta) and torch.equal(lab, dlab)
    assert torch.equal(lab2, dlab2) and torch.equal(wgt.view(torch.int32), dwgt.view(torch.int32))
    assert (dmeta[:, 4] != 0).any() and (dmeta[:, 5] >= 0).any() and (wgt != 1).any()
    pts, meta, lengths = pts.cpu().numpy(), meta.cpu().numpy(), lengths.cpu().numpy()
    dense, samples, dsamples = dense.cpu().numpy(), samples.cpu().numpy(), dsamples.cpu().numpy()
    dropped = 0
    for b in range(idx.size):
        want, n = mask_rows(dense[b], meta[b, 8:], n_bins, Nt, DROP)
        assert lengths[b] == n and np.array_equal(_bits(pts[b]), _bits(want)), b
        frames = masked_axes(meta[b, 8:], n_bins, Nt)[1]
        for j in range(Nt):
            if frames[j]:                                                 # not loaded: zeros
                assert (_bits(samples[b, j]) == 0).all(), (b, j)
                dropped += 1
            else:
                assert np.array_equal(_bits(samples[b, j]), _bits(dsamples[b, j])), (b, j)
    assert dropped >= 8


# ---- 5. through the Trainer ---------------------------------------------------------------------------------
def _train_clips(lengths):
    return [orc.synth_clip(90 + i, 2 * i, seconds=n / FS)[:n] for i, n in enumerate(lengths)]


@pytest.mark.parametrize("graph", [True, False], ids=["hipgraph", "eager"])
@pytest.mark.parametrize("mode,targets", [("drop", False), ("drop", True), ("floor", False)],
                         ids=["drop", "drop-mix_targets", "floor"])
def test_trainer_masks_afresh_resumes_and_evaluates(dev, tmp_path, graph, mode, targets):
    import dataset
    from pca_hip import _lib, trainer
    new = dict(freq_masks=2, freq_mask_width=8, time_masks=1, time_mask_width=2, mask_mode=mode)
    if targets:
        new.update(mix_clips="self", mix_prob=0.5, mix_snr_db=(-10.0, 10.0), mix_targets=True)
    kw_tr = dict(batch_size=16, mode=_lib.MODE_BF16)                      # n_fft 128, Ntemp 4: N = 256

    def dataset_of(lengths, y, **opts):
        return dataset.ESC_wave_pc_temp(_train_clips(lengths), y, FS, 128, 4, seed=9, device=dev, **opts)

    # (a) one batch of 16 sets, the same indices every step: the packed batch and the counts still change
    ds = dataset_of([4100], [3], **new)
    assert ds.num_points == 256 and ds.stochastic and ds.variable_length == (mode == "drop")
    assert len(ds) == 16
    tr = trainer.Trainer(_net(dev, 3, seed=4), ds, use_graph=graph, shuffle=False, seed=5, **kw_tr)
    assert (tr.lengths is not None) == (mode == "drop") and (tr.labels2 is not None) == targets
    seen = []
    for _ in range(3):
        tr.step()
        torch.cuda.synchronize()
        seen.append((tr.X.clone(), tr.idx.clone(), None if tr.lengths is None else tr.lengths.clone()))
    for p, q in ((0, 1), (1, 2)):
        assert torch.equal(seen[p][1], seen[q][1]) and not torch.equal(seen[p][0], seen[q][0])
        if mode == "drop":
            assert not torch.equal(seen[p][2], seen[q][2])
    if mode == "drop":
        for X, _, ln in seen:
            assert (ln >= 1).all() and (ln <= 256).all() and (ln < 256).any()
            beyond = torch.arange(256, device=dev)[None, :] >= ln[:, None]
            assert (X[beyond].view(torch.int32) == 0).all()               # rows beyond lengths
            assert (X[~beyond][:, 0] >= 0).all() and torch.isfinite(X).all()
    assert torch.isfinite(tr.eng.flat).all()

    # (b) 6 steps straight = 3 steps + checkpoint + a fresh Trainer + 3 steps, bitwise
    lengths, y = [3000, 5200, 4100, 6000], [1, 8, 3, 6]                   # 11 + 20 + 16 + 23 = 70 sets

    def make(**opts):
        d = dataset_of(lengths, y, **opts)
        assert len(d) == 70                                               # 4 steps per epoch
        return _net(dev, 3, seed=4), d, dict(seed=5, **kw_tr)

    _resume_case(lambda: make(**new), 3, tmp_path, graph=graph)

    # (c) the held-out pass takes the plain view: dense, deterministic, and the plain view of a dataset built
    # without the masks, bit for bit
    net, d, kw = make(**new)
    a = trainer.Trainer(net, d, use_graph=graph, **kw)
    for _ in range(2):
        a.step()
    assert torch.isfinite(_state(a)[0]).all()
    assert not d.plain().variable_length and not d.plain().stochastic
    ev = trainer.Evaluator(a.eng.model, d.plain(), 16, _lib.MODE_BF16)
    assert all(ln is None for _, _, ln in ev.engines)
    r1, r2 = ev.run(), ev.run()
    _, d0, _ = make()
    assert not d0.stochastic
    r0 = trainer.Evaluator(a.eng.model, d0.plain(), 16, _lib.MODE_BF16).run()
    for r in (r2, r0):
        assert r["n"] == 70 and r["loss"] == r1["loss"] and r["acc"] == r1["acc"]
        assert torch.equal(r["confusion"], r1["confusion"])
    assert np.isfinite(r1["loss"])


def test_getitem_returns_the_unpadded_set(corpus, dev):
    clips, y = corpus
    ds = _dataset(clips, y, dev, 4, 64, seed=3, **MASK3)
    sizes = set()
    for i in range(12):
        pts, lbl = ds[i]
        assert pts.ndim == 2 and pts.shape[1] == 3 and 1 <= pts.shape[0] <= 128
        assert (pts[:, 0] > 0).sum() >= pts.shape[0] - 4                # no padding row: farr is 0 at bin 0 only
        assert int(lbl) == ds.labels[i]
        sizes.add(pts.shape[0])
    assert len(sizes) > 3
    assert ds.plain()[0][0].shape == (128, 3)
