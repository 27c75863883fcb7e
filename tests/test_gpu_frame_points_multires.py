"""pca_frame_points_multires / dataset.ESC_wave_pc_multires / evalsweep.multires_sweep on the device: every
level of a multi-resolution set is, bit for bit, what pca_frame_points gives for that level alone wherever
the plain launch can express it; offsets and spans it cannot express are the numpy restatement
(tests/multires_ref.py) of what ``meta`` says was drawn; the draws are reproducible and advance per replay
of a captured launch; the Trainer steps and resumes on the dataset."""
import json

import numpy as np
import pytest
import torch

from multires_ref import multires_ref
from oracle import st_oracle as orc
from test_gpu_trainer_eval import _net, _resume_case, _same_bits, _state

pytestmark = pytest.mark.gpu

FS = 44100
TOL = 5e-5          # test_gpu_frame_points.py's bar: the same fp64 arithmetic on both sides


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


def _bits(t):
    return t.contiguous().view(torch.int32)


def _shuffled_with_repeats(n, seed, dev, clamp=True):
    rng = np.random.Generator(np.random.PCG64(seed))
    idx = np.concatenate([rng.permutation(n), rng.integers(0, n, size=max(8, n // 10))])
    if clamp:
        idx = np.concatenate([idx, [-3, n + 5]])                          # clamped to the first / last set
    return torch.from_numpy(idx).to(dev)


def _resident(clips, y, set_off, dev):
    lens = [len(c) for c in clips]
    i64 = lambda a: torch.as_tensor(np.asarray(a, dtype=np.int64)).to(dev)   # noqa: E731
    waves = torch.cat([torch.from_numpy(c).to(dev) for c in clips])
    return dict(waves=waves, woff=i64([0] + list(np.cumsum(lens))), soff=i64(set_off), lab=i64(y),
                max_len=max(lens), min_len=min(lens))


def _spec(n_fft, hop, Nt, n_bins, offset=0, wins=None, time_axis=True):
    """A level as host values (what multires_ref takes): true frame times, ESC_wave_pc's frequency axis."""
    return dict(n_fft=n_fft, hop=hop, Nt=Nt, n_bins=n_bins, offset=offset,
                farr=np.linspace(0, FS / 2, n_bins) / FS,
                tarr=(offset + np.arange(Nt) * hop) / FS if time_axis else None,
                win_lengths=[n_fft] if wins is None else list(wins))


def _dev_level(spec, dev):
    import pca_hip
    f32 = lambda a: torch.as_tensor(np.asarray(a, dtype=np.float64)).float().to(dev)   # noqa: E731
    return pca_hip.FrameLevel(spec["n_fft"], spec["hop"], spec["n_bins"], spec["Nt"], f32(spec["farr"]),
                              None if spec["tarr"] is None else f32(spec["tarr"]),
                              torch.tensor(spec["win_lengths"], dtype=torch.int32, device=dev), spec["offset"])


def _multires(res, idx, levels, span, **kw):
    import pca_hip
    return pca_hip.frame_points_multires(res["waves"], res["woff"], res["soff"], idx, levels, span,
                                         max_len=res["max_len"], min_len=res["min_len"],
                                         clip_labels=res["lab"], **kw)


def _plain(res, idx, lv, **kw):
    """pca_hip.frame_points of one level alone, on the same resident tensors and set offsets."""
    import pca_hip
    return pca_hip.frame_points(res["waves"], res["woff"], res["soff"], idx, lv.n_fft, lv.hop, lv.n_bins,
                                lv.farr, lv.tarr, lv.Nt, max_len=res["max_len"], min_len=res["min_len"],
                                clip_labels=res["lab"], win_lengths=lv.win_lengths, **kw)


# ---- 1. one level is the plain launch ---------------------------------------------------------------------
@pytest.mark.parametrize("n_fft,Nt,n_bins,time_axis", [(64, 1, 33, False), (256, 4, 128, True),
                                                       (1024, 2, 512, True)],
                         ids=["64-2d-nyquist", "256-Nt4", "1024-Nt2"])
def test_one_level_is_the_plain_launch(n_fft, Nt, n_bins, time_axis, corpus, dev):
    import dataset
    clips, y = corpus
    hop = n_fft // 2
    res = _resident(clips, y, dataset.wave_set_offsets([len(c) for c in clips], hop, Nt), dev)
    lv = _dev_level(_spec(n_fft, hop, Nt, n_bins, wins=(n_fft, n_fft * 3 // 4), time_axis=time_axis), dev)
    idx = _shuffled_with_repeats(int(res["soff"][-1]), 1, dev)
    aug = dict(jitter=37, gain_db=6.0, norm_mode=1, seed=11, draw=5, want_meta=True)
    pts, lab, meta = _multires(res, idx, [lv], Nt * hop, **aug)
    want, want_lab, want_meta = _plain(res, idx, lv, **aug)
    assert pts.shape == want.shape == (idx.numel(), Nt * n_bins, 3 if time_axis else 2)
    assert torch.equal(_bits(pts), _bits(want)) and torch.equal(lab, want_lab)
    assert meta.shape == (idx.numel(), 8) and torch.equal(meta[:, :4], want_meta)
    m = meta.cpu().numpy()
    assert len(set(m[:, 4].tolist())) > 20 and set(m[:, 5].tolist()) == {0, 1} and not m[:, 6:].any()
    assert np.abs(m[:, 4]).max() <= 37
    assert set(m[:, 2].tolist()) == {n_fft, n_fft * 3 // 4} and len(set(m[:, 3].tolist())) > 32


# ---- 2. every level of a mixed set is the plain launch's rows ---------------------------------------------
MIXED = [(256, 128, 2, 128, (256, 200)), (64, 32, 8, 32, (64, 48)), (128, 64, 4, 65, (128, 96))]


@pytest.mark.parametrize("norm_mode", [0, 1], ids=["norm-n_fft", "norm-win"])
def test_every_level_of_a_mixed_set_is_the_plain_launch(norm_mode, corpus, dev):
    import dataset
    clips, y = corpus
    span = 256
    res = _resident(clips, y, dataset.wave_span_offsets([len(c) for c in clips], span), dev)
    levels = [_dev_level(_spec(n, h, t, f, wins=w), dev) for n, h, t, f, w in MIXED]
    assert all(lv.Nt * lv.hop == span for lv in levels)                   # the same centres in both launches
    assert [lv.n_fft for lv in levels] != sorted((lv.n_fft for lv in levels), reverse=True)
    idx = _shuffled_with_repeats(int(res["soff"][-1]), 2, dev)
    aug = dict(jitter=300, gain_db=6.0, norm_mode=norm_mode, seed=7, draw=3)
    pts, lab, meta = _multires(res, idx, levels, span, want_meta=True, **aug)
    N = sum(lv.Nt * lv.n_bins for lv in levels)
    assert pts.shape == (idx.numel(), N, 3) and N == 256 + 256 + 260
    p = 0
    for r, lv in enumerate(levels):
        want, want_lab, want_meta = _plain(res, idx, lv, want_meta=True, **aug)
        n = lv.Nt * lv.n_bins
        assert torch.equal(_bits(pts[:, p:p + n]), _bits(want)), f"level {r}"
        assert torch.equal(lab, want_lab)
        assert torch.equal(meta[:, 0], want_meta[:, 0]) and torch.equal(meta[:, 3], want_meta[:, 3])
        if r == 0:
            assert torch.equal(meta[:, :4], want_meta)
        p += n
    m = meta.cpu().numpy()
    assert set(m[:, 5].tolist()) == {0, 1} and m[:, 4].min() < -200 and m[:, 4].max() > 200


# ---- 3. offsets and spans the plain launch cannot express -------------------------------------------------
def _gain(meta_row):
    return np.array([meta_row[3]], dtype=np.int32).view(np.float32)[0]


def _against_ref(clips, set_off, idx, pts, meta, specs, span, norm_mode, jitter):
    """Every slot rebuilt from what ``meta`` reports; (max |delta| of the values, the clamps seen)."""
    worst, low, high = 0.0, 0, 0
    total = set_off[-1]
    for b, i in enumerate(idx):
        i = min(max(int(i), 0), total - 1)
        c, centre0, win0, _, delta, wi = (int(v) for v in meta[b][:6])
        assert set_off[c] <= i < set_off[c + 1] and -jitter <= delta <= jitter
        s, L = i - set_off[c], len(clips[c])
        first = s * span + delta
        assert centre0 == min(max(first + specs[0]["offset"], 0), L)
        assert win0 == specs[0]["win_lengths"][wi]
        want = multires_ref(clips[c], s, delta, _gain(meta[b]), wi, specs, span, norm_mode)
        assert want.shape == pts[b].shape
        assert np.array_equal(pts[b][:, :-1], want[:, :-1]), b            # coordinates: exactly
        worst = max(worst, float(np.abs(pts[b][:, -1] - want[:, -1]).max()))
        ends = [first + sp["offset"] + j * sp["hop"] for sp in specs for j in range(sp["Nt"])]
        low += min(ends) < 0
        high += max(ends) > L
    return worst, low, high


def test_offsets_and_spans_against_numpy(corpus, dev):
    import dataset
    clips, y = corpus
    span, jitter = 200, 500
    set_off = dataset.wave_span_offsets([len(c) for c in clips], span)
    assert set_off[1] == 11                                               # the 0.05 s clip: 2205 samples
    res = _resident(clips, y, set_off, dev)
    specs = [_spec(256, 128, 1, 128, wins=(256, 200)), _spec(64, 32, 5, 32, offset=-64, wins=(64, 48))]
    levels = [_dev_level(sp, dev) for sp in specs]
    rng = np.random.Generator(np.random.PCG64(5))
    idx = np.concatenate([np.tile(np.arange(11), 12), set_off[:-1], np.asarray(set_off[1:]) - 1,
                          rng.integers(0, set_off[-1], size=50)])
    pts, lab, meta = _multires(res, torch.from_numpy(idx).to(dev), levels, span, jitter=jitter, gain_db=6.0,
                               seed=13, draw=2, want_meta=True)
    pts, lab, meta = pts.cpu().numpy(), lab.cpu().numpy(), meta.cpu().numpy()
    assert pts.shape == (idx.size, 128 + 160, 3) and np.isfinite(pts).all()
    assert np.array_equal(lab, y[meta[:, 0]])
    # the coordinate columns are the axes, bit for bit
    f32 = lambda a: np.asarray(a, dtype=np.float64).astype(np.float32)    # noqa: E731
    fcol = np.concatenate([np.tile(f32(sp["farr"]), sp["Nt"]) for sp in specs])
    tcol = np.concatenate([np.repeat(f32(sp["tarr"]), sp["n_bins"]) for sp in specs])
    assert np.array_equal(pts[:, :, 0], np.broadcast_to(fcol, pts.shape[:2]))
    assert np.array_equal(pts[:, :, 1], np.broadcast_to(tcol, pts.shape[:2]))
    worst, low, high = _against_ref(clips, set_off, idx, pts, meta, specs, span, 0, jitter)
    print(f"frame_points_multires vs numpy: max |delta| {worst:.3e} over {idx.size} slots, "
          f"{low} clamped at a clip's start, {high} at its end")
    assert low > 0 and high > 0
    assert worst <= TOL


# ---- 4. the LDS opt-in ------------------------------------------------------------------------------------
def test_n_fft_4096_next_to_n_fft_64(corpus, dev):
    """96 KiB of dynamic LDS for the large level; the small level's workgroups reserve as much."""
    import dataset
    clips, y = corpus
    clips, y = clips[4:], y[4:]                                           # the 0.5 s clip
    span = 2048
    set_off = dataset.wave_span_offsets([len(clips[0])], span)
    assert set_off == [0, 10]
    res = _resident(clips, y, set_off, dev)
    specs = [_spec(4096, 2048, 1, 2048), _spec(64, 32, 4, 32, offset=-64)]
    levels = [_dev_level(sp, dev) for sp in specs]
    idx = torch.tensor([3, 9], device=dev)
    pts, lab, meta = _multires(res, idx, levels, span, gain_db=3.0, seed=2, draw=1, want_meta=True)
    want, want_lab = _plain(res, idx, levels[0], gain_db=3.0, seed=2, draw=1)
    assert pts.shape == (2, 2048 + 128, 3)
    assert torch.equal(_bits(pts[:, :2048]), _bits(want)) and torch.equal(lab, want_lab)
    worst, _, _ = _against_ref(clips, set_off, idx.cpu().numpy(), pts.cpu().numpy(), meta.cpu().numpy(),
                               specs, span, 0, 0)
    print(f"n_fft 4096 + 64: max |delta| {worst:.3e}")
    assert worst <= TOL


# ---- 5. the draws -----------------------------------------------------------------------------------------
def test_draws_reproduce_and_advance_per_replay(corpus, dev):
    import dataset
    clips, y = corpus
    span = 256
    res = _resident(clips, y, dataset.wave_span_offsets([len(c) for c in clips], span), dev)
    levels = [_dev_level(_spec(n, h, t, f, wins=w), dev) for n, h, t, f, w in MIXED[:2]]
    idx = _shuffled_with_repeats(int(res["soff"][-1]), 3, dev, clamp=False)[:64].contiguous()
    aug = dict(jitter=100, gain_db=6.0, seed=5)
    a, _, ma = _multires(res, idx, levels, span, draw=4, want_meta=True, **aug)
    b, _, mb = _multires(res, idx, levels, span, draw=4, want_meta=True, **aug)
    assert torch.equal(_bits(a), _bits(b)) and torch.equal(ma, mb)
    c, _, mc = _multires(res, idx, levels, span, draw=5, want_meta=True, **aug)
    assert not torch.equal(_bits(a), _bits(c))
    for col in (3, 4, 5):                                                 # g, delta, wi
        assert not torch.equal(ma[:, col], mc[:, col]), col
    assert torch.equal(ma[:, 0], mc[:, 0])                                # the same clips
    # the device half of the draw number, captured
    out = torch.zeros_like(a)
    lab = torch.zeros(idx.numel(), dtype=torch.int64, device=dev)
    cnt = torch.zeros(2, dtype=torch.int32, device=dev)
    side = torch.cuda.Stream(dev)
    side.wait_stream(torch.cuda.current_stream(dev))
    with torch.cuda.stream(side):
        _multires(res, idx, levels, span, draw=4, out=out, labels_out=lab, draw_dev=cnt, **aug)
    torch.cuda.current_stream(dev).wait_stream(side)
    torch.cuda.synchronize()
    assert torch.equal(_bits(out), _bits(a))
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        _multires(res, idx, levels, span, draw=4, out=out, labels_out=lab, draw_dev=cnt, **aug)
    seen = []
    for k in (1, 2):
        cnt[0] = k
        g.replay()
        torch.cuda.synchronize()
        seen.append(out.clone())
        eager, eager_lab = _multires(res, idx, levels, span, draw=4 + k, **aug)
        assert torch.equal(_bits(seen[-1]), _bits(eager)) and torch.equal(lab, eager_lab), k
    assert not torch.equal(_bits(seen[0]), _bits(seen[1]))
    assert torch.equal(_bits(seen[0]), _bits(c))


# ---- 6. the dataset ---------------------------------------------------------------------------------------
DS_LEVELS = [dict(n_fft=256, win_lengths=(256, 200)), dict(n_fft=64, win_lengths=(64, 48), offset=16)]


def test_dataset_batches_views_and_items(corpus, dev):
    import dataset
    import pca_hip
    clips, y = corpus
    ds = dataset.ESC_wave_pc_multires(clips, y, FS, DS_LEVELS, 256, jitter=40, gain_db=6.0, norm="win", seed=4,
                                      device=dev)
    lay = ds.layout
    assert ds.stochastic and ds.num_points == 512 and lay["point_off"] == [0, 256]
    n = len(ds)
    idx = torch.tensor([0, n - 1, 5, 5, 9, 2, n // 2], device=dev)
    ds._draw = 6
    pts, lab, meta = ds.batch(idx, want_meta=True)
    assert ds._draw == 7 and tuple(pts.shape) == (7, 512, 3) and tuple(meta.shape) == (7, 8)
    # the binding with the same arguments
    res = _resident(clips, y, ds.set_off, dev)
    specs = [_spec(256, 128, 2, 128, wins=(256, 200)), _spec(64, 32, 8, 32, offset=16, wins=(64, 48))]
    levels = [_dev_level(sp, dev) for sp in specs]
    aug = dict(jitter=40, gain_db=6.0, norm_mode=pca_hip.NORM_WIN, seed=4)
    want = _multires(res, idx, levels, 256, draw=7, want_meta=True, **aug)
    assert torch.equal(_bits(pts), _bits(want[0])) and torch.equal(lab, want[1]) and torch.equal(meta, want[2])
    assert torch.equal(lab.cpu(), torch.from_numpy(ds.labels)[idx.cpu()])
    # buffers passed in, as the Trainer passes them
    o2, l2 = torch.full_like(pts, 3.0), torch.zeros(7, dtype=torch.int64, device=dev)
    ds._draw = 6
    ds.batch(idx, out=o2, labels_out=l2)
    assert torch.equal(_bits(o2), _bits(pts)) and torch.equal(l2, lab)
    # plain(): deterministic, window index 0, one resident store
    p = ds.plain()
    assert not p.stochastic and p._resident()[0].data_ptr() == ds._resident()[0].data_ptr()
    q1, q2 = p.batch(idx, want_meta=True), p.batch(idx, want_meta=True)
    assert torch.equal(_bits(q1[0]), _bits(q2[0])) and torch.equal(q1[2], q2[2])
    m = q1[2].cpu().numpy()
    assert (m[:, 2] == 256).all() and not m[:, 4:].any()
    assert (m[:, 3] == np.array([1.0], dtype=np.float32).view(np.int32)[0]).all()
    off = [dict(sp, win_lengths=sp["win_lengths"][:1]) for sp in specs]
    want = _multires(res, idx, [_dev_level(sp, dev) for sp in off], 256, norm_mode=pca_hip.NORM_WIN)
    assert torch.equal(_bits(q1[0]), _bits(want[0]))
    assert (ds.plain(1).batch(idx, want_meta=True)[2][:, 2] == 200).all()
    # with_levels: a level's rows in the view are its rows in the full set
    v = ds.with_levels([1])
    assert v.num_points == 256 and v._resident()[0].data_ptr() == ds._resident()[0].data_ptr()
    v._draw = 6
    rows, vlab = v.batch(idx)
    assert tuple(rows.shape) == (7, 256, 3)
    assert torch.equal(_bits(rows), _bits(pts[:, 256:])) and torch.equal(vlab, lab)
    sw = ds.with_levels([1, 0])
    sw._draw = 6
    rows = sw.batch(idx)[0]
    assert torch.equal(_bits(rows[:, :256]), _bits(pts[:, 256:]))
    assert torch.equal(_bits(rows[:, 256:]), _bits(pts[:, :256]))
    # one item goes through batch, to the host
    item, lbl = p[5]
    assert item.device.type == "cpu" and tuple(item.shape) == (512, 3)
    assert torch.equal(item, q1[0][2].cpu()) and int(lbl) == int(q1[1][2])
    # 2-D rows
    flat = dataset.ESC_wave_pc_multires(clips, y, FS, [dict(n_fft=256, Ntemp=1), dict(n_fft=64, Ntemp=1)], 256,
                                        device=dev, time_axis=False)
    fp, _ = flat.batch(idx)
    assert tuple(fp.shape) == (7, 160, 2)
    three = dataset.ESC_wave_pc_multires(clips, y, FS, [dict(n_fft=256, Ntemp=1), dict(n_fft=64, Ntemp=1)], 256,
                                         device=dev)
    tp, _ = three.batch(idx)
    assert torch.equal(_bits(fp), _bits(tp[:, :, [0, 2]]))
    with pytest.raises(ValueError):
        dataset.PeakPoints(ds, 16)


# ---- 7. through the Trainer -------------------------------------------------------------------------------
TRAIN_LEVELS = [dict(n_fft=256, hop=128, Ntemp=2, win_lengths=(256, 200)),
                dict(n_fft=64, hop=32, Ntemp=8, win_lengths=(64, 48))]


@pytest.mark.parametrize("graph", [True, False], ids=["hipgraph", "eager"])
def test_trainer_steps_are_the_steps_issued_by_hand_and_resume(dev, tmp_path, graph):
    import dataset
    from pca_hip import _lib, trainer
    B, N = 8, 512
    lengths, y = [1500, 2600, 2100, 3000], [1, 8, 3, 6]                    # 5 + 10 + 8 + 11 = 34 sets
    clips = [orc.synth_clip(90 + i, 2 * i, seconds=n / FS)[:n] for i, n in enumerate(lengths)]

    def make():
        d = dataset.ESC_wave_pc_multires(clips, y, FS, TRAIN_LEVELS, 256, jitter=64, gain_db=6.0, seed=9,
                                         device=dev)
        assert len(d) == 34 and d.num_points == N and d.stochastic        # 4 steps per epoch
        return _net(dev, 3, seed=4), d, dict(seed=5, batch_size=B, mode=_lib.MODE_BF16)

    net, ds, kw = make()
    tr = trainer.Trainer(net, ds, use_graph=graph, **kw)
    assert tr.lengths is None and tr.N == N and not tr._cursor_mode
    losses, batches = [], []
    for _ in range(3):
        tr.step()
        torch.cuda.synchronize()
        losses.append(float(tr.eng.loss))
        batches.append(tr.X.clone())
    want = _state(tr)
    assert torch.isfinite(want[0]).all() and all(np.isfinite(losses)) and len(set(losses)) == 3, losses
    assert not torch.equal(batches[0], batches[1])

    # by hand: ds.batch -> STEngine.fwd_bwd -> Adam
    net, ds, _ = make()
    eng = trainer.STEngine(net, B, N, _lib.MODE_BF16, training=True)
    n = eng.flat.numel()
    m, v = torch.zeros(n, device=dev), torch.zeros(n, device=dev)
    step_count = torch.zeros(2, dtype=torch.int32, device=dev)
    X = torch.empty((B, N, 3), device=dev)
    lab = torch.zeros(B, dtype=torch.int64, device=dev)
    stream = trainer.ShardedIndexStream(len(ds), B, 0, 1, 5, True, dev)
    for s in range(3):
        if graph:                  # a captured step froze the host draw number of its recorded call, the 2nd
            ds._draw = 1
        ds.batch(stream.next().clone(), out=X, labels_out=lab, draw_dev=step_count)
        eng.fwd_bwd(X, lab)
        _lib.check(_lib.lib().pca_adam_step(eng.flat.data_ptr(), eng.grads.data_ptr(), m.data_ptr(),
                                            v.data_ptr(), n, 1e-3, 0.9, 0.999, 1e-8, 1e-3, 1.0,
                                            step_count.data_ptr(), 1, eng._stream()), "pca_adam_step")
        torch.cuda.synchronize()
        assert torch.equal(_bits(X), _bits(batches[s])), s
        assert float(eng.loss) == losses[s], (s, float(eng.loss), losses[s])
    _same_bits((eng.flat, m, v, step_count), want)

    # 6 steps straight = 3 steps + checkpoint + a fresh Trainer + 3 steps, bitwise
    _resume_case(make, 3, tmp_path, graph=graph)
    r = trainer.Evaluator(net, ds.plain(), 16, _lib.MODE_BF16).run()
    assert r["n"] == 34 and np.isfinite(r["loss"])


# ---- 8. the sweep -----------------------------------------------------------------------------------------
def test_multires_sweep(corpus, dev, tmp_path):
    import dataset
    import evalsweep
    import models
    clips, y = corpus
    clips = [torch.from_numpy(c).to(dev) for c in clips[:3]]
    y = y[:3]
    torch.manual_seed(11)
    net = models.ST(dim_input=3, num_outputs=1, dim_output=10, num_inds=4, dim_hidden=16,
                    num_heads=4).to(dev).eval()
    path = str(tmp_path / "multires.json")
    levels = [dict(n_fft=256), dict(n_fft=64, offset=16)]
    out = evalsweep.multires_sweep(net, clips, y, FS, levels, 256, batch_size=8, json_file=path,
                                   sets_per_call=6)
    assert list(out["data"]) == ["0+1", "0", "1"] and out["list_subsets"] == [[0, 1], [0], [1]]
    assert out["span"] == 256 and [lv["n_fft"] for lv in out["levels"]] == [256, 64]
    assert out["levels"][1] == dict(n_fft=64, hop=32, Ntemp=8, F=32, offset=16, win_lengths=[64])
    back = json.load(open(path))
    assert back == json.loads(json.dumps(out)) and back["data"] == {k: list(v) for k, v in out["data"].items()}
    ds = dataset.ESC_wave_pc_multires(clips, y, FS, levels, 256, device=dev)
    assert len(ds) >= 16
    acc = lambda d: evalsweep._dataset_accuracy(net, d, None, 3, 8, evalsweep._lib.MODE_F32, 6)  # noqa: E731
    assert out["data"]["0+1"] == [acc(ds), 0]
    for k in (0, 1):
        assert out["data"][str(k)] == [acc(ds.with_levels([k])), 0]
    assert all(0.0 <= v[0] <= 1.0 for v in out["data"].values())
    # subsets of the caller's choice; three levels' defaults
    out = evalsweep.multires_sweep(net, clips, y, FS, levels, 256, subsets=[(1,), (1, 0)], sets_per_call=6)
    assert list(out["data"]) == ["0+1", "1", "1+0"]
    assert evalsweep.default_level_subsets(3) == [(0,), (1,), (2,), (1, 2), (0, 2), (0, 1)]
