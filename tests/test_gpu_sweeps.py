"""Batch-scale sweeps on the device (evalsweep.subsample_sweep / importance_sweep /
reframe_sweep_temporal) and the two entry points they add: pca_eval_tally (device-side correct
counts) and pca_stft_logmag_batch_norm (the re-framing loops' divide-by-N spectrum).

Small seeded corpora; models at the shipped shape (d = 64, 8 heads, 64 inducing points) and at
d = 128.  Max-K / max-heat results are compared exactly with the existing item-level path; the
random selections are re-drawn with the same (seed, draw, slot, set) keys and re-evaluated."""
import json
import math

import numpy as np
import pytest
import torch

from util import T

pytestmark = pytest.mark.gpu

FS = 22050
SHAPES = {"shipped": dict(d=64, h=8, m=64), "d128": dict(d=128, h=4, m=16)}


@pytest.fixture(scope="module")
def dev():
    return torch.device("cuda", 0)


def _net(din, shape, dev, seed=0):
    import models
    torch.manual_seed(seed)
    s = SHAPES[shape]
    return models.ST(dim_input=din, dim_output=10, num_inds=s["m"], dim_hidden=s["d"],
                     num_heads=s["h"]).to(dev)


def _fst_corpus(n=61, F=1025, seed=3):
    rng = np.random.Generator(np.random.PCG64(seed))
    x = rng.normal(-9, 3, size=(F, n)).astype(np.float32)
    y = rng.integers(0, 10, size=n)
    farr = np.linspace(0, 44100 / 2, F) / 44100
    return x, y, farr


def _3st_corpus(n=27, F=512, Nt=10, seed=4):
    rng = np.random.Generator(np.random.PCG64(seed))
    x = rng.normal(-9, 3, size=(F, Nt, n)).astype(np.float32)
    y = rng.integers(0, 10, size=n)
    farr = np.linspace(0, 44100 / 2, F) / 44100
    tarr = np.linspace(0, (512 / 44100) * Nt, Nt)
    return x, y, farr, tarr


# ----------------------------------------------------------------------------------------------- #
# pca_eval_tally                                                                                   #
# ----------------------------------------------------------------------------------------------- #
def _ref_count(logits, labels):
    return int((logits.argmax(1) == labels).sum())          # torch.argmax on the host


def test_eval_tally_matches_argmax(dev):
    import pca_hip
    g = torch.Generator().manual_seed(5)
    cases = []
    for B, C in ((37, 10), (1, 10), (5, 1), (1, 1), (300, 50), (64, 130)):
        lg = torch.randint(-3, 4, (B, C), generator=g).float()     # many ties
        y = torch.randint(0, C, (B,), generator=g)
        cases.append((lg, y))
    lg = torch.randn(40, 10, generator=g)
    lg[3, 7] = float("nan")                                  # NaN is the maximum
    lg[5, :] = float("nan")                                  # first NaN wins
    lg[6, 2] = float("nan")
    lg[6, 8] = float("nan")
    lg[9, :] = float("-inf")
    lg[10, 4] = float("inf")
    lg[11, :] = 2.0                                          # all equal: index 0
    y = torch.randint(0, 10, (40,), generator=g)
    y[3], y[5], y[6], y[9], y[10], y[11] = 7, 0, 2, 0, 4, 0
    cases.append((lg, y))
    for lg, y in cases:
        counts = torch.zeros(3, dtype=torch.int64, device=dev)
        pca_hip.eval_tally(lg.to(dev), y.to(dev), counts, 1)
        ref = _ref_count(lg, y)
        assert counts.tolist() == [0, ref, 0], (tuple(lg.shape), counts.tolist(), ref)
    # the NaN / inf / all-equal rows are all counted as correct above
    assert _ref_count(lg[[3, 5, 6, 9, 10, 11]], y[[3, 5, 6, 9, 10, 11]]) == 6


def test_eval_tally_accumulates_and_replays(dev):
    import pca_hip
    g = torch.Generator().manual_seed(6)
    lg = torch.randint(-2, 3, (97, 10), generator=g).float()
    y = torch.randint(0, 10, (97,), generator=g)
    ref = _ref_count(lg, y)
    lgd, yd = lg.to(dev), y.to(dev)
    counts = torch.zeros(2, dtype=torch.int64, device=dev)
    for _ in range(3):
        pca_hip.eval_tally(lgd, yd, counts, 0)
    pca_hip.eval_tally(lgd[:50], yd[:50], counts, 1)
    pca_hip.eval_tally(lgd[50:], yd[50:], counts, 1)
    assert counts.tolist() == [3 * ref, ref]
    # captured into a graph: every replay adds the same count
    cg = torch.zeros(2, dtype=torch.int64, device=dev)
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        pca_hip.eval_tally(lgd, yd, cg, 0)                  # warm-up outside the capture
    torch.cuda.current_stream().wait_stream(s)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        pca_hip.eval_tally(lgd, yd, cg, 0)
        pca_hip.eval_tally(lgd[10:], yd[10:], cg, 1)
    cg.zero_()
    for _ in range(4):
        graph.replay()
    torch.cuda.synchronize()
    assert cg.tolist() == [4 * ref, 4 * _ref_count(lg[10:], y[10:])]
    with pytest.raises(pca_hip.PcaHipError):
        from pca_hip import _lib
        _lib.check(_lib.lib().pca_eval_tally(lgd.data_ptr(), yd.data_ptr(), 0, 10,
                                             counts.data_ptr(), 0, None), "pca_eval_tally")


# ----------------------------------------------------------------------------------------------- #
# pca_stft_logmag_batch_norm                                                                       #
# ----------------------------------------------------------------------------------------------- #
def _np_stft_logmag_div(wave, n_fft, win_length, hop, norm, drop_nyquist):
    """librosa.stft(x, n_fft, win_length, hop, 'hann', center=True, reflect) / norm, then
    log(1e-8 + |.|) (Code/pc_temp3d_eval.py:75-77), in float64 -> float32."""
    n = np.arange(win_length)
    w = 0.5 - 0.5 * np.cos(2 * np.pi * n / win_length)     # periodic Hann
    lpad = (n_fft - win_length) // 2
    win = np.zeros(n_fft)
    win[lpad:lpad + win_length] = w
    x = np.pad(wave.astype(np.float64), n_fft // 2, mode="reflect")
    Tn = 1 + len(wave) // hop
    out = np.empty((1 + n_fft // 2, Tn))
    for t in range(Tn):
        out[:, t] = np.abs(np.fft.rfft(x[t * hop:t * hop + n_fft] * win)) / norm
    out = np.log(1.0e-8 + out)
    return (out[:-1] if drop_nyquist else out).astype(np.float32)


def _clips(secs, fs=FS, base=40):
    from oracle import st_oracle as orc
    return [orc.synth_clip(base + i, (3 * i) % 10, seconds=s, fs=fs) for i, s in enumerate(secs)]


def test_stft_norm_divisor(dev):
    import pca_hip
    waves = _clips((0.5, 0.11, 0.37))
    quiet = waves[0].copy()
    quiet[2000:6000] = 0.0                                   # exact silence: the log floor
    waves.append(quiet)
    wd = [T(w, dev) for w in waves]
    for n_fft, win, drop in ((1024, 1024, True), (256, 200, False), (2048, 2048, False)):
        hop = win // 2
        for fm in (False, True):
            a, oa = pca_hip.stft_logmag_batch(wd, n_fft, win, hop, drop_nyquist=drop, frame_major=fm)
            b, ob = pca_hip.stft_logmag_batch(wd, n_fft, win, hop, drop_nyquist=drop, frame_major=fm,
                                              norm=n_fft)
            assert oa == ob and torch.equal(a, b), (n_fft, fm)
    for N in (1000, 200):
        n_fft = 1 << math.ceil(math.log2(N))
        hop = int(N * 0.5)
        spec, off = pca_hip.stft_logmag_batch(wd, n_fft, N, hop, drop_nyquist=True, norm=N)
        for c, w in enumerate(waves):
            ref = _np_stft_logmag_div(w, n_fft, N, hop, N, True)
            got = spec[:, off[c]:off[c + 1]].cpu().numpy()
            assert got.shape == ref.shape
            assert np.max(np.abs(got - ref)) < 5e-5, (N, c, float(np.max(np.abs(got - ref))))
        # the divisor is N, not n_fft: every bin moves by log(n_fft / N) against the plain call
        plain, _ = pca_hip.stft_logmag_batch(wd, n_fft, N, hop, drop_nyquist=True)
        d = (plain - spec)[spec > -15]
        assert abs(float(d.mean()) + math.log(n_fft / N)) < 1e-3
    with pytest.raises(pca_hip.PcaHipError):
        pca_hip.stft_logmag_batch(wd, 1024, norm=0.0)


def test_stft_frame_align(dev):
    """frame_align: every clip starts on a multiple of it, its frames unchanged, the gaps zero."""
    import pca_hip
    wd = [T(w, dev) for w in _clips((0.5, 0.11, 0.37, 0.23))]
    plain, po = pca_hip.stft_logmag_batch(wd, 512, 400, 200, drop_nyquist=True, frame_major=True,
                                          norm=400)
    al, ao = pca_hip.stft_logmag_batch(wd, 512, 400, 200, drop_nyquist=True, frame_major=True,
                                       norm=400, frame_align=10)
    assert all(o % 10 == 0 for o in ao) and al.shape[0] == ao[-1]
    filled = torch.zeros(al.shape[0], dtype=torch.bool, device=dev)
    for c in range(len(wd)):
        n = po[c + 1] - po[c]
        assert torch.equal(al[ao[c]:ao[c] + n], plain[po[c]:po[c + 1]])
        filled[ao[c]:ao[c] + n] = True
    assert bool((al[~filled] == 0).all())


# ----------------------------------------------------------------------------------------------- #
# sub-sampling sweeps                                                                              #
# ----------------------------------------------------------------------------------------------- #
@pytest.mark.parametrize("shape", ["shipped", "d128"])
def test_maxK_sweep_equals_item_path_fst(shape, dev, tmp_path):
    import dataset
    import evalsweep
    import utils
    from pca_hip import trainer
    x, y, farr = _fst_corpus()
    net = _net(2, shape, dev)
    full = (x.shape[1] // 8) * 8
    list_K = [1, 51, x.shape[0]]
    files = (str(tmp_path / "FST_randK_expt2.json"), str(tmp_path / "FST_maxK_expt2.json"))
    out_r, out_m = evalsweep.subsample_sweep(net, x, y, farr, list_K=list_K, n_runs=2,
                                             json_files=files)
    for K in list_K:
        xs, fss = utils.pc_maxK(x[:, :full], farr, K)
        acc, n = trainer.evaluate(net, dataset.ESC_pc_ss(xs, y[:full], fss, device=dev), 8)
        assert n == full
        assert out_m["data"][K] == [acc, 0], (K, out_m["data"][K], acc)
    back_r, back_m = json.load(open(files[0])), json.load(open(files[1]))
    assert back_m["list_K"] == list_K and back_r["list_K"] == list_K
    assert [float(v[0]) for v in back_m["data"].values()] == [out_m["data"][K][0] for K in list_K]
    assert list(back_r["data"].keys()) == [str(K) for K in list_K]


@pytest.mark.parametrize("shape", ["shipped", "d128"])
def test_maxK_sweep_equals_item_path_3st(shape, dev):
    import dataset
    import evalsweep
    from pca_hip import trainer
    x, y, farr, tarr = _3st_corpus()
    net = _net(3, shape, dev)
    full = (x.shape[2] // 8) * 8
    list_K = [1, 51, x.shape[0] * x.shape[1]]
    _, out_m = evalsweep.subsample_sweep(net, x, y, farr, tarr, list_K=list_K, n_runs=1)
    for K in list_K:
        ds = dataset.ESC_pc_temp_maxKSS(x[:, :, :full], y[:full], farr, tarr, K, device=dev)
        acc, n = trainer.evaluate(net, ds, 8)
        assert n == full
        assert out_m["data"][K] == [acc, 0], (K, out_m["data"][K], acc)


def _rerun(net, pts, lab, mode=0):
    from pca_hip import trainer
    eng = trainer.STEngine(net, pts.shape[0], pts.shape[1], mode, training=False)
    return int((eng.forward(pts.contiguous()).argmax(1) == lab).sum())


@pytest.mark.parametrize("kind", ["fst", "3st"])
def test_randK_sweep_reproduces_selections(kind, dev):
    """Each random run re-drawn with its (seed, draw, slot, set) keys - one selection launch over
    the first `full` sets, slot = set - and re-evaluated gives the driver's mean / variance; runs
    differ and every selection holds K distinct points."""
    import evalsweep
    import pca_hip
    if kind == "fst":
        x, y, farr = _fst_corpus(n=45)
        tarr, n = None, 45
    else:
        x, y, farr, tarr = _3st_corpus(n=21)
        n = 21
    din = 2 if tarr is None else 3
    net = _net(din, "shipped", dev)
    full = (n // 8) * 8
    n_runs, seed = 3, 11
    list_K = [1, 51, 400]
    # one engine call per selection launch (sets_per_call = full): the re-run below has the same B
    out_r, out_m = evalsweep.subsample_sweep(net, x, y, farr, tarr, list_K=list_K, n_runs=n_runs,
                                             seed=seed, sets_per_call=full)
    xs, lab, f32, t32 = evalsweep._resident_sets(x, y, farr, tarr, dev)
    pos = torch.arange(full, device=dev)
    for ki, K in enumerate(list_K):
        accs, sels = [], []
        for r in range(n_runs):
            pts, lb, sel = pca_hip.subsample_points(xs, f32, t32, pos, K, pca_hip.RANDK, seed,
                                                    evalsweep.sweep_draw(ki, r, n_runs), lab,
                                                    want_sel=True)
            accs.append(_rerun(net, pts, lb) / full)
            s = sel.cpu().numpy()
            assert all(len(set(row.tolist())) == K for row in s), (K, r)
            sels.append(s)
        accs = np.array(accs)
        assert out_r["data"][K] == [float(np.mean(accs)), float(np.var(accs))], (K, accs)
        if K > 1:
            assert not np.array_equal(sels[0], sels[1]) and not np.array_equal(sels[1], sels[2])
        pts, lb = pca_hip.subsample_points(xs, f32, t32, pos, K, pca_hip.MAXK, seed, 0, lab)
        assert out_m["data"][K] == [_rerun(net, pts, lb) / full, 0]
    # the same sweep with the default grouping (all runs and the max-K pass in one engine call)
    out_r2, out_m2 = evalsweep.subsample_sweep(net, x, y, farr, tarr, list_K=list_K,
                                               n_runs=n_runs, seed=seed)
    assert out_r2 == out_r and out_m2 == out_m
    # another seed draws other selections
    _, _, sel_a = pca_hip.subsample_points(xs, f32, t32, pos, 51, pca_hip.RANDK, seed,
                                           evalsweep.sweep_draw(1, 0, n_runs), lab, want_sel=True)
    _, _, sel_b = pca_hip.subsample_points(xs, f32, t32, pos, 51, pca_hip.RANDK, seed + 1,
                                           evalsweep.sweep_draw(1, 0, n_runs), lab, want_sel=True)
    assert not torch.equal(sel_a, sel_b)


def test_importance_sweep_reproduces_selections(dev, tmp_path):
    import dataset
    import evalsweep
    import pca_hip
    from pca_hip import trainer
    x, y, farr, tarr = _3st_corpus(n=19)
    net = _net(3, "shipped", dev)
    full = 16
    n_runs, seed = 2, 5
    list_K, list_winF = [1, 51, 700], [64, 8]
    files = (str(tmp_path / "3ST_rebut_expt_randK.json"), str(tmp_path / "3ST_rebut_expt_maxK.json"))
    out_r, out_m = evalsweep.importance_sweep(net, x, y, farr, tarr, list_K=list_K,
                                              list_winF=list_winF, n_runs=n_runs, seed=seed,
                                              json_files=files, sets_per_call=full)
    xs, lab, f32, t32 = evalsweep._resident_sets(x, y, farr, tarr, dev)
    pos = torch.arange(full, device=dev)
    for wi, winF in enumerate(list_winF):
        kern = pca_hip.importance_kernel(winF).to(dev)
        for ki, K in enumerate(list_K):
            accs, sels = [], []
            for r in range(n_runs):
                d = evalsweep.sweep_draw(wi * len(list_K) + ki, r, n_runs)
                pts, lb, sel = pca_hip.importance_points(xs, f32, t32, pos, K, 0, kern, seed, d,
                                                         lab, want_sel=True)
                accs.append(_rerun(net, pts, lb) / full)
                sels.append(sel)
            accs = np.array(accs)
            assert out_r["data"][winF][K] == [float(np.mean(accs)), float(np.var(accs))]
            if K > 1:
                assert not torch.equal(sels[0], sels[1])
            # choice 1 is exact: the item-level dataset gives the same accuracy
            ds = dataset.ESC_pc_temp_importancerandKSS(x[:, :, :full], y[:full], farr, tarr, K, 1,
                                                       winF, device=dev)
            acc, n = trainer.evaluate(net, ds, 8)
            assert out_m["data"][winF][K] == [acc, 0], (winF, K)
    back = json.load(open(files[1]))
    assert list(back["data"].keys()) == ["64", "8"] and back["list_K"] == list_K
    assert list(back["data"]["8"].keys()) == [str(K) for K in list_K]
    assert json.load(open(files[0]))["data"]["64"]["51"] == out_r["data"][64][51]


# ----------------------------------------------------------------------------------------------- #
# 3-D re-framing sweep                                                                             #
# ----------------------------------------------------------------------------------------------- #
def _host_temporal(net, waves, labels, fs, N, Ntemp, hf, dev, spectra=None):
    """Code/pc_temp3d_eval.py:70-99 on the host: spectrum / N, hsplit, the tail dropped, ESC_pc_temp,
    trainer.evaluate over the full batches in order.  ``spectra``: per-clip spectra to use instead of
    the numpy restatement."""
    import dataset
    from pca_hip import trainer
    n_fft = 1 << math.ceil(math.log2(N))
    hop = int(N * hf)
    d_esc, l_esc = [], []
    for i, w in enumerate(waves):
        a = _np_stft_logmag_div(w, n_fft, N, hop, N, True) if spectra is None else spectra[i]
        for ss in np.hsplit(a, np.arange(0, a.shape[1], Ntemp)):
            if ss.shape[1] < Ntemp:
                continue
            d_esc.append(ss)
            l_esc.append(labels[i])
    x = np.dstack(d_esc)
    y = np.array(l_esc).astype(int)
    full = (x.shape[2] // 8) * 8
    farr = np.linspace(0, fs / 2, x.shape[0]) / fs
    tarr = np.linspace(0, ((hf * N) / fs) * Ntemp, Ntemp)
    ds = dataset.ESC_pc_temp(x[:, :, :full], y[:full], farr, tarr, device=dev)
    acc, n = trainer.evaluate(net, ds, 8)
    return acc, full


def _device_spectra(waves_d, N, hf):
    import pca_hip
    n_fft = 1 << math.ceil(math.log2(N))
    out = []
    for w in waves_d:
        s, _ = pca_hip.stft_logmag_batch([w], n_fft, N, int(N * hf), drop_nyquist=True, norm=N)
        out.append(s.cpu().numpy())
    return out


@pytest.mark.parametrize("shape", ["shipped", "d128"])
def test_reframe_sweep_temporal_equals_host_construction(shape, dev, tmp_path):
    import evalsweep
    import pca_hip
    waves = _clips((1.6, 1.1, 2.0, 0.9, 1.3), base=70)
    labels = [3, 1, 4, 1, 5]
    wd = [T(w, dev) for w in waves]
    net = _net(3, shape, dev, seed=2)
    list_N, Ntemp, hf = [1024, 1000, 512, 200], 10, 0.5
    Fs2 = 16000.0
    jf = str(tmp_path / "3ST_expt1.json")
    out = evalsweep.reframe_sweep_temporal(net, wd, labels, FS, list_N, Ntemp, hf,
                                           list_Fs=[FS, Fs2], json_file=jf)
    assert out["list_N"] == list_N and out["list_Fs"] == [FS, Fs2]
    for j, N in enumerate(list_N):
        # bit-exact against the same construction from the device spectrum of each clip
        acc, full = _host_temporal(net, waves, labels, FS, N, Ntemp, hf, dev,
                                   spectra=_device_spectra(wd, N, hf))
        assert out["data"][FS][j] == acc, (N, out["data"][FS][j], acc)
        # and against the numpy restatement (log-magnitudes within 5e-5: at most a flip)
        acc_np, full = _host_temporal(net, waves, labels, FS, N, Ntemp, hf, dev)
        assert abs(out["data"][FS][j] - acc_np) <= 1.0 / full + 1e-12, (N, acc_np)
        # the resampled rate: pca_hip.resample, then the same construction at Fs2
        rs = [pca_hip.resample(w, FS, Fs2, scale=True) for w in wd]
        acc_rs, _ = _host_temporal(net, [r.cpu().numpy() for r in rs], labels, Fs2, N, Ntemp, hf,
                                   dev, spectra=_device_spectra(rs, N, hf))
        assert out["data"][Fs2][j] == acc_rs, (N, out["data"][Fs2][j], acc_rs)
    back = json.load(open(jf))
    assert back["list_N"] == list_N and back["list_Fs"] == [FS, Fs2]
    assert list(back["data"].keys()) == [str(FS), str(Fs2)]
    assert back["data"][str(FS)] == out["data"][FS]
    # engine calls of a few sets at a time give the same counts
    out2 = evalsweep.reframe_sweep_temporal(net, wd, labels, FS, list_N[:2], Ntemp, hf,
                                            sets_per_call=5)
    assert out2["data"][FS] == out["data"][FS][:2]
