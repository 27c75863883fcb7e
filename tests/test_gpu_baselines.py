"""The baselines' forwards on the device (pca_fb_forward / pca_cnn_temp_forward through
pca_hip.BaselineEngine) and their sweeps (evalsweep.baseline_*): against the reference's recorded
outputs (golden_baselines*.npz, golden_base.npz), against the zero-filled dense inputs the
reference builds, against pca_subsample_points' selections, and against the host item route."""
import numpy as np
import pytest
import torch

import baseline_ref as br
import inputs as gi
import inputs_baselines as gb

pytestmark = pytest.mark.gpu

FS = 22050
FLOOR = float(np.float32(np.log(1e-8)))          # log(1e-8 + 0): silent bins


@pytest.fixture(scope="module")
def dev():
    return torch.device("cuda", 0)


def _model(kind, dev):
    """(stock torch module with the golden weights, eval mode, on dev; its engine)."""
    import models
    import pca_hip
    if kind == "fb":
        m, p = models.baseline_ff(gb.FB_DIMS, gb.NCLASS), br.shipped_params("fb")
    elif kind == "cnn":
        m, p = models.CNN_classifier(gb.NT, gb.NF, gb.CNN_DIMS, gb.NCLASS), \
            br.shipped_params("cnntemp")
    elif kind == "ff_small":
        m, p = models.baseline_ff(gi.BASE_FF_DIMS, gi.BASE_NCLASS), br.small_params("ff")
    else:
        m, p = models.CNN_classifier(gi.BASE_NT, gi.BASE_NF, gi.BASE_CNN_DIMS, gi.BASE_NCLASS), \
            br.small_params("cnn")
    m.load_state_dict({k: torch.from_numpy(np.ascontiguousarray(v)) for k, v in p.items()})
    m = m.to(dev).eval()
    return m, pca_hip.BaselineEngine(m)


def _spec(x, cnn, dev):
    """Reference-layout items (FB [S, F], CNN_temp [S, Nt, Nf]) -> the resident spectrogram the
    engine reads (FB [F, T], CNN_temp [F, Nt, S])."""
    x = torch.as_tensor(np.ascontiguousarray(x), dtype=torch.float32).to(dev)
    return x.permute(2, 1, 0) if cnn else x.t()


def _items(spec, cnn):
    return spec.permute(2, 1, 0) if cnn else spec.t()


def _fwd(eng, spec, **kw):
    idx = torch.arange(spec.shape[-1], dtype=torch.int64, device=spec.device)
    return eng.forward(spec, idx, **kw)


# ---- 1. forwards against the reference ----------------------------------------------------------- #
@pytest.mark.parametrize("kind", ["fb", "cnn", "ff_small", "cnn_small"])
def test_forward_matches_reference(kind, dev):
    cnn = kind.startswith("cnn")
    _, eng = _model(kind, dev)
    if kind == "fb":
        x, ref = gb.fb_frames(), np.load(f"{br.GOLDEN}/golden_baselines.npz")["fb/y"]
    elif kind == "cnn":
        x, ref = gb.cnn_chunks(), np.load(f"{br.GOLDEN}/golden_baselines.npz")["cnn/y"]
    elif kind == "ff_small":
        x, ref = gi.base_ff_input(), np.load(f"{br.GOLDEN}/golden_base.npz")["ff/y"]
    else:
        x, ref = gi.base_cnn_input(), np.load(f"{br.GOLDEN}/golden_base.npz")["cnn/y"]
    got = _fwd(eng, _spec(x, cnn, dev))[0].cpu().numpy()
    assert got.shape == ref.shape
    err = np.abs(got - ref).max()
    assert err <= 1e-5 * np.abs(ref).max(), (kind, err)
    assert (got.argmax(1) == ref.argmax(1)).all()


# ---- 2. fused max-K against the zero-filled dense input ---------------------------------------- #
def _with_floor_ties(x, frac, seed):
    rng = np.random.Generator(np.random.PCG64(seed))
    x = x.copy()
    x[rng.random(x.shape) < frac] = FLOOR
    return x


@pytest.mark.parametrize("kind", ["fb", "cnn"])
def test_fused_maxK_equals_dense_zero_fill(kind, dev):
    import dataset
    import pca_hip
    import utils
    cnn = kind == "cnn"
    model, eng = _model(kind, dev)
    gbl = np.load(f"{br.GOLDEN}/golden_baselines.npz")
    # (a) tie-free sets: the reference's own zero-filled items
    x = (gb.cnn_chunks() if cnn else gb.fb_frames())[:gb.MAXK_SETS]
    spec = _spec(x, cnn, dev)
    for K in gb.MAXK_K[kind]:
        dense = _spec(gbl[f"{kind}/maxK{K}"], cnn, dev)
        fused = _fwd(eng, spec, K=K, mode=pca_hip.MAXK)[0]
        ref = _fwd(eng, dense)[0]
        assert float((fused - ref).abs().max()) <= 1e-6, K
        assert torch.equal(fused.argmax(1), ref.argmax(1))
    # (b) sets with many cells at the log(1e-8) floor: ties in the kept set's boundary
    x = _with_floor_ties(gb.cnn_chunks() if cnn else gb.fb_frames(), 0.4, 7)
    spec = _spec(x, cnn, dev)
    n = x[0].size
    for K in (1, 51, 501, n - 3, n):
        fused, _, sel = _fwd(eng, spec, K=K, mode=pca_hip.MAXK, want_sel=True)
        if cnn:
            # ESC_baseline_temporal_maxK(flag="max") with the tie order pinned to the selection
            ds = dataset.ESC_baseline_temporal_maxK(x.transpose(2, 1, 0), np.zeros(len(x), int), K)
            dense_items = np.stack([ds[i][1].numpy() for i in range(len(x))])
            vals = x.reshape(len(x), -1)
            keep = np.zeros_like(vals, dtype=bool)
            np.put_along_axis(keep, sel.cpu().numpy().astype(np.int64), True, axis=1)
            dense = np.where(keep, vals, 0).reshape(x.shape).astype(np.float32)
            # the reference's unstable argsort may pick other floor cells; values equal elsewhere
            diff = dense_items != dense
            assert np.all((dense_items[diff] == FLOOR) | (dense[diff] == FLOOR))
        else:
            dense = utils.pc_maxK_replace(x.T, K).T.astype(np.float32)     # Code/utils.py:86-96
        ref = _fwd(eng, _spec(dense, cnn, dev))[0]
        assert float((fused - ref).abs().max()) <= 1e-6, K
        assert torch.equal(fused.argmax(1), ref.argmax(1))
        with torch.no_grad():
            stock = model(_items(_spec(dense, cnn, dev), cnn))
        assert float((fused - stock).abs().max()) <= 1e-5 * float(stock.abs().max())


# ---- 3. random-K keeps pca_subsample_points' cells ----------------------------------------------- #
@pytest.mark.parametrize("kind", ["fb", "cnn"])
def test_randK_keeps_subsample_points_selection(kind, dev):
    import pca_hip
    cnn = kind == "cnn"
    _, eng = _model(kind, dev)
    x = _with_floor_ties(gb.cnn_chunks() if cnn else gb.fb_frames(), 0.2, 3)
    spec = _spec(x, cnn, dev)
    F = spec.shape[0]
    farr = torch.zeros(F, device=dev)
    tarr = torch.zeros(gb.NT, device=dev) if cnn else None
    idx = torch.tensor([5, 0, 5, 9, 2, 9], dtype=torch.int64, device=dev)   # repeated sets
    step = torch.tensor([17], dtype=torch.int32, device=dev)
    for mode in (pca_hip.RANDK, pca_hip.MAXK):
        for K, seed, draw, dd in ((1, 0, 1, None), (51, 3, 8, None), (700, 11, 2, step)):
            got, _, sel = eng.forward(spec, idx, K, mode, seed, draw, draw_dev=dd, want_sel=True)
            _, _, ref_sel = pca_hip.subsample_points(spec, farr, tarr, idx, K, mode, seed, draw,
                                                     want_sel=True, draw_dev=dd)
            assert torch.equal(sel, ref_sel), (mode, K, seed)
            # and the output is the forward of exactly those cells
            vals = _items(spec, cnn)[idx].reshape(idx.numel(), -1)
            keep = torch.zeros_like(vals, dtype=torch.bool)
            keep.scatter_(1, sel.long(), True)
            dense = torch.where(keep, vals, torch.zeros_like(vals)).reshape(
                (idx.numel(),) + tuple(_items(spec, cnn).shape[1:]))
            ref = _fwd(eng, _spec(dense.cpu().numpy(), cnn, dev))[0]
            assert float((got - ref).abs().max()) <= 1e-6
    a = eng.forward(spec, idx, 51, pca_hip.RANDK, 0, 1, want_sel=True)[2]
    b = eng.forward(spec, idx, 51, pca_hip.RANDK, 1, 1, want_sel=True)[2]
    assert not torch.equal(a, b)


# ---- 4. sub-sampling sweeps ---------------------------------------------------------------------- #
def _corpus(kind, n, seed):
    rng = np.random.Generator(np.random.PCG64(seed))
    shape = (n, gb.NT, gb.NF) if kind == "cnn" else (n, gb.FB_DIMS[0])
    x = rng.normal(-9, 3, size=shape).astype(np.float32)
    x[rng.random(shape) < 0.1] = FLOOR
    return x, rng.integers(0, 10, size=n)


def _host_maxK_accuracy(model, x, y, K, kind, dev):
    """The item route of Code/baseline_eval.py:170-190 / baseline_temp_eval.py:171-193: zero-filled
    items, the stock model, batches of 128 (FB) / 2 with a trailing single set skipped (CNN_temp)."""
    import dataset
    import utils
    if kind == "fb":
        items = torch.from_numpy(utils.pc_maxK_replace(x.T, K).T).float()
        bs, keep_short = 128, True
    else:
        ds = dataset.ESC_baseline_temporal_maxK(x.transpose(2, 1, 0), y, K, "max")
        items = torch.stack([ds[i][1] for i in range(len(ds))]).float()
        bs, keep_short = 2, False
    correct = total = 0
    with torch.no_grad():
        for a in range(0, len(x), bs):
            xb = items[a:a + bs].to(dev)
            if xb.shape[0] < bs and not keep_short:
                continue
            correct += int((model(xb).argmax(1).cpu() == torch.from_numpy(y[a:a + bs])).sum())
            total += xb.shape[0]
    return correct / total


@pytest.mark.parametrize("kind", ["fb", "cnn"])
def test_maxK_sweep_equals_host_item_route(kind, dev, tmp_path):
    import evalsweep
    model, eng = _model(kind, dev)
    x, y = _corpus(kind, 61 if kind == "fb" else 27, 5)     # tie-free only where it matters
    x = x + np.arange(x[0].size, dtype=np.float32).reshape(x[0].shape) * 1e-4   # no ties
    spec = _spec(x, kind == "cnn", dev)
    list_K = [1, 51, 501] + ([1024] if kind == "fb" else [5120])
    out_r, out_m = evalsweep.baseline_subsample_sweep(eng, spec, y, list_K, n_runs=3,
                                                      json_files=(str(tmp_path / "r.json"),
                                                                  str(tmp_path / "m.json")))
    for K in list_K:
        assert out_m["data"][K][0] == _host_maxK_accuracy(model, x, y, K, kind, dev), K
    # random-K: reproducible across calls, changes with the seed
    again = evalsweep.baseline_subsample_sweep(eng, spec, y, list_K, n_runs=3)
    assert again[0] == out_r and again[1] == out_m
    other = evalsweep.baseline_subsample_sweep(eng, spec, y, list_K, n_runs=3, seed=9)
    assert other[1] == out_m and other[0] != out_r


# ---- 5. (Fs, N) re-framing sweeps ----------------------------------------------------------------- #
def _clips(secs, fs=FS, base=60):
    from oracle import st_oracle as orc
    return [orc.synth_clip(base + i, (3 * i) % 10, seconds=s, fs=fs) for i, s in enumerate(secs)]


def test_reframe_sweeps_equal_host_construction(dev):
    import evalsweep
    import pca_hip
    clips = _clips((0.9, 0.4, 1.3, 0.6))
    labels = [3, 7, 1, 3]
    wd = [torch.from_numpy(c).float().to(dev) for c in clips]
    for kind in ("fb", "cnn"):
        model, eng = _model(kind, dev)
        n_fft = 2048 if kind == "fb" else 1024
        list_N = [n_fft, int(0.7 * n_fft), int(0.25 * n_fft)]
        if kind == "fb":
            out = evalsweep.baseline_reframe_sweep(eng, wd, labels, FS, list_N)
        else:
            out = evalsweep.baseline_reframe_sweep_temporal(eng, wd, labels, FS, list_N)
        assert out["list_N"] == list_N and out["list_Fs"] == [FS]
        for N, acc in zip(list_N, out["data"][FS]):
            hop = int(N * 0.5)
            items, ys = [], []
            for w, lab in zip(wd, labels):
                s = pca_hip.stft_logmag(w, n_fft, win_length=N, hop=hop,
                                        drop_nyquist=kind == "cnn")          # [F, T] / n_fft
                if kind == "fb":
                    items.append(s.t())
                    ys += [lab] * s.shape[1]
                else:
                    for a in range(0, s.shape[1], gb.NT):                  # hsplit, tail dropped
                        if a + gb.NT <= s.shape[1]:
                            items.append(s[:, a:a + gb.NT].t()[None])
                            ys.append(lab)
            items = torch.cat(items)
            ys = torch.tensor(ys)
            full = len(ys) if kind == "fb" else (len(ys) // 2) * 2
            with torch.no_grad():
                pred = model(items[:full]).argmax(1).cpu()
            assert acc == int((pred == ys[:full]).sum()) / full, (kind, N)


# ---- 6. determinism -------------------------------------------------------------------------------- #
@pytest.mark.parametrize("kind", ["fb", "cnn"])
def test_same_call_twice_is_bitwise_equal(kind, dev):
    import pca_hip
    cnn = kind == "cnn"
    _, eng = _model(kind, dev)
    spec = _spec(gb.cnn_chunks() if cnn else gb.fb_frames(), cnn, dev)
    for mode, K in ((pca_hip.SEL_ALL, None), (pca_hip.MAXK, 77), (pca_hip.RANDK, 300)):
        a = _fwd(eng, spec, K=K, mode=mode, seed=4, draw=2)[0]
        b = _fwd(eng, spec, K=K, mode=mode, seed=4, draw=2)[0]
        assert torch.equal(a, b), mode
