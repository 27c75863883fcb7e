"""Host-side checks of the baseline forwards (FB, CNN_temp) and their sweeps: a float64 numpy
restatement of both models against the reference's recorded outputs, the C ABI surface, and the
JSON the sweeps write.  No GPU."""
import ctypes
import json
import os
import re

import numpy as np
import pytest
import torch

import baseline_ref as br
import inputs as gi
import inputs_baselines as gb

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_SYMBOLS = ["pca_baseline_param_count", "pca_fb_forward", "pca_cnn_temp_forward"]


@pytest.fixture(scope="module")
def gbl():
    return np.load(os.path.join(br.GOLDEN, "golden_baselines.npz"))


def test_restated_forwards_match_golden_base():
    z = np.load(os.path.join(br.GOLDEN, "golden_base.npz"))
    y = br.fb_forward64(gi.base_ff_input(), br.small_params("ff"))
    np.testing.assert_allclose(y, z["ff/y"], rtol=0, atol=1e-6)
    y = br.cnn_forward64(gi.base_cnn_input(), br.small_params("cnn"))
    np.testing.assert_allclose(y, z["cnn/y"], rtol=0, atol=1e-5 * np.abs(z["cnn/y"]).max())


def test_restated_forwards_match_shipped_fixture(gbl):
    p = br.shipped_params("fb")
    assert [v.shape for v in p.values()] == [(513, 1025), (513,), (256, 513), (256,), (10, 256),
                                             (10,)]
    y = br.fb_forward64(gb.fb_frames(), p)
    ref = gbl["fb/y"]
    np.testing.assert_allclose(y, ref, rtol=0, atol=1e-5 * np.abs(ref).max())
    assert (y.argmax(1) == ref.argmax(1)).all()
    p = br.shipped_params("cnntemp")
    assert sum(v.size for v in p.values()) == 158049
    y = br.cnn_forward64(gb.cnn_chunks(), p)
    ref = gbl["cnn/y"]
    np.testing.assert_allclose(y, ref, rtol=0, atol=1e-5 * np.abs(ref).max())
    assert (y.argmax(1) == ref.argmax(1)).all()


def test_fixture_maxK_items_are_stable_max_selections(gbl):
    """The reference's zero-filled items on tie-free inputs keep the K largest cells, in the
    time-major cell order p = t*F + f for CNN_temp."""
    xf = gb.fb_frames()[:gb.MAXK_SETS]
    for K in gb.MAXK_K["fb"]:
        np.testing.assert_array_equal(gbl[f"fb/maxK{K}"], br.maxK_replace64(xf, K))
    xc = gb.cnn_chunks()[:gb.MAXK_SETS]                       # [S, Nt, Nf]
    for K in gb.MAXK_K["cnn"]:
        flat = br.maxK_replace64(xc.reshape(gb.MAXK_SETS, -1), K).reshape(xc.shape)
        np.testing.assert_array_equal(gbl[f"cnn/maxK{K}"], flat)
        assert (gbl[f"cnn/maxK{K}"] != 0).sum() == K * gb.MAXK_SETS


def test_header_declares_and_library_exports_the_baseline_entry_points():
    txt = open(os.path.join(ROOT, "include", "pca_hip.h")).read()
    body = re.sub(r"/\*.*?\*/", "", txt, flags=re.S)
    from pca_hip import _lib
    handle = ctypes.CDLL(_lib.LIB_PATH)
    for s in NEW_SYMBOLS:
        assert re.search(r"\b%s\s*\(" % s, body), s
        assert s in _lib.SIGNATURES, s
        assert hasattr(handle, s), s
    for s in ("PCA_SEL_MAXK = 0", "PCA_SEL_RANDK = 1", "PCA_SEL_ALL = 2"):
        assert s in body


def _count(cnn, Nt, Nf, dims, C):
    from pca_hip import _lib
    arr = (ctypes.c_int * len(dims))(*dims)
    return _lib.lib().pca_baseline_param_count(int(cnn), Nt, Nf, arr, len(dims), C)


def test_param_count_and_refused_shapes():
    assert _count(0, 1, 0, [1025, 513, 256], 10) == 660492          # FB config model_params
    assert _count(1, 10, 512, [512, 256, 100], 10) == 158049        # CNNTemp config model_params
    assert _count(0, 1, 0, gi.BASE_FF_DIMS, gi.BASE_NCLASS) == \
        sum(v.size for v in br.small_params("ff").values())
    assert _count(1, gi.BASE_NT, gi.BASE_NF, gi.BASE_CNN_DIMS, gi.BASE_NCLASS) == \
        sum(v.size for v in br.small_params("cnn").values())
    assert _count(1, 10, 512, [600, 256], 10) == -1                  # conv width < 1
    assert _count(0, 1, 0, [], 10) == -1
    assert _count(0, 1, 0, [0, 4], 10) == -1


def test_baseline_config_reads_the_models():
    import models
    from pca_hip.baseline import baseline_config
    assert baseline_config(models.baseline_ff([1025, 513, 256], 10)) == \
        (False, 1, 0, [1025, 513, 256], 10)
    assert baseline_config(models.CNN_classifier(10, 512, [512, 256, 100], 10)) == \
        (True, 10, 512, [512, 256, 100], 10)
    assert baseline_config(torch.nn.DataParallel(models.CNN_classifier(4, 24, [20, 12, 6], 5))) \
        == (True, 4, 24, [20, 12, 6], 5)


class _FakeEngine:
    """Stands in for BaselineEngine where only its shape and device are read."""

    def __init__(self, cnn):
        from pca_hip.baseline import BaselineEngine
        self.__class__ = type("Fake", (BaselineEngine,), {})
        self.cnn, self.dev, self.nclasses = cnn, torch.device("cpu"), 10


def _ref_two_dicts(list_K, n_runs, full, per_slot):
    """The dictionaries Code/baseline_eval.py:115-200 / Code/baseline_temp_eval.py:114-200 build."""
    lk = np.asarray(list_K)
    dr = {"data": {(int)(k): 0 for k in lk}}
    dm = {"data": {(int)(k): 0 for k in lk}}
    dm["list_K"] = lk.tolist()
    dr["list_K"] = lk.tolist()
    for Km in lk:
        vals = np.array([(per_slot(r, int(Km)) * full // 16) / full for r in range(n_runs)])
        dr["data"][(int)(Km)] = [np.mean(vals), np.var(vals)]
        dm["data"][(int)(Km)] = [(per_slot(n_runs, int(Km)) * full // 16) / full, 0]
    return dr, dm


@pytest.mark.parametrize("kind", ["fb", "cnn"])
def test_baseline_subsample_sweep_json_layout(kind, tmp_path, monkeypatch):
    import evalsweep
    per_slot = lambda slot, K: (slot * 5 + K) % 16           # noqa: E731
    seen = []

    def run(eng, x, lab, ids, pieces, counts, K=None, sel_of_slot=None, seed=0, cap=None):
        seen.append((K, list(pieces), [sel_of_slot(s) for s, _, _, _ in pieces]))
        for slot, draw, p0, p1 in pieces:
            counts[slot] += per_slot(slot, K) * (p1 - p0) // 16

    monkeypatch.setattr(evalsweep, "_baseline_run", run)
    rng = np.random.default_rng(0)
    if kind == "fb":
        n = 203
        spec = rng.normal(size=(1025, n)).astype(np.float32)
        list_K, full = np.arange(1, 1024, 50), n                     # every frame counts
        list_K[-1] = 1024
    else:
        n = 61
        spec = rng.normal(size=(16, 10, n)).astype(np.float32)
        list_K, full = np.arange(1, 160, 50), 60                     # trailing one-set batch
        list_K[-1] = 160
    y = rng.integers(0, 10, size=n)
    files = (str(tmp_path / "randK.json"), str(tmp_path / "maxK.json"))
    out_r, out_m = evalsweep.baseline_subsample_sweep(_FakeEngine(kind == "cnn"), spec, y,
                                                      n_runs=4, json_files=files)
    ref_r, ref_m = _ref_two_dicts(list_K, 4, full, per_slot)
    assert open(files[0]).read() == json.dumps(ref_r)
    assert open(files[1]).read() == json.dumps(ref_m)
    assert json.dumps(out_r) == json.dumps(ref_r) and json.dumps(out_m) == json.dumps(ref_m)
    assert [s[0] for s in seen] == list_K.tolist()
    for K, pieces, modes in seen:
        assert [(slot, p0, p1) for slot, _, p0, p1 in pieces] == [(r, 0, full) for r in range(5)]
        assert modes == [1, 1, 1, 1, 0]                              # RANDK runs, then MAXK
    draws = [d for s in seen for (slot, d, _, _) in s[1] if slot < 4]
    assert len(set(draws)) == len(draws) == 4 * len(list_K)


def test_baseline_reframe_json_layout(tmp_path, monkeypatch):
    """{"data": {Fs: [acc per N]}, "list_Fs", "list_N"}: Code/baseline_eval.py:54-103."""
    import evalsweep

    def frames(clips, labels, N, n_fft, hf=0.5):
        assert n_fft == 2048                                         # the model's window
        return torch.zeros(1025, 10 + N % 7), torch.zeros(10 + N % 7, dtype=torch.int64)

    def run(eng, x, lab, ids, pieces, counts, K=None, sel_of_slot=None, seed=0, cap=None):
        assert sel_of_slot is None and pieces == [(0, 0, 0, x.shape[1])]
        counts[0] += 3

    monkeypatch.setattr(evalsweep, "baseline_frames", frames)
    monkeypatch.setattr(evalsweep, "_baseline_run", run)
    eng = _FakeEngine(False)
    eng.layer_dims, eng.Nf = [1025, 513, 256], 0
    path = str(tmp_path / "FB_expt1.json")
    list_N = [2048, 1945, 204]
    out = evalsweep.baseline_reframe_sweep(eng, [None], [0], 44100, list_N, json_file=path)
    ref = {"data": {44100: [3 / (10 + n % 7) for n in list_N]}, "list_Fs": [44100],
           "list_N": list_N}
    assert open(path).read() == json.dumps(ref) and json.dumps(out) == json.dumps(ref)


def test_bad_shapes_are_refused_before_any_launch():
    """PCA_EINVAL with a message, decided from the arguments alone (the pointers are never read)."""
    from pca_hip import _lib
    L = _lib.lib()
    fake = ctypes.c_void_p(4096)
    dims = [1025, 513, 256]
    fb_n = _count(0, 1, 0, dims, 10)
    cdims = [512, 256, 100]
    cnn_n = _count(1, 10, 512, cdims, 10)

    def fb(F, K, mode, n=fb_n, d=dims):
        arr = (ctypes.c_int * len(d))(*d)
        return L.pca_fb_forward(fake, 1, F, fake, 4, F, arr, len(d), 10, fake, n, K, mode, 0, 0,
                                None, fake, None, None, None, None)

    def cnn(F, Nt, Nf, K, mode, n=cnn_n):
        arr = (ctypes.c_int * 3)(*cdims)
        return L.pca_cnn_temp_forward(fake, 1, F, F * Nt, fake, 4, F, Nt, Nf, arr, 3, 10, fake, n,
                                      K, mode, 0, 0, None, fake, None, None, None, None)

    cases = [
        (lambda: fb(1024, 5, 0), "layer_dims[0]"),            # F != layer_dims[0]
        (lambda: fb(1025, 0, 0), "outside"),                  # K < 1
        (lambda: fb(1025, 1026, 1), "outside"),               # K > N
        (lambda: fb(1025, 5, 3), "mode"),
        (lambda: fb(1025, 5, 0, n=fb_n - 1), "weights"),
        (lambda: cnn(500, 10, 512, 5, 0), "Nf"),              # F != Nf
        (lambda: cnn(512, 10, 512, 5121, 0), "outside"),
        (lambda: cnn(512, 40, 512, 5, 1, n=_count(1, 40, 512, cdims, 10)), "16384"),
    ]
    for call, word in cases:
        rc = call()
        assert rc == -1, word
        assert word in L.pca_last_error().decode(), (word, L.pca_last_error())
