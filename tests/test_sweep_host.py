"""Host-side pieces of the batch-scale sweeps (evalsweep.subsample_sweep / importance_sweep /
reframe_sweep_temporal): the K grid, the JSON the reference writes, the chunk plan and the 3-D axes.
No GPU: the engine pass is replaced by a stand-in that fills the counters."""
import json
import math

import numpy as np
import pytest
import torch

import evalsweep


def _ref_list_K(n):
    # Code/pceval.py:111-112, Code/pc_temp3d_eval.py:113-114
    list_K = np.arange(1, n, 50)
    list_K[-1] = n
    return list_K


@pytest.mark.parametrize("n", [2048 // 2, 1024 * 10 // 2, 77, 51, 52])
def test_default_list_K_matches_reference(n):
    got = evalsweep.default_list_K(n)
    ref = _ref_list_K(n)
    assert got == ref.tolist()
    assert all(type(k) is int for k in got)


def test_default_list_K_shipped_lengths():
    assert len(evalsweep.default_list_K(1024)) == 21
    assert len(evalsweep.default_list_K(5120)) == 103
    assert evalsweep.default_list_K(5120)[-1] == 5120


def test_sweep_draws_are_distinct():
    n_runs, n_K = 10, 103
    d = {evalsweep.sweep_draw(i, r, n_runs) for i in range(n_K) for r in range(n_runs)}
    assert len(d) == n_runs * n_K and min(d) >= 1


class _Net(torch.nn.Module):
    """Stands in for models.ST where only the parameters' device is read."""

    def __init__(self):
        super().__init__()
        self.w = torch.nn.Parameter(torch.zeros(1))


def _fake_pass(per_slot):
    """_run_pieces stand-in: counts[slot] += per_slot(slot, K) * (p1 - p0) // 16, recording the
    pieces it was handed."""
    seen = []

    def run(model, npts, din, mode, cap, pieces, select, counts):
        seen.append((npts, din, list(pieces)))
        for slot, draw, p0, p1 in pieces:
            counts[slot] += per_slot(slot, npts) * (p1 - p0) // 16
    return run, seen


def _ref_two_dicts(list_K, n_runs, full, per_slot, nest=None):
    """The dictionaries Code/pceval.py:116-188 (or, nested by winF, Code/rebut_expts.py:64-145)
    build, from the same counts."""
    lk = np.asarray(list_K)
    if nest is None:
        dr = {"data": {(int)(k): 0 for k in lk}}
        dm = {"data": {(int)(k): 0 for k in lk}}
    else:
        dr = {"data": {(int)(w): {(int)(k): 0 for k in lk} for w in nest}}
        dm = {"data": {(int)(w): {(int)(k): 0 for k in lk} for w in nest}}
    dm["list_K"] = lk.tolist()
    dr["list_K"] = lk.tolist()
    for w in (nest or [None]):
        for Km in lk:
            vals = np.array([(per_slot(r, int(Km)) * full // 16) / full for r in range(n_runs)])
            r_ = [np.mean(vals), np.var(vals)]
            m_ = [(per_slot(n_runs, int(Km)) * full // 16) / full, 0]
            if w is None:
                dr["data"][(int)(Km)] = r_
                dm["data"][(int)(Km)] = m_
            else:
                dr["data"][w][Km] = r_
                dm["data"][w][Km] = m_
    return dr, dm


@pytest.mark.parametrize("kind", ["fst", "3st"])
def test_subsample_sweep_json_layout(kind, tmp_path, monkeypatch):
    per_slot = lambda slot, K: (slot * 3 + K) % 16           # noqa: E731
    run, seen = _fake_pass(per_slot)
    monkeypatch.setattr(evalsweep, "_run_pieces", run)
    monkeypatch.setattr(evalsweep, "_model_device", lambda m: torch.device("cpu"))
    monkeypatch.setattr(evalsweep, "_sets_per_call", lambda *a: 64)
    rng = np.random.default_rng(0)
    if kind == "fst":
        spec, n, tarr = rng.normal(size=(1025, 203)).astype(np.float32), 203, None
        farr = np.linspace(0, 22050, 1025) / 44100
    else:
        spec, n = rng.normal(size=(16, 10, 61)).astype(np.float32), 61
        farr, tarr = np.linspace(0, 0.5, 16), np.linspace(0, 0.1, 10)
    y = rng.integers(0, 10, size=n)
    files = (str(tmp_path / "randK.json"), str(tmp_path / "maxK.json"))
    out_r, out_m = evalsweep.subsample_sweep(_Net(), spec, y, farr, tarr, n_runs=4,
                                             json_files=files)
    list_K = _ref_list_K(1024 if kind == "fst" else 160).tolist()
    full = (n // 8) * 8
    ref_r, ref_m = _ref_two_dicts(list_K, 4, full, per_slot)
    # byte-for-byte what the reference's json.dump writes (int K keys -> strings, list_K ints)
    assert open(files[0]).read() == json.dumps(ref_r)
    assert open(files[1]).read() == json.dumps(ref_m)
    assert json.dumps(out_r) == json.dumps(ref_r) and json.dumps(out_m) == json.dumps(ref_m)
    assert all(type(k) is int for k in out_r["data"]) and out_r["list_K"] == list_K
    # every K: n_runs random runs with their own draw numbers and one max-K pass, all over the
    # first `full` sets
    assert [s[0] for s in seen] == list_K
    assert all(s[1] == (2 if kind == "fst" else 3) for s in seen)
    draws = [d for s in seen for (slot, d, p0, p1) in s[2] if slot < 4]
    assert len(set(draws)) == len(draws) == 4 * len(list_K)
    for s in seen:
        assert [(slot, p0, p1) for slot, _, p0, p1 in s[2]] == [(r, 0, full) for r in range(5)]


def test_importance_sweep_json_layout(tmp_path, monkeypatch):
    per_slot = lambda slot, K: (slot + 5 * K) % 16           # noqa: E731
    run, seen = _fake_pass(per_slot)
    monkeypatch.setattr(evalsweep, "_run_pieces", run)
    monkeypatch.setattr(evalsweep, "_model_device", lambda m: torch.device("cpu"))
    monkeypatch.setattr(evalsweep, "_sets_per_call", lambda *a: 64)
    rng = np.random.default_rng(1)
    spec = rng.normal(size=(12, 10, 45)).astype(np.float32)
    y = rng.integers(0, 10, size=45)
    farr, tarr = np.linspace(0, 0.5, 12), np.linspace(0, 0.1, 10)
    files = (str(tmp_path / "r.json"), str(tmp_path / "m.json"))
    out_r, out_m = evalsweep.importance_sweep(_Net(), spec, y, farr, tarr, list_winF=(64, 8),
                                              n_runs=3, json_files=files)
    list_K = _ref_list_K(120).tolist()
    ref_r, ref_m = _ref_two_dicts(list_K, 3, 40, per_slot, nest=[64, 8])
    assert open(files[0]).read() == json.dumps(ref_r)
    assert open(files[1]).read() == json.dumps(ref_m)
    assert list(out_r["data"].keys()) == [64, 8]
    draws = [d for s in seen for (slot, d, p0, p1) in s[2] if slot < 3]
    assert len(set(draws)) == len(draws) == 3 * 2 * len(list_K)


@pytest.mark.parametrize("Ntemp", [10, 4, 1])
def test_chunk_plan_equals_hsplit(Ntemp):
    """Code/pc_temp3d_eval.py:78-83 on ragged clips: hsplit at arange(0, T, Ntemp), pieces narrower
    than Ntemp dropped - the chunk plan names the same frames, in the same order."""
    frames = [23, 9, 30, 10, 1, 41, 19]
    offs = np.cumsum([0] + frames)
    ref = []
    for c, t in enumerate(frames):
        a = np.arange(offs[c], offs[c] + t)[None, :]          # frame ids of clip c, as columns
        for ss in np.hsplit(a, np.arange(0, a.shape[1], Ntemp)):
            if ss.shape[1] < Ntemp:
                continue
            ref.append((c, ss[0]))
    foff, ids, clip_of = evalsweep.chunk_plan(frames, Ntemp)
    assert len(foff) == len(frames) + 1 and all(o % Ntemp == 0 for o in foff)
    assert all(foff[c] + frames[c] <= foff[c + 1] for c in range(len(frames)))
    assert len(ids) == len(ref) == sum(t // Ntemp for t in frames)
    for (c, ref_frames), j, cj in zip(ref, ids, clip_of):
        assert cj == c
        rows = j * Ntemp + np.arange(Ntemp)                   # rows of the aligned layout
        np.testing.assert_array_equal(rows - foff[c] + offs[c], ref_frames)
    assert ids == sorted(ids) and len(set(ids)) == len(ids)


@pytest.mark.parametrize("N", [2048, 1536, 1280, 1075, 1024, 972, 921, 819, 716, 614, 512, 256,
                               102])
def test_temporal_axes_follow_reference(N):
    fs, Ntemp, hf = 22050.0, 10, 0.5
    farr, tarr = evalsweep.temporal_axes(fs, N, Ntemp, hf)
    Nfft = N                                                  # pc_temp3d_eval.py:67
    nbins = int(2 ** (np.ceil(np.log2(Nfft)))) // 2           # x[:-1, :] of 1 + n_fft/2 rows
    np.testing.assert_array_equal(farr, np.linspace(0, fs / 2, nbins) / fs)
    np.testing.assert_array_equal(tarr, np.linspace(0, ((hf * Nfft) / fs) * Ntemp, Ntemp))
    assert len(farr) == (1 << math.ceil(math.log2(N))) // 2
