"""Host-side pieces of the batch-scale sweeps (evalsweep.subsample_sweep / importance_sweep /
reframe_sweep_temporal): the K grid, the JSON the reference writes, the chunk plan and the 3-D axes,
the call packing of the engine pass and the (Fs, N) loop of the re-framing sweeps.
No GPU: the engine pass is replaced by a stand-in that fills the counters, or runs on a stand-in
engine."""
import json
import math
import types

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


def _rows(view):
    """(the buffer a leading-dimension slice views, its first row, its end row)."""
    base = view if view._base is None else view._base
    r0 = (view.storage_offset() - base.storage_offset()) // base.stride(0)
    return base, r0, r0 + view.shape[0]


@pytest.mark.parametrize("cap, pieces, sizes", [
    (5, [(0, 1, 0, 7), (1, 2, 0, 7), (2, 0, 0, 7)], [5, 5, 5, 5, 1]),
    (8, [(0, 0, 0, 3)], [3])])
def test_run_pieces_call_packing(cap, pieces, sizes, monkeypatch):
    """_run_pieces cuts the pieces into engine calls of `cap` sets (the last one shorter), builds one
    engine per call size, hands `select` every position once, and the views it passes to `select`
    and to the tally tile each call's buffers."""
    npts, din = 6, 2
    built, events = [], []

    class Engine:
        def __init__(self, model, B, n, mode, training=True):
            assert training is False
            built.append((B, n))
            self.cfg, self.B = types.SimpleNamespace(k=1), B

        def forward(self, X):
            assert X.shape == (self.B, npts, din) and X.dtype == torch.float32
            events.append(("forward", X, torch.zeros(self.B, 4)))
            return events[-1][2]

    def select(slot, draw, pos, out, labels_out):
        assert pos.dtype == torch.int64 and labels_out.dtype == torch.int64
        events.append(("select", slot, draw, pos.tolist(), out, labels_out))

    monkeypatch.setattr(evalsweep, "STEngine", Engine)
    monkeypatch.setattr(evalsweep.pca_hip, "eval_tally",
                        lambda logits, lab, counts, slot: events.append(("tally", slot, logits, lab)))
    evalsweep._run_pieces(_Net(), npts, din, 0, cap, pieces, select, torch.zeros(3, dtype=torch.int64))
    forwards = [e for e in events if e[0] == "forward"]
    assert [e[1].shape[0] for e in forwards] == sizes
    assert built == [(b, npts) for b in dict.fromkeys(sizes)]      # once per size, in order of use
    for slot, draw, p0, p1 in pieces:
        mine = [e for e in events if e[0] == "select" and e[1] == slot]
        assert all(e[2] == draw for e in mine)
        assert [p for e in mine for p in e[3]] == list(range(p0, p1))
    # per call: selects, one forward, tallies; the views tile [0, B) of X, labels and logits
    i = 0
    for b in sizes:
        j = i
        while events[j][0] == "select":
            j += 1
        kind, X, logits = events[j]
        assert kind == "forward" and j > i
        sel, tal = events[i:j], events[j + 1:j + 1 + (j - i)]
        assert [e[0] for e in tal] == ["tally"] * (j - i)
        assert [e[1] for e in tal] == [e[1] for e in sel]            # same slots, same order
        end, lab_bufs = 0, []
        for s_, t_ in zip(sel, tal):
            n = len(s_[3])
            spans = [_rows(v) for v in (s_[4], s_[5], t_[2], t_[3])]
            assert all((r0, r1) == (end, end + n) for _, r0, r1 in spans)
            assert spans[0][0] is X and spans[2][0] is logits and spans[1][0] is spans[3][0]
            lab_bufs.append(spans[1][0])
            end += n
        assert end == b and tuple(lab_bufs[0].shape) == (b,)
        assert all(buf is lab_bufs[0] for buf in lab_bufs)
        i = j + 1 + (j - i)
    assert i == len(events)


REFRAME_SWEEPS = ["reframe_sweep", "reframe_sweep_temporal", "baseline_reframe_sweep",
                  "baseline_reframe_sweep_temporal"]


@pytest.mark.parametrize("name", REFRAME_SWEEPS)
def test_reframe_sweeps_trim_once_resample_per_rate(name, tmp_path, monkeypatch):
    """The (Fs, N) loop of the four re-framing sweeps (Code/pceval.py:61-104 and its counterparts):
    one trim, before any resampling; one resampling per clip and rate; the reference's dictionary,
    rates as keys in the given order; NaN where an N leaves less than one batch."""
    from test_baselines_host import _FakeEngine
    fs, list_N, short_N = 44100, [1024, 600, 100], 600
    list_Fs = [fs, fs / 2]
    clips = [torch.zeros(8192 + c) for c in range(3)]
    baseline, temporal = name.startswith("baseline"), name.endswith("temporal")
    batch = (2 if temporal else 1) if baseline else 8
    events, cur = [], {}
    n_of = lambda N: batch - 1 if N == short_N else 16 + N % 5                # noqa: E731
    hits = lambda L, N: (L // 1024 + N) % 7 + 1                              # noqa: E731

    def trim_batch(cs, top_db):
        events.append(("trim", [int(x.numel()) for x in cs], top_db))
        return cs, torch.tensor([[0, int(x.numel())] for x in cs])

    def resample(x, fs_in, fs_out, scale=False):
        assert fs_in == fs and scale is True
        events.append(("resample", int(x.numel()), fs_out))
        return x[:int(x.numel() * fs_out / fs_in)]

    class DS:
        def __init__(self, n, npts):
            self.n, self.num_points = n, npts

        def __len__(self):
            return self.n

    def build(cs, N, rate=None):
        assert rate is None or rate == fs * cs[0].numel() // 8192        # the clips of that rate
        cur["hits"] = hits(cs[0].numel(), N)
        return n_of(N)

    def framewise(cs, labels, rate, N, hf=0.5):
        return DS(build(cs, N, rate), 1 + N)

    def temporal_ds(cs, labels, rate, N, Ntemp=10, hf=0.5):
        n = build(cs, N, rate)
        return DS(n + 3, N), torch.arange(n)

    def frames(cs, labels, N, n_fft, hf=0.5):
        n = build(cs, N)
        return torch.zeros(1025, n), torch.zeros(n, dtype=torch.int64)

    def chunks(cs, labels, N, n_fft, Ntemp=10, hf=0.5):
        n = build(cs, N)
        return torch.zeros(512, Ntemp, n + 3), torch.zeros(n + 3, dtype=torch.int64), torch.arange(n)

    def run_pieces(model, npts, din, mode, cap, pieces, select, counts):
        counts[0] += cur["hits"]

    def baseline_run(eng, x, lab, ids, pieces, counts, K=None, sel_of_slot=None, seed=0, cap=None):
        counts[0] += cur["hits"]

    monkeypatch.setattr(evalsweep.pca_hip, "trim_batch", trim_batch)
    monkeypatch.setattr(evalsweep.pca_hip, "resample", resample)
    for attr, fake in (("framewise_dataset", framewise), ("temporal_dataset", temporal_ds),
                       ("baseline_frames", frames), ("baseline_chunks", chunks),
                       ("_run_pieces", run_pieces), ("_baseline_run", baseline_run),
                       ("_model_device", lambda m: torch.device("cpu")),
                       ("_sets_per_call", lambda *a: 64)):
        monkeypatch.setattr(evalsweep, attr, fake)
    if baseline:
        model = _FakeEngine(temporal)
        model.layer_dims, model.Nf, model.Nt = [1025, 513, 256], 512, 10
    else:
        model = _Net()
    path = str(tmp_path / "expt1.json")
    out = getattr(evalsweep, name)(model, clips, [0, 1, 2], fs, list_N, list_Fs=list_Fs,
                                   trim_dB=60, json_file=path)
    assert events[0] == ("trim", [8192, 8193, 8194], 60)
    assert [e[0] for e in events].count("trim") == 1
    assert events[1:] == [("resample", 8192 + c, F) for F in list_Fs for c in range(3)]
    full = (n_of(1024) // batch) * batch, (n_of(100) // batch) * batch
    ref = {"data": {F: [hits(int(8192 * F / fs), 1024) / full[0], float("nan"),
                        hits(int(8192 * F / fs), 100) / full[1]] for F in list_Fs},
           "list_Fs": list_Fs, "list_N": list_N}
    assert open(path).read() == json.dumps(ref) and json.dumps(out) == json.dumps(ref)
    assert list(out["data"].keys()) == list_Fs and math.isnan(out["data"][fs / 2][1])
