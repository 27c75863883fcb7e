"""pca_clip_aggregate on the device against the float64 restatement tests/clip_ref.py, and
evalsweep.clip_accuracy end to end.

votes are compared exactly (a frame's argmax compares the same fp32 values on both sides);
mean_logprob to the fp32 forward bar, 1e-4 of max(1, max|ref|); predictions for every clip whose
float64 top-2 margin in mean log-prob is at least 1e-3 and whose vote is not tied - and the inputs are
such that this is every clip (asserted here, and without a GPU in tests/test_clip_host.py)."""
import json

import numpy as np
import pytest
import torch

import clip_ref as cr
import trim_ref as tr
from util import T

pytestmark = pytest.mark.gpu

TOL = 1e-4
FS = tr.SWEEP_FS


@pytest.fixture(scope="module")
def dev():
    return torch.device("cuda", 0)


def _run(logits, off, dev, labels=None, counts=None, slot=0):
    import pca_hip
    lg = logits if torch.is_tensor(logits) else T(logits, dev)
    of = off if torch.is_tensor(off) else T(np.asarray(off, dtype=np.int64), dev)
    lab = None if labels is None else T(np.asarray(labels, dtype=np.int64), dev)
    pred, mean, votes = pca_hip.clip_aggregate(lg, of, lab, counts, slot)
    return pred.cpu().numpy(), mean.cpu().numpy(), votes.cpu().numpy()


def _check_mean(mean, ref_mean, what):
    """1e-4 of max(1, max|ref|) over the finite entries; -inf and NaN must sit where the reference's do."""
    fin = np.isfinite(ref_mean)
    assert np.array_equal(np.isnan(mean), np.isnan(ref_mean)), what
    assert np.array_equal(np.isneginf(mean), np.isneginf(ref_mean)), what
    assert np.array_equal(np.isfinite(mean), fin), what
    if not fin.any():
        return 0.0
    scale = max(1.0, float(np.abs(ref_mean[fin]).max()))
    err = float(np.abs(mean[fin].astype(np.float64) - ref_mean[fin]).max())
    print(f"{what}: max|mean - ref| = {err:.3e} (bar {TOL * scale:.3e})")
    assert err <= TOL * scale, (what, err, scale)
    return err


@pytest.mark.parametrize("C", cr.CLASSES)
def test_clip_aggregate_matches_float64_reference(C, dev):
    logits, off, labels = cr.gpu_case(C)
    ref = cr.clip_ref(logits, off, labels)
    assert not cr.left_out(ref).any()                 # no clip is excused from the comparison
    counts = torch.zeros(6, dtype=torch.int64, device=dev)
    pred, mean, votes = _run(logits, off, dev, labels, counts, 1)
    assert votes.dtype == np.int32 and pred.dtype == np.int64 and mean.dtype == np.float32
    assert np.array_equal(votes, ref["votes"])
    assert np.array_equal(votes.sum(1), np.diff(off))             # every frame voted once
    _check_mean(mean, ref["mean"], f"C={C}")
    assert np.array_equal(pred, ref["pred"])
    assert counts.tolist() == [0, 0, ref["counts"][0], ref["counts"][1], 0, 0]


def test_crafted_ties(dev):
    logits, off, want_pred, want_votes = cr.crafted_case()
    pred, mean, votes = _run(logits, off, dev)
    assert pred.tolist() == want_pred.tolist()
    for c, v in enumerate(want_votes):
        want = np.zeros(logits.shape[1], dtype=np.int64)
        for k, n in v.items():
            want[k] = n
        assert votes[c].tolist() == want.tolist(), c
    assert mean[0, 3] == mean[0, 7] and mean[1, 4] == mean[1, 7]  # exact ties, not near ones
    assert (mean[5] == 0).all() and (votes[5] == 0).all()          # the clip without rows
    _check_mean(mean, cr.clip_ref(logits, off)["mean"], "crafted")
    # the same clips in the middle of a longer call, tallied
    labels = want_pred[:, 0].copy()
    labels[3] = 0                                  # clip 3: right for the mean rule only
    counts = torch.zeros(2, dtype=torch.int64, device=dev)
    pred2, _, _ = _run(logits, off, dev, labels, counts)
    assert pred2.tolist() == want_pred.tolist()
    n = len(want_votes) - 1                                         # the empty clip is not tallied
    assert counts.tolist() == [n - 1, n - 1]       # vote misses clip 3; mean misses clip 4 (0, not 4)


def test_more_classes_than_one_pass_holds(dev):
    """C = 4100: the classes are aggregated in three passes of at most 2048."""
    rng = np.random.Generator(np.random.PCG64(21))
    C, lens = 4100, [5, 0, 1, 9, 4]
    off = np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)
    own = [4099, 0, 2048, 17, 2047]
    logits = rng.normal(0, 1, size=(int(off[-1]), C)).astype(np.float32)
    for c, k in enumerate(own):
        logits[off[c]:off[c + 1], k] += np.float32(6.0)
    ref = cr.clip_ref(logits, off, own)
    assert not cr.left_out(ref).any()
    counts = torch.zeros(2, dtype=torch.int64, device=dev)
    pred, mean, votes = _run(logits, off, dev, own, counts)
    assert np.array_equal(votes, ref["votes"]) and np.array_equal(pred, ref["pred"])
    _check_mean(mean, ref["mean"], "C=4100")
    assert counts.tolist() == ref["counts"] == [4, 4]


def test_offsets_are_clamped_to_the_logits(dev):
    """Rows past n_sets are not read: a last offset beyond the buffer aggregates what is there."""
    logits, off, _ = cr.gpu_case(10)
    n = int(off[3])
    bad = off[:4].copy()
    bad[3] = n + 1000
    pred, mean, votes = _run(np.ascontiguousarray(logits[:n]), bad, dev)
    ref = cr.clip_ref(logits[:n], off[:4])
    assert np.array_equal(votes, ref["votes"]) and np.array_equal(pred, ref["pred"])


def test_reproducible_captured_and_accumulating(dev):
    import pca_hip
    logits, off, labels = cr.gpu_case(50)
    ref = cr.clip_ref(logits, off, labels)
    lg, of, lab = T(logits, dev), T(off, dev), T(labels, dev)
    a = pca_hip.clip_aggregate(lg, of)
    b = pca_hip.clip_aggregate(lg, of)
    for x, y in zip(a, b):
        assert torch.equal(x.view(torch.int32) if x.dtype == torch.float32 else x,
                           y.view(torch.int32) if y.dtype == torch.float32 else y)
    # counts accumulate over calls and slots; without labels they are not touched
    counts = torch.zeros(6, dtype=torch.int64, device=dev)
    for _ in range(3):
        pca_hip.clip_aggregate(lg, of, lab, counts, 0)
    pca_hip.clip_aggregate(lg, of, lab, counts, 2)
    pca_hip.clip_aggregate(lg, of)
    v, m = ref["counts"]
    assert counts.tolist() == [3 * v, 3 * m, 0, 0, v, m]
    with pytest.raises(AssertionError):
        pca_hip.clip_aggregate(lg, of, lab, None)
    # captured into a graph: the replay gives the eager call's bits and adds the same counts
    cg = torch.zeros(2, dtype=torch.int64, device=dev)
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        pca_hip.clip_aggregate(lg, of, lab, cg, 0)           # warm-up outside the capture
    torch.cuda.current_stream().wait_stream(s)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        got = pca_hip.clip_aggregate(lg, of, lab, cg, 0)
    cg.zero_()
    for t in got:
        t.zero_()
    for _ in range(4):
        graph.replay()
    torch.cuda.synchronize()
    assert cg.tolist() == [4 * v, 4 * m]
    assert torch.equal(got[0], a[0]) and torch.equal(got[2], a[2])
    assert torch.equal(got[1].view(torch.int32), a[1].view(torch.int32))


# ---- end to end: evalsweep.clip_accuracy -----------------------------------------------------------------
class HostReads:
    """Counts the device-to-host reads made through torch.Tensor while it is active."""
    NAMES = ("tolist", "item", "cpu", "numpy", "__int__", "__float__", "__bool__", "__index__")

    def __enter__(self):
        self.n, self.saved = 0, {}

        def patch(name, make):
            self.saved[name] = torch.Tensor.__dict__.get(name)      # None: inherited
            setattr(torch.Tensor, name, make(getattr(torch.Tensor, name)))

        def reader(orig):
            def wrapped(t, *a, **k):
                self.n += bool(t.is_cuda)
                return orig(t, *a, **k)
            return wrapped

        def mover(orig):
            def to(t, *a, **k):
                r = orig(t, *a, **k)
                self.n += bool(t.is_cuda and not r.is_cuda)
                return r
            return to

        for name in self.NAMES:
            patch(name, reader)
        patch("to", mover)
        return self

    def __exit__(self, *exc):
        for name, own in self.saved.items():
            if own is None:
                delattr(torch.Tensor, name)
            else:
                setattr(torch.Tensor, name, own)


def _st(din, dev, seed=2):
    import models
    torch.manual_seed(seed)
    return models.ST(dim_input=din, dim_output=10, num_inds=64, dim_hidden=64, num_heads=8).to(dev)


def _trim_short():
    """Digital silence but for 450 samples inside one hop: librosa's trim keeps 4 * 512 = 2048 samples
    (tests/test_gpu_trim.py), which is no frame for n_fft = 4096."""
    short = np.zeros(30000, np.float32)
    short[10250:10700] = tr.synth(9, 2, 450, FS)
    assert tr.trim_ref(short, 60) == (19 * 512, 23 * 512)
    return short


E2E = {
    # name: (N, Ntemp, trim_dB, the extra clip that yields no set, sets per engine call)
    "frames": (1024, None, None, np.zeros(500, np.float32), 64),
    "frames_trim": (4096, None, 60, _trim_short, 16),
    "chunks": (1024, 10, None, tr.synth(5, 1, 3000, FS), 8),       # 6 frames: no whole chunk
    "chunks_trim": (1024, 10, 60, None, 8),
}


@pytest.mark.parametrize("case", list(E2E))
def test_clip_accuracy_equals_reference_on_engine_logits(case, dev, tmp_path):
    import evalsweep
    import pca_hip
    from pca_hip.trainer import STEngine
    N, Ntemp, trim_dB, extra, cap = E2E[case]
    clips, _ = tr.sweep_clips()
    if extra is not None:
        clips = clips[:2] + [extra() if callable(extra) else extra] + clips[2:]
    wd = [T(y, dev) for y in clips]
    net = _st(2 if Ntemp is None else 3, dev)
    n_fft, hop = evalsweep._pow2_fft([N]), N // 2

    # the existing route: host-sliced clips -> the existing datasets -> engine forward of the same sets
    host = [y[slice(*tr.trim_ref(y, trim_dB))] if trim_dB is not None else y for y in clips]
    sets_of = [0 if y.size <= n_fft // 2 else
               (1 + y.size // hop) // (1 if Ntemp is None else Ntemp) for y in host]
    keep = [c for c, y in enumerate(host) if y.size > n_fft // 2]
    kept = [T(np.ascontiguousarray(host[c]), dev) for c in keep]
    if Ntemp is None:
        ds = evalsweep.framewise_dataset(kept, [0] * len(kept), FS, N)
        ids = torch.arange(len(ds), device=dev)
    else:
        ds, ids = evalsweep.temporal_dataset(kept, [0] * len(kept), FS, N, Ntemp)
    n_sets = sum(sets_of)
    assert ids.numel() == n_sets and n_sets > 2 * cap          # several engine calls
    assert (min(sets_of) == 0) == (extra is not None)
    parts, engines, done = [], {}, 0
    while done < n_sets:
        b = min(cap, n_sets - done)
        if b not in engines:
            engines[b] = STEngine(net, b, ds.num_points, training=False)
        X = ds.batch(ids[done:done + b])[0]
        parts.append(engines[b].forward(X).clone())
        done += b
    logits = torch.cat(parts)
    off = np.concatenate([[0], np.cumsum(sets_of)]).astype(np.int64)
    ref = cr.clip_ref(logits.cpu().numpy(), off)
    assert not cr.left_out(ref).any()                 # the model's clips are all decided clearly
    # labels the two rules get partly right, whatever the untrained model predicts
    labels = [int(ref["pred"][c, c % 2]) if c % 3 else (int(ref["pred"][c, 0]) + 1) % 10
              for c in range(len(clips))]
    ref = cr.clip_ref(logits.cpu().numpy(), off, labels)
    set_lab = np.repeat(np.asarray(labels, dtype=np.int64), sets_of)
    tally = torch.zeros(1, dtype=torch.int64, device=dev)
    pca_hip.eval_tally(logits, T(set_lab, dev), tally, 0)
    n_live = sum(1 for n in sets_of if n)

    jf = str(tmp_path / "clip.json")
    with HostReads() as reads:
        out = evalsweep.clip_accuracy(net, wd, labels, FS, N, Ntemp=Ntemp, trim_dB=trim_dB,
                                      batch_size=cap, json_file=jf)
    # one read of the counters; the trim's read of its bounds is the only other one
    assert reads.n == (1 if trim_dB is None else 2), reads.n
    print(case, out, "host reads", reads.n)
    assert out["n_sets"] == n_sets and out["n_clips"] == len(clips)
    assert out["n_empty"] == len(clips) - n_live
    assert out["frame"] == int(tally.item()) / n_sets
    assert out["frame"] == float((ref["frame_argmax"] == set_lab).sum()) / n_sets
    assert out["clip_vote"] == ref["counts"][0] / n_live
    assert out["clip_mean"] == ref["counts"][1] / n_live
    assert 0 < ref["counts"][0] < n_live
    assert json.load(open(jf)) == out
    # engine calls of a few sets at a time: as many host reads, however many batches
    with HostReads() as reads2:
        out2 = evalsweep.clip_accuracy(net, wd, labels, FS, N, Ntemp=Ntemp, trim_dB=trim_dB,
                                       batch_size=3)
    assert reads2.n == reads.n and out2["n_sets"] == n_sets
