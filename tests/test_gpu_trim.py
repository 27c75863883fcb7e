"""pca_hip.trim / trim_batch (pca_trim_bounds) on the device against the numpy restatement
tests/trim_ref.py, and the ``trim_dB`` argument of the four re-framing sweeps.

The bounds are compared EXACTLY: tests/test_trim_host.py checks that every waveform used here keeps
each frame at least 1e-6 dB away from the threshold, six orders of magnitude more than two fp64
summation orders differ by."""
import numpy as np
import pytest
import torch

import trim_ref as tr
from util import T

pytestmark = pytest.mark.gpu

FS = tr.SWEEP_FS


@pytest.fixture(scope="module")
def dev():
    return torch.device("cuda", 0)


@pytest.mark.parametrize("fl,hop", tr.CONFIGS)
def test_bounds_equal_restatement(fl, hop, dev):
    """Every case alone and the ragged batch of all of them, for both thresholds; the clips returned are
    views of the inputs equal to y[start:end]; a second run gives the same bounds."""
    import pca_hip
    cases = tr.gpu_cases(fl, hop)
    wd = [T(y, dev) for _, y in cases]
    for top_db in tr.TOP_DBS:
        ref = np.array([tr.trim_ref(y, top_db, fl, hop) for _, y in cases], dtype=np.int64)
        clips, b = pca_hip.trim_batch(wd, top_db, fl, hop)
        assert b.dtype == np.int64 and b.shape == (len(cases), 2)
        for (name, _), got, want in zip(cases, b.tolist(), ref.tolist()):
            print(f"{fl}/{hop} top_db={top_db} {name}: got {got} ref {want}")
        assert np.array_equal(b, ref), (fl, hop, top_db, b.tolist(), ref.tolist())
        _, b2 = pca_hip.trim_batch(wd, top_db, fl, hop)
        assert np.array_equal(b, b2)
        for (name, y), w, v, (s, e) in zip(cases, wd, clips, ref.tolist()):
            one, se = pca_hip.trim(w, top_db, fl, hop)
            assert se == (s, e), (name, se, (s, e))
            for view in (v, one):
                assert view.numel() == e - s
                assert view.untyped_storage().data_ptr() == w.untyped_storage().data_ptr()
                assert view.data_ptr() == w.data_ptr() + 4 * s
                assert np.array_equal(view.cpu().numpy(), y[s:e])


def test_batch_offsets_of_any_alignment(dev):
    """Clips whose offsets in the concatenated corpus are 0..3 samples off a 16-byte boundary give the
    bounds of the clip alone (the kernel's vector and scalar loads sum the same squares)."""
    import pca_hip
    base = [y for _, y in tr.gpu_cases(2048, 512) if y.size < 100000]
    lead = [tr.gpu_cases(2048, 512)[0][1][:4096 + k] for k in (1, 2, 3)]
    order = [lead[0], base[0], lead[1], base[3], base[4], lead[2], base[1], base[5]]
    wd = [T(np.ascontiguousarray(y), dev) for y in order]
    _, b = pca_hip.trim_batch(wd, 60)
    ref = np.array([tr.trim_ref(y, 60) for y in order], dtype=np.int64)
    for y in lead:
        assert tr.decision_margin(y, 60) >= 1e-6
    assert np.array_equal(b, ref), (b.tolist(), ref.tolist())
    # a strided view of the device tensor is trimmed as its samples, the result a view of it
    w = T(np.repeat(order[1], 2), dev)[::2]
    v, se = pca_hip.trim(w, 60)
    assert se == tuple(ref[1].tolist())
    assert v.untyped_storage().data_ptr() == w.untyped_storage().data_ptr()
    assert np.array_equal(v.cpu().numpy(), order[1][se[0]:se[1]])


def test_kept_interval_never_shrinks_as_top_db_grows(dev):
    import pca_hip
    for fl, hop in tr.CONFIGS:
        wd = [T(y, dev) for _, y in tr.gpu_cases(fl, hop)]
        prev = None
        for top_db in (0.5, 5, 10, 20, 30, 40, 60, 80, 120):
            _, b = pca_hip.trim_batch(wd, top_db, fl, hop)
            assert np.all(b[:, 0] <= b[:, 1])
            if prev is not None:
                assert np.all(b[:, 0] <= prev[:, 0]) and np.all(b[:, 1] >= prev[:, 1]), (fl, hop, top_db)
            prev = b
        assert np.array_equal(prev, np.array([[0, w.numel()] for w in wd]))   # 120 dB: nothing goes


def test_formula_corner_cases(dev):
    """top_db = 0: no frame is strictly above its own maximum -> (0, 0), an empty view; bad arguments
    raise."""
    import pca_hip
    y = tr.synth(4, 5, 25000)
    w = T(y, dev)
    v, se = pca_hip.trim(w, 0)
    assert se == (0, 0) and v.numel() == 0
    assert tr.trim_ref(y, 0) == (0, 0)
    with pytest.raises(pca_hip.PcaHipError):
        pca_hip.trim(w[:1024], 60)                        # L must exceed frame_length / 2
    with pytest.raises(pca_hip.PcaHipError):
        pca_hip.trim(w, 60, frame_length=2047)
    with pytest.raises(pca_hip.PcaHipError):
        pca_hip.trim(w, float("nan"))
    with pytest.raises(pca_hip.PcaHipError):
        pca_hip.trim(w.double(), 60)


# ---- the sweeps --------------------------------------------------------------------------------------
def _st(din, dev, seed=2):
    import models
    torch.manual_seed(seed)
    return models.ST(dim_input=din, dim_output=10, num_inds=64, dim_hidden=64, num_heads=8).to(dev)


def _sliced(clips, dev):
    """The host route: y[start:end] with the restatement's bounds, uploaded as clips of their own."""
    out = []
    for y in clips:
        s, e = tr.trim_ref(y, 60)
        out.append(T(np.ascontiguousarray(y[s:e]), dev))
    return out


def test_reframe_sweep_trim_equals_host_sliced_clips(dev):
    import evalsweep
    clips, labels = tr.sweep_clips()
    wd = [T(y, dev) for y in clips]
    net = _st(2, dev)
    list_N = [1024, 1000, 200]
    want = evalsweep.reframe_sweep(net, _sliced(clips, dev), labels, FS, list_N)
    got = evalsweep.reframe_sweep(net, wd, labels, FS, list_N, trim_dB=60)
    assert got == want
    plain = evalsweep.reframe_sweep(net, wd, labels, FS, list_N)
    assert evalsweep.reframe_sweep(net, wd, labels, FS, list_N, trim_dB=None) == plain
    # the sampling-rate axis: trimmed first, then resampled (Code/pceval.py:74)
    Fs = [FS, 16000.0]
    want = evalsweep.reframe_sweep(net, _sliced(clips, dev), labels, FS, list_N[:2], list_Fs=Fs)
    got = evalsweep.reframe_sweep(net, wd, labels, FS, list_N[:2], list_Fs=Fs,
                                  trim_dB=evalsweep.trim_dB_of({"trim_dB": 60}))
    assert got == want


def test_reframe_sweep_temporal_trim_equals_host_sliced_clips(dev):
    import evalsweep
    clips, labels = tr.sweep_clips()
    wd = [T(y, dev) for y in clips]
    net = _st(3, dev)
    list_N = [1024, 200]
    want = evalsweep.reframe_sweep_temporal(net, _sliced(clips, dev), labels, FS, list_N)
    got = evalsweep.reframe_sweep_temporal(net, wd, labels, FS, list_N, trim_dB=60)
    assert got == want
    plain = evalsweep.reframe_sweep_temporal(net, wd, labels, FS, list_N)
    assert evalsweep.reframe_sweep_temporal(net, wd, labels, FS, list_N, trim_dB=None) == plain


def test_baseline_sweeps_trim_equals_host_sliced_clips(dev):
    import evalsweep
    import models
    clips, labels = tr.sweep_clips()
    wd = [T(y, dev) for y in clips]
    torch.manual_seed(3)
    fb = models.baseline_ff([1025, 513, 256], 10).to(dev).eval()
    cnn = models.CNN_classifier(10, 512, [512, 256, 100], 10).to(dev).eval()
    for model, sweep, list_N in ((fb, evalsweep.baseline_reframe_sweep, [2048, 1024]),
                                 (cnn, evalsweep.baseline_reframe_sweep_temporal, [1024, 512])):
        want = sweep(model, _sliced(clips, dev), labels, FS, list_N)
        got = sweep(model, wd, labels, FS, list_N, trim_dB=60)
        assert got == want
        plain = sweep(model, wd, labels, FS, list_N)
        assert sweep(model, wd, labels, FS, list_N, trim_dB=None) == plain


def test_clip_trimmed_below_the_stft_minimum_raises(dev):
    """A clip that is digital silence but for 450 samples inside one hop (10240, 10752) keeps the four
    frames 19..22 that see them: 4 * 512 = 2048 samples, not more than the n_fft / 2 = 2048 of N = 4096;
    the error names the clip and its bounds."""
    import evalsweep
    clips, labels = tr.sweep_clips()
    short = np.zeros(30000, np.float32)
    short[10250:10700] = tr.synth(9, 2, 450, FS)
    s, e = tr.trim_ref(short, 60)
    assert (s, e) == (19 * 512, 23 * 512) and tr.decision_margin(short, 60) >= 1e-6
    wd = [T(y, dev) for y in clips[:2] + [short] + clips[2:]]
    labels = labels[:2] + [7] + labels[2:]
    net = _st(2, dev)
    with pytest.raises(ValueError, match=rf"clip 2: .*\[{s}, {e}\)"):
        evalsweep.reframe_sweep(net, wd, labels, FS, [4096], trim_dB=60)
    with pytest.raises(ValueError, match=r"clip 2"):
        evalsweep.reframe_sweep_temporal(_st(3, dev), wd, labels, FS, [4096], trim_dB=60)
    # fine where the window is short enough
    evalsweep.reframe_sweep(net, wd, labels, FS, [1024], trim_dB=60)
