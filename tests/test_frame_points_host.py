"""pca_frame_points without a GPU: the numpy restatement of one frame (tests/frame_ref.py) against the
STFT oracle on the regular grid, the entry point's host checks, and the set layout of the waveform
datasets."""
import ctypes

import numpy as np
import pytest

import pca_hip
from pca_hip import _lib

from frame_ref import frame_ref
from oracle import st_oracle as orc


@pytest.mark.parametrize("n_fft,win", [(64, 64), (256, 200), (1024, 1024)])
def test_frame_ref_on_the_grid_is_the_stft_oracle(n_fft, win):
    wave = orc.synth_clip(3, 7, seconds=0.1)
    hop = n_fft // 2
    want = orc.stft_logmag(wave, n_fft, win, hop)                       # [F, T]
    F, T = want.shape
    assert T == 1 + len(wave) // hop and T >= 5
    for t in range(T):                                                  # first and last: reflected padding
        got = frame_ref(wave, t * hop, n_fft, win, 1.0, n_fft, F)
        assert np.array_equal(got, want[:, t]), t
    # fewer bins are a prefix (the dropped Nyquist bin)
    assert np.array_equal(frame_ref(wave, hop, n_fft, win, 1.0, n_fft, F - 1), want[:-1, 1])


def _call(L, **over):
    """pca_frame_points with valid host arguments and stand-in device addresses (a refused call never
    reads them), ``over`` replacing some."""
    P = 0x1000
    aug = dict(jitter=0, gain_db=0.0, win_lengths=P, n_win=1, norm_mode=0, seed=0, draw=0,
               draw_dev=None)
    a = dict(waves=P, wave_off=P, set_off=P, n_clips=2, max_len=9000, min_len=3000, clip_labels=P,
             idx=P, B=4, n_fft=256, hop=128, n_bins=129, Nt=1, farr=P, tarr=None, out=P,
             labels_out=P, meta_out=None)
    for k, v in over.items():
        (aug if k in aug else a)[k] = v
    s = _lib.PcaFrameAug(aug["jitter"], aug["gain_db"], aug["win_lengths"], aug["n_win"],
                         aug["norm_mode"], aug["seed"], aug["draw"], aug["draw_dev"])
    return L.pca_frame_points(a["waves"], a["wave_off"], a["set_off"], a["n_clips"], a["max_len"],
                              a["min_len"], a["clip_labels"], a["idx"], a["B"], a["n_fft"], a["hop"],
                              a["n_bins"], a["Nt"], a["farr"], a["tarr"], ctypes.byref(s), a["out"],
                              a["labels_out"], a["meta_out"], None)


@pytest.mark.parametrize("over,word", [
    (dict(waves=None), b"null pointer"),
    (dict(idx=None), b"null pointer"),
    (dict(win_lengths=None), b"win_lengths"),
    (dict(labels_out=None), b"go together"),
    (dict(n_fft=384), b"power of two"),
    (dict(n_fft=8192, n_bins=129), b"power of two"),
    (dict(min_len=128), b"longer than n_fft/2"),
    (dict(jitter=-1), b"jitter=-1"),
    (dict(gain_db=float("nan")), b"gain_db"),
    (dict(gain_db=float("inf")), b"gain_db"),
    (dict(gain_db=-1.0), b"gain_db"),
    (dict(n_win=0), b"n_win=0"),
    (dict(norm_mode=2), b"norm_mode=2"),
    (dict(Nt=128, tarr=0x1000), b"points per set"),                     # 128 * 129 = 16512 > 16384
    (dict(B=65536), b"B=65536"),
    (dict(hop=0), b"hop=0"),
    (dict(n_bins=130), b"n_bins=130"),
], ids=lambda v: None if isinstance(v, bytes) else "-".join(f"{k}={x}" for k, x in v.items()))
def test_entry_point_refuses_without_gpu(over, word):
    L = pca_hip.lib()
    assert _call(L, **over) == -1
    msg = L.pca_last_error()
    assert msg.startswith(b"frame_points:") and word in msg, msg


def test_set_offsets_as_the_datasets_build_them():
    import dataset
    lens = [2205, 4851, 16170, 22050]
    hop, ntemp = 32, 10
    frames = [1 + n // hop for n in lens]
    assert frames == [69, 152, 506, 690]
    assert dataset.wave_set_offsets(lens, hop) == [0, 69, 221, 727, 1417]
    assert dataset.wave_set_offsets(lens, hop, ntemp) == [0, 6, 21, 71, 140]
    clips = [np.zeros(n, dtype=np.float32) for n in lens]
    y = [3, 1, 4, 1]
    d2 = dataset.ESC_wave_pc(clips, y, 44100, 64)                       # hop defaults to n_fft / 2
    assert d2.hop == hop and d2.set_off == [0, 69, 221, 727, 1417] and len(d2) == 1417
    assert d2.num_points == 33 and not d2.stochastic and d2.batch_seq is None
    assert dataset.ESC_wave_pc(clips, y, 44100, 64, drop_nyquist=True).num_points == 32
    d3 = dataset.ESC_wave_pc_temp(clips, y, 44100, 64, ntemp)
    assert d3.set_off == [0, 6, 21, 71, 140] and len(d3) == 140 and d3.num_points == 320
    # chunks are whole: T // Ntemp per clip, the tail dropped (Code/settransformertemp.py:54-58)
    for t, a, b in zip(frames, d3.set_off, d3.set_off[1:]):
        assert b - a == t // ntemp == orc.chunk_frames(np.zeros((2, t)), ntemp).shape[2]
    assert np.array_equal(d3.labels, np.repeat(y, [6, 15, 50, 69]))
    assert np.array_equal(d3.farr, np.linspace(0, 22050, 32) / 44100)
    assert np.array_equal(d3.tarr, np.linspace(0, (32 / 44100) * ntemp, ntemp))
    # stochastic iff an augmentation is on; plain() turns all of them off and keeps the nominal window
    for kw in (dict(jitter=1), dict(gain_db=0.5), dict(win_lengths=(48, 64))):
        aug = dataset.ESC_wave_pc(clips, y, 44100, 64, **kw)
        assert aug.stochastic and not aug.plain().stochastic
    assert dataset.ESC_wave_pc(clips, y, 44100, 64, win_lengths=(48, 64)).plain().win_lengths == (48,)
    assert not dataset.ESC_wave_pc(clips, y, 44100, 64, win_lengths=(48,)).stochastic
    with pytest.raises(ValueError):
        dataset.ESC_wave_pc(clips, y, 44100, 64, win_lengths=(65,))
    with pytest.raises(ValueError):
        dataset.ESC_wave_pc(clips, y, 44100, 64, norm="hop")
