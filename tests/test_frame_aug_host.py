"""pca_frame_points_ex / pca_clip_rms without a GPU: the C ABI, the entry point's host checks, the numpy
restatement of one augmented frame (tests/frame_aug_ref.py) and the datasets' new options."""
import ctypes
import os
import re

import numpy as np
import pytest

import pca_hip
from pca_hip import _lib

from frame_aug_ref import aug_samples, frame_aug_ref, frame_of_samples, speed_centre, speed_clip
from frame_ref import frame_ref
from oracle import resample_oracle
from oracle import st_oracle as orc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ---- the C ABI ---------------------------------------------------------------------------------------
def test_header_declares_and_library_exports_the_entry_points():
    txt = open(os.path.join(ROOT, "include", "pca_hip.h")).read()
    txt = re.sub(r"/\*.*?\*/", "", txt, flags=re.S)
    handle = ctypes.CDLL(_lib.LIB_PATH)
    for name in ("pca_frame_points_ex", "pca_clip_rms", "pca_frame_points"):
        assert re.search(r"\b%s\s*\(" % name, txt), f"{name} not declared in pca_hip.h"
        assert hasattr(handle, name), f"{name} not exported"
        assert name in _lib.SIGNATURES
        assert getattr(pca_hip.lib(), name).argtypes == _lib.SIGNATURES[name][1]
    assert "PcaFrameAugEx" in txt and "typedef struct PcaFrameAug {" in txt
    assert pca_hip.lib().pca_abi_version() == 2
    # the struct as the header lays it out: PcaFrameAug's seven fields first, at the same offsets
    for name, _ in _lib.PcaFrameAug._fields_:
        assert getattr(_lib.PcaFrameAugEx, name).offset == getattr(_lib.PcaFrameAug, name).offset
    assert _lib.PcaFrameAugEx.ratios.offset == ctypes.sizeof(_lib.PcaFrameAug) + 16
    assert _lib.PcaFrameAugEx.ratios.size == 8 * 8
    assert ctypes.sizeof(_lib.PcaFrameAugEx) == ctypes.sizeof(_lib.PcaFrameAug) + 16 + 64 + 5 * 8 + 8 + 24


P = 0x1000
AUG = dict(jitter=0, gain_db=0.0, win_lengths=P, n_win=1, norm_mode=0, seed=0, draw=0, draw_dev=None,
           n_speed=2, nwin=8193, num_table=512, n_bg=3, ratios=(1.0, 0.8), tables=P, bg_waves=P, bg_off=P,
           bg_rms=P, clip_rms=P, bg_max_len=5000, mix_prob=0.5, snr_lo_db=0.0, snr_hi_db=20.0)


def _call(L, **over):
    """pca_frame_points_ex with valid host arguments (speed and mix on) and stand-in device addresses (a
    refused call never reads them), ``over`` replacing some."""
    aug = dict(AUG)
    a = dict(waves=P, wave_off=P, set_off=P, n_clips=2, max_len=9000, min_len=3000, clip_labels=P,
             idx=P, B=4, n_fft=256, hop=128, n_bins=129, Nt=1, farr=P, tarr=None, out=P,
             labels_out=P, meta_out=None, samples_out=None)
    for k, v in over.items():
        (aug if k in aug else a)[k] = v
    r = tuple(aug["ratios"]) + (1.0,) * (8 - len(aug["ratios"]))
    s = _lib.PcaFrameAugEx(aug["jitter"], aug["gain_db"], aug["win_lengths"], aug["n_win"],
                           aug["norm_mode"], aug["seed"], aug["draw"], aug["draw_dev"], aug["n_speed"],
                           aug["nwin"], aug["num_table"], aug["n_bg"], (ctypes.c_double * 8)(*r),
                           aug["tables"], aug["bg_waves"], aug["bg_off"], aug["bg_rms"], aug["clip_rms"],
                           aug["bg_max_len"], aug["mix_prob"], aug["snr_lo_db"], aug["snr_hi_db"])
    return L.pca_frame_points_ex(a["waves"], a["wave_off"], a["set_off"], a["n_clips"], a["max_len"],
                                 a["min_len"], a["clip_labels"], a["idx"], a["B"], a["n_fft"], a["hop"],
                                 a["n_bins"], a["Nt"], a["farr"], a["tarr"], ctypes.byref(s), a["out"],
                                 a["labels_out"], a["meta_out"], a["samples_out"], None)


NAN, INF = float("nan"), float("inf")


@pytest.mark.parametrize("over,word", [
    # everything pca_frame_points refuses
    (dict(waves=None), b"null pointer"),
    (dict(idx=None), b"null pointer"),
    (dict(win_lengths=None), b"win_lengths"),
    (dict(labels_out=None), b"go together"),
    (dict(n_fft=384), b"power of two"),
    (dict(n_fft=8192, n_bins=129), b"power of two"),
    (dict(min_len=128), b"longer than n_fft/2"),
    (dict(jitter=-1), b"jitter=-1"),
    (dict(gain_db=NAN), b"gain_db"),
    (dict(gain_db=INF), b"gain_db"),
    (dict(gain_db=-1.0), b"gain_db"),
    (dict(n_win=0), b"n_win=0"),
    (dict(norm_mode=2), b"norm_mode=2"),
    (dict(Nt=128, tarr=0x1000), b"points per set"),
    (dict(B=65536), b"B=65536"),
    (dict(hop=0), b"hop=0"),
    (dict(n_bins=130), b"n_bins=130"),
    # speed
    (dict(n_speed=0), b"n_speed=0"),
    (dict(n_speed=9), b"n_speed=9"),
    (dict(ratios=(1.0, 0.49)), b"ratios[1]=0.49"),
    (dict(ratios=(2.5, 1.0)), b"ratios[0]=2.5"),
    (dict(ratios=(1.0, NAN)), b"ratios[1]"),
    (dict(ratios=(INF, 1.0)), b"ratios[0]"),
    (dict(tables=None), b"null tables"),
    (dict(nwin=0), b"nwin=0"),
    (dict(nwin=-3), b"nwin=-3"),
    (dict(num_table=0), b"num_table=0"),
    (dict(num_table=-1), b"num_table=-1"),
    (dict(min_len=200, ratios=(1.0, 0.5)), b"min_len * ratio"),        # int(200 * 0.5) = 100 <= 128
    # mix
    (dict(mix_prob=-0.1), b"mix_prob=-0.1"),
    (dict(mix_prob=1.5), b"mix_prob=1.5"),
    (dict(mix_prob=NAN), b"mix_prob"),
    (dict(snr_lo_db=NAN), b"snr_lo_db"),
    (dict(snr_hi_db=INF), b"snr_hi_db"),
    (dict(snr_lo_db=21.0), b"snr_lo_db=21"),
    (dict(clip_rms=None), b"clip_rms"),
    (dict(bg_rms=None), b"bg_rms"),
    (dict(bg_off=None), b"bg_off"),
    (dict(n_bg=0), b"n_bg=0"),
    (dict(bg_max_len=0), b"bg_max_len=0"),
], ids=lambda v: None if isinstance(v, bytes) else "-".join(f"{k}={x}" for k, x in v.items()))
def test_entry_point_refuses_without_gpu(over, word):
    L = pca_hip.lib()
    assert _call(L, **over) == -1
    msg = L.pca_last_error()
    assert msg.startswith(b"frame_points_ex:") and word in msg, msg


def test_clip_rms_refuses_without_gpu():
    L = pca_hip.lib()
    assert L.pca_clip_rms(None, P, 2, 100, P, None) == -1
    assert L.pca_last_error().startswith(b"clip_rms: null pointer")
    assert L.pca_clip_rms(P, P, 0, 100, P, None) == -1
    assert b"n_clips=0" in L.pca_last_error()


# ---- the numpy restatement ---------------------------------------------------------------------------
def test_restatement_with_nothing_on_is_frame_ref():
    wave = orc.synth_clip(3, 7, seconds=0.1)
    L = len(wave)
    assert speed_clip(wave, 1.0) is not None and np.array_equal(speed_clip(wave, 1.0), wave)
    for centre in (0, 1, 77, 128, L // 2, L - 100, L - 1, L):          # both reflections
        for win, gain, norm, nb in ((256, 1.0, 256, 129), (200, np.float32(1.7), 200, 128)):
            got = frame_aug_ref(wave, centre, 256, win, gain, norm, nb)
            assert np.array_equal(got, frame_ref(wave, centre, 256, win, gain, norm, nb)), centre
            # alpha 0 reads no background
            assert np.array_equal(frame_aug_ref(wave, centre, 256, win, gain, norm, nb, None, 5, 0.0), got)
    assert speed_centre(1000, 1.0, L) == 1000 and speed_centre(-3, 1.0, L) == 0
    assert speed_centre(L + 9, 1.0, L) == L


def test_restatement_of_the_speed_change():
    """A tone played faster sits higher on the frequency axis, by the speed; the resampled clip is the
    oracle's, unscaled, cut to int(L * ratio) and rounded to float32."""
    fs, n_fft, f0 = 8000, 256, 500.0
    wave = np.sin(2 * np.pi * f0 * np.arange(4000) / fs).astype(np.float32)
    for speed in (0.8, 1.25):
        ratio = 1.0 / speed
        y = speed_clip(wave, speed)
        assert y.dtype == np.float32 and len(y) == int(4000 * ratio)
        full = resample_oracle.resample(wave, speed, 1.0, scale=False)
        assert np.array_equal(y, full[:len(y)].astype(np.float32))
        # the same moment of the clip: nominal centre 2000 -> round(2000 * ratio)
        c = speed_centre(2000, ratio, len(y))
        assert c == int(np.floor(2000 * ratio + 0.5))
        v = frame_aug_ref(y, c, n_fft, n_fft, 1.0, n_fft, 129)
        peak = int(np.argmax(v))
        assert abs(peak - f0 * speed / fs * n_fft) <= 1, (speed, peak)
        # amplitude kept (scale=False): log(|.| / n_fft) of a unit tone under a Hann window ~ log(1/4)
        assert abs(v[peak] - np.log(0.25)) < 0.1
    # the clamp and both reflections act in y's timeline
    y = speed_clip(wave, 1.25)
    Ly = len(y)
    assert Ly == 3200 and speed_centre(4000 + 37, 0.8, Ly) == Ly and speed_centre(-37, 0.8, Ly) == 0
    s = aug_samples(y, Ly, n_fft)
    assert np.array_equal(s[:128], y[Ly - 128:]) and np.array_equal(s[128:], y[Ly - 2:Ly - 130:-1])
    s = aug_samples(y, 0, n_fft)
    assert np.array_equal(s[128:], y[:128]) and np.array_equal(s[:128], y[128:0:-1])


def test_restatement_of_the_mix():
    rng = np.random.Generator(np.random.PCG64(2))
    wave = orc.synth_clip(5, 2, seconds=0.05)
    bg = rng.standard_normal(100).astype(np.float32)                    # shorter than n_fft: wraps twice
    alpha = np.float32(0.37)
    start = 93 + 128                                                    # p + j * hop
    s0 = aug_samples(wave, 700, 256)
    s = aug_samples(wave, 700, 256, bg, start, alpha)
    assert s.dtype == np.float32
    for n in (0, 6, 7, 99, 106, 107, 255):
        want = np.float32(np.float64(s0[n]) + np.float64(alpha) * np.float64(bg[(start + n) % 100]))
        assert s[n] == want, n
    assert np.array_equal(s[7:107] - s0[7:107] != 0, bg != 0)
    got = frame_aug_ref(wave, 700, 256, 200, np.float32(0.9), 256, 129, bg, start, alpha)
    assert np.array_equal(got, frame_of_samples(s, 200, np.float32(0.9), 256, 129))
    assert not np.array_equal(got, frame_ref(wave, 700, 256, 200, np.float32(0.9), 256, 129))


# ---- the datasets ------------------------------------------------------------------------------------
def test_dataset_options_on_the_host():
    import dataset
    lens = [2205, 4851, 16170]
    clips = [np.zeros(n, dtype=np.float32) for n in lens]
    y = [3, 1, 4]
    mk = lambda **kw: dataset.ESC_wave_pc(clips, y, 44100, 64, **kw)    # noqa: E731
    off = mk()
    assert not off.stochastic and off.speeds == (1.0,) and off.ratios == (1.0,) and off.mix_prob == 0.0
    assert not mk(speeds=(1.0,)).stochastic
    assert not mk(mix_clips="self").stochastic                          # mix_prob 0: off
    for kw in (dict(speeds=(1.0, 0.8)), dict(speeds=(1.25,)), dict(mix_clips="self", mix_prob=0.3),
               dict(mix_clips=[np.ones(10, np.float32)], mix_prob=1.0)):
        for d in (mk(**kw), dataset.ESC_wave_pc_temp(clips, y, 44100, 64, 4, **kw)):
            assert d.stochastic
            v = d.plain()
            assert not v.stochastic and v.speeds == (1.0,) and v.ratios == (1.0,) and v.mix_prob == 0.0
            assert v._store is d._store                                 # one resident store
            assert d.stochastic                                         # the view switched nothing off here
    d = mk(speeds=(1.0, 0.8, 1.25))
    assert d.ratios == (1.0, 1.0 / 0.8, 1.0 / 1.25)
    assert mk(mix_clips="self", mix_prob=0.5, mix_snr_db=(5, 5)).mix_snr_db == (5.0, 5.0)
    for kw in (dict(speeds=(1.0, 0.49)), dict(speeds=(2.01,)), dict(speeds=()), dict(speeds=(1.0,) * 9),
               dict(speeds=(float("nan"),)),
               dict(mix_clips="self", mix_prob=-0.1), dict(mix_clips="self", mix_prob=1.1),
               dict(mix_clips="self", mix_prob=0.5, mix_snr_db=(20.0, 0.0)),
               dict(mix_clips="self", mix_prob=0.5, mix_snr_db=(0.0, float("inf"))),
               dict(mix_prob=0.5), dict(mix_clips="other", mix_prob=0.5),
               dict(mix_clips=[], mix_prob=0.5), dict(mix_clips=[np.zeros(0, np.float32)], mix_prob=0.5)):
        with pytest.raises(ValueError):
            mk(**kw)
    # the shortest clip, played at the fastest speed, still covers the reflect padding
    with pytest.raises(ValueError):
        dataset.ESC_wave_pc([np.zeros(60, np.float32)], [0], 44100, 64, speeds=(1.0, 2.0))
    dataset.ESC_wave_pc([np.zeros(66, np.float32)], [0], 44100, 64, speeds=(1.0, 2.0))
