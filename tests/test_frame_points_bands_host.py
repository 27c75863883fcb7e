"""pca_frame_points_bands without a GPU: the symbol and its prototype, the entry point's host checks, the mel
formulae of pca_hip.mel_bank against their independent restatement (tests/bands_ref.py), the packing of
pca_hip.FilterBank, and the host side of the datasets' ``bands=``."""
import ctypes
import os
import re

import numpy as np
import pytest

import pca_hip
from pca_hip import _lib

import bands_ref

FS = 44100
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ---- the symbol -------------------------------------------------------------------------------------------
def test_symbol_is_declared_exported_and_bound():
    header = open(os.path.join(ROOT, "include", "pca_hip.h")).read()
    assert re.search(r"\bint pca_frame_points_bands\(", header)
    assert "typedef struct PcaFrameBands {" in header and "#define PCA_ABI_VERSION 2" in header
    L = pca_hip.lib()
    assert L.pca_abi_version() == 2
    res, args = _lib.SIGNATURES["pca_frame_points_bands"]
    fn = L.pca_frame_points_bands                                       # AttributeError if not exported
    assert fn.restype is res is ctypes.c_int and list(fn.argtypes) == args and len(args) == 20
    assert args[14] == ctypes.POINTER(_lib.PcaFrameAug) and args[15] == ctypes.POINTER(_lib.PcaFrameBands)
    # pca_frame_points' prototype with n_bins taken out and the bank put in behind aug
    plain = list(_lib.SIGNATURES["pca_frame_points"][1])
    assert args == plain[:11] + plain[12:16] + [ctypes.POINTER(_lib.PcaFrameBands)] + plain[16:]
    assert [n for n, _ in _lib.PcaFrameBands._fields_] == ["n_bands", "nnz", "band_lo", "band_off", "weights",
                                                           "power", "amin"]
    assert ctypes.sizeof(_lib.PcaFrameBands) == 40
    for name in ("FilterBank", "mel_bank", "frame_points_bands"):
        assert hasattr(pca_hip, name), name


# ---- the entry point's refusals ---------------------------------------------------------------------------
P = 0x1000


def _call(L, bank="default", **over):
    """pca_frame_points_bands with valid host arguments and stand-in device addresses (a refused call never
    reads them), ``over`` replacing some; ``bank`` "null": no bank at all."""
    aug = dict(jitter=0, gain_db=0.0, win_lengths=P, n_win=1, norm_mode=0, seed=0, draw=0, draw_dev=None)
    bk = dict(n_bands=16, nnz=227, band_lo=P, band_off=P, weights=P, power=2, amin=1e-8)
    a = dict(waves=P, wave_off=P, set_off=P, n_clips=2, max_len=9000, min_len=3000, clip_labels=P, idx=P,
             B=4, n_fft=256, hop=128, Nt=2, farr=P, tarr=P, out=P, labels_out=P, meta_out=None, aug="given")
    for k, v in over.items():
        (aug if k in aug else bk if k in bk else a)[k] = v
    s = _lib.PcaFrameAug(aug["jitter"], aug["gain_db"], aug["win_lengths"], aug["n_win"], aug["norm_mode"],
                         aug["seed"], aug["draw"], aug["draw_dev"])
    b = _lib.PcaFrameBands(bk["n_bands"], bk["nnz"], bk["band_lo"], bk["band_off"], bk["weights"],
                           bk["power"], bk["amin"])
    return L.pca_frame_points_bands(a["waves"], a["wave_off"], a["set_off"], a["n_clips"], a["max_len"],
                                    a["min_len"], a["clip_labels"], a["idx"], a["B"], a["n_fft"], a["hop"],
                                    a["Nt"], a["farr"], a["tarr"], None if a["aug"] is None else ctypes.byref(s),
                                    None if bank == "null" else ctypes.byref(b), a["out"], a["labels_out"],
                                    a["meta_out"], None)


@pytest.mark.parametrize("bank,over,word", [
    ("null", {}, b"null pointer"),
    ("default", dict(waves=None), b"null pointer"),
    ("default", dict(wave_off=None), b"null pointer"),
    ("default", dict(set_off=None), b"null pointer"),
    ("default", dict(idx=None), b"null pointer"),
    ("default", dict(farr=None), b"null pointer"),
    ("default", dict(aug=None), b"null pointer"),
    ("default", dict(out=None), b"null pointer"),
    ("default", dict(win_lengths=None), b"null win_lengths"),
    ("default", dict(band_lo=None), b"null pointer"),
    ("default", dict(band_off=None), b"null pointer"),
    ("default", dict(weights=None), b"null pointer"),
    ("default", dict(n_bands=0), b"n_bands=0"),
    ("default", dict(n_bands=-3), b"n_bands=-3"),
    ("default", dict(nnz=15), b"nnz=15"),
    ("default", dict(power=0), b"power=0"),
    ("default", dict(power=3), b"power=3"),
    ("default", dict(amin=0.0), b"amin"),
    ("default", dict(amin=-1e-8), b"amin"),
    ("default", dict(amin=float("inf")), b"amin"),
    ("default", dict(amin=float("nan")), b"amin"),
    ("default", dict(n_bands=8193, nnz=9000), b"points per set"),       # 2 * 8193 = 16386
    ("default", dict(n_fft=384), b"n_fft=384"),
    ("default", dict(n_fft=32), b"n_fft=32"),
    ("default", dict(n_fft=8192), b"n_fft=8192"),
    ("default", dict(hop=0), b"hop=0"),
    ("default", dict(Nt=0), b"Nt=0"),
    ("default", dict(B=0), b"B=0"),
    ("default", dict(B=65536), b"B=65536"),
    ("default", dict(n_clips=0), b"n_clips=0"),
    ("default", dict(min_len=128), b"longer than n_fft/2"),
    ("default", dict(max_len=2000), b"longer than n_fft/2"),            # max_len < min_len
    ("default", dict(max_len=1 << 31), b"int32 centres"),
    ("default", dict(labels_out=None), b"go together"),
    ("default", dict(clip_labels=None), b"go together"),
    ("default", dict(jitter=-1), b"jitter=-1"),
    ("default", dict(jitter=(1 << 30) + 1), b"jitter="),
    ("default", dict(gain_db=float("nan")), b"gain_db"),
    ("default", dict(gain_db=float("inf")), b"gain_db"),
    ("default", dict(gain_db=-1.0), b"gain_db"),
    ("default", dict(n_win=0), b"n_win=0"),
    ("default", dict(norm_mode=2), b"norm_mode=2"),
], ids=lambda v: None if isinstance(v, bytes) else
    ("-".join(f"{k}={x}" for k, x in v.items()) if isinstance(v, dict) else None))
def test_entry_point_refuses_without_gpu(bank, over, word):
    L = pca_hip.lib()
    assert _call(L, bank, **over) == -1
    msg = L.pca_last_error()
    assert msg.startswith(b"frame_points_bands:") and word in msg, msg


def test_binding_refuses_before_any_tensor_is_read():
    bank = pca_hip.mel_bank(FS, 256, 16)
    with pytest.raises(TypeError, match="FilterBank"):
        pca_hip.frame_points_bands(None, None, None, None, 256, 128, object(), None, max_len=1, min_len=1)
    with pytest.raises(ValueError, match="129 bins"):
        pca_hip.frame_points_bands(None, None, None, None, 512, 256, bank, None, max_len=1, min_len=1)


# ---- mel_bank ---------------------------------------------------------------------------------------------
MEL_SHAPES = [(256, 16, False), (512, 64, False), (1024, 64, False), (2048, 128, False), (64, 8, True)]


def test_mel_scale():
    assert bands_ref.hz_to_mel(1000.0) == 15.0 and pca_hip.ops._hz_to_mel(1000.0, False) == 15.0
    assert abs(float(pca_hip.ops._hz_to_mel(500.0, False)) - 7.5) < 1e-12
    assert abs(float(pca_hip.ops._hz_to_mel(6400.0, False)) - 42.0) < 1e-12     # 15 + 27
    assert abs(float(pca_hip.ops._hz_to_mel(700.0, True)) - 2595.0 * np.log10(2.0)) < 1e-12
    for htk in (False, True):
        f = np.array([0.0, 30.0, 999.0, 1000.0, 1001.0, 8000.0, 22050.0])
        assert np.abs(pca_hip.ops._mel_to_hz(pca_hip.ops._hz_to_mel(f, htk), htk) - f).max() < 1e-9
        for v in f:
            assert abs(float(pca_hip.ops._hz_to_mel(v, htk)) - bands_ref.hz_to_mel(float(v), htk)) < 1e-12


@pytest.mark.parametrize("n_fft,n_mels,htk", MEL_SHAPES, ids=lambda v: str(v))
def test_mel_bank_properties(n_fft, n_mels, htk):
    bank = pca_hip.mel_bank(FS, n_fft, n_mels, htk=htk)                 # no empty band: it would raise
    flat = pca_hip.mel_bank(FS, n_fft, n_mels, htk=htk, norm=None)
    assert bank.n_bands == flat.n_bands == n_mels and bank.n_src == n_fft // 2 + 1 and bank.n_fft == n_fft
    assert bank.power == 2 and bank.amin == 1e-8
    p = bands_ref.mel_points(FS, n_mels, htk=htk)
    assert np.abs(bank.centres - p[1:-1]).max() < 1e-9 and np.all(np.diff(bank.centres) > 0)
    assert abs(p[0]) < 1e-9 and abs(p[-1] - FS / 2) < 1e-6
    for W in (bank.W, flat.W):
        assert W.shape == (n_mels, n_fft // 2 + 1) and (W >= 0).all()
        for m in range(n_mels):
            nz = np.flatnonzero(W[m])
            assert nz.size >= 1 and np.array_equal(nz, np.arange(nz[0], nz[-1] + 1)), m     # contiguous
    assert flat.W.max() <= 1.0
    assert np.abs(bank.W - flat.W * (2.0 / (p[2:] - p[:-2]))[:, None]).max() < 1e-15
    for b, norm in ((bank, "slaney"), (flat, None)):
        assert np.abs(b.W - bands_ref.mel_matrix(FS, n_fft, n_mels, htk=htk, norm=norm)).max() <= 1e-12
    # a mel band is narrow: what the kernel's four-lanes-a-band mapping is sized for
    # (neighbouring triangles overlap by half, so every bin lies in at most two of them)
    assert np.diff(bank.band_off).max() <= 65 and bank.nnz <= 2 * (n_fft // 2 + 1)


def test_mel_bank_names_the_empty_band():
    W = bands_ref.mel_matrix(FS, 256, 32, htk=True)
    assert [m for m in range(32) if not W[m].any()] == [0]              # exactly one, between bins 0 and 1
    with pytest.raises(ValueError, match=r"band 0 has no non-zero weight"):
        pca_hip.mel_bank(FS, 256, 32, htk=True)
    for bad in (dict(n_mels=0), dict(norm="l2"), dict(fmin=100.0, fmax=50.0), dict(fmax=FS)):
        with pytest.raises(ValueError):
            pca_hip.mel_bank(FS, 256, **dict(dict(n_mels=8), **bad))
    assert pca_hip.mel_bank(FS, 256, 8, fmin=300.0, fmax=8000.0, power=1, amin=1e-5).summary() == dict(
        n_bands=8, power=1, amin=1e-5, nnz=pca_hip.mel_bank(FS, 256, 8, fmin=300.0, fmax=8000.0).nnz)


# ---- FilterBank -------------------------------------------------------------------------------------------
def test_filter_bank_packing_round_trips():
    rng = np.random.Generator(np.random.PCG64(3))
    W = np.zeros((5, 33))
    W[0, :] = 1.0                                                       # every bin
    W[1, 32] = 0.25                                                     # Nyquist alone
    W[2, 3:9] = [0.5, 0.0, 0.0, 1.5, 0.0, 2.0]                          # zeros inside the span are kept
    W[3, 6:12] = rng.uniform(0.1, 1.0, 6)
    W[4, 0] = 1e-3
    bank = pca_hip.FilterBank(W, np.arange(5) * 100.0, power=1, amin=1e-6)
    assert bank.n_bands == 5 and bank.n_src == 33 and bank.n_fft == 64 and bank.power == 1
    assert bank.band_lo.tolist() == [0, 32, 3, 6, 0] and bank.band_off.tolist() == [0, 33, 34, 40, 46, 47]
    assert bank.nnz == 47 and bank.weights.dtype == np.float32 and bank.band_lo.dtype == np.int32
    assert np.array_equal(bank.dense(), W.astype(np.float32).astype(np.float64))
    assert np.array_equal(bank.W, W)
    assert bank.summary() == dict(n_bands=5, power=1, amin=1e-6, nnz=47)
    for n_fft, n_mels in ((256, 16), (1024, 64)):
        mel = pca_hip.mel_bank(FS, n_fft, n_mels)
        assert np.array_equal(mel.dense(), mel.W.astype(np.float32).astype(np.float64))
    # the raw form clips as the launch does
    raw = pca_hip.FilterBank.from_packed([-2, 30, 40], [0, 4, 9, 10], np.arange(1, 11), 33)
    D = raw.dense()
    assert D[0].tolist()[:3] == [3.0, 4.0, 0.0] and D[1, 30:].tolist() == [5.0, 6.0, 7.0] and not D[2].any()
    assert raw.centres.tolist() == [0.0, 1.0, 2.0]


@pytest.mark.parametrize("make,word", [
    (lambda: pca_hip.FilterBank(np.ones((2, 33)) * [[1.0], [0.0]], [0, 1]), "band 1 has no non-zero weight"),
    (lambda: pca_hip.FilterBank(-np.ones((2, 33)), [0, 1]), "negative or non-finite"),
    (lambda: pca_hip.FilterBank(np.full((2, 33), np.nan), [0, 1]), "negative or non-finite"),
    (lambda: pca_hip.FilterBank(np.full((2, 33), np.inf), [0, 1]), "negative or non-finite"),
    (lambda: pca_hip.FilterBank(np.ones(33), [0]), "shape"),
    (lambda: pca_hip.FilterBank(np.ones((2, 34)), [0, 1]), "power of two"),
    (lambda: pca_hip.FilterBank(np.ones((2, 33)), [0, 1, 2]), "centres"),
    (lambda: pca_hip.FilterBank(np.ones((2, 33)), [0, 1], power=3), "power 3"),
    (lambda: pca_hip.FilterBank(np.ones((2, 33)), [0, 1], amin=0.0), "amin"),
    (lambda: pca_hip.FilterBank(np.ones((2, 33)), [0, 1], amin=float("nan")), "amin"),
    (lambda: pca_hip.FilterBank(np.ones((2, 33)), [0, 1], amin=1e-60), "amin"),      # 0 in fp32
    (lambda: pca_hip.FilterBank.from_packed([0, 1], [0, 1], [1.0, 1.0], 33), "offsets"),
    (lambda: pca_hip.FilterBank.from_packed([0, 1], [0, 1, 2], [1.0], 33), "weights"),
], ids=["empty-band", "negative", "nan", "inf", "1-d", "columns", "centres", "power", "amin-0", "amin-nan",
        "amin-fp32", "packed-offsets", "packed-nnz"])
def test_filter_bank_refuses(make, word):
    with pytest.raises(ValueError, match=word):
        make()


# ---- the datasets -----------------------------------------------------------------------------------------
def _clips():
    lens = [2205, 4851, 16170]
    return [np.zeros(n, dtype=np.float32) for n in lens], [3, 1, 4]


def test_dataset_host_side():
    import dataset
    clips, y = _clips()
    bank = pca_hip.mel_bank(FS, 256, 16)
    grid = dataset.ESC_wave_pc(clips, y, FS, 256)
    ds = dataset.ESC_wave_pc(clips, y, FS, 256, bands=bank, jitter=5)
    assert grid.bands is None and grid.F == 129 and grid.num_points == 129
    assert ds.bands is bank and ds.F == 16 and ds.num_points == 16 and len(ds) == len(grid)
    assert np.array_equal(ds.farr, bank.centres / FS) and ds.tarr is None
    assert ds.stochastic and not ds.variable_length and not ds.soft_targets
    p = ds.plain()
    assert p.bands is bank and p.F == 16 and not p.stochastic and p._store is ds._store   # a representation
    assert not dataset.ESC_wave_pc(clips, y, FS, 256, bands=bank).stochastic
    back = ds.with_bands(None)
    assert back.bands is None and back.F == 129 and np.array_equal(back.farr, grid.farr)
    assert back._store is ds._store and back.jitter == 5
    other = grid.with_bands(pca_hip.mel_bank(FS, 256, 8))
    assert other.F == 8 and grid.F == 129 and other._store is grid._store
    t = dataset.ESC_wave_pc_temp(clips, y, FS, 256, 4, bands=bank)
    assert t.F == 16 and t.num_points == 64 and t.tarr is not None and t.with_bands(None).F == 128
    assert np.array_equal(t.with_bands(None).farr, dataset.ESC_wave_pc_temp(clips, y, FS, 256, 4).farr)
    peaks = dataset.PeakPoints(t, 8)
    assert (peaks.F, peaks.Nt, peaks.din) == (16, 4, 3)


@pytest.mark.parametrize("kw", [
    dict(speeds=(1.0, 1.1)), dict(mix_clips="self", mix_prob=0.5), dict(mix_clips="self", mix_targets=True),
    dict(freq_masks=1, freq_mask_width=4), dict(reassign=True), dict(drop_nyquist=True),
], ids=["speeds", "mix", "mix-targets", "masks", "reassign", "drop-nyquist"])
def test_dataset_refuses_what_lives_in_other_launches(kw):
    import dataset
    clips, y = _clips()
    bank = pca_hip.mel_bank(FS, 256, 16)
    with pytest.raises(ValueError, match="out of scope"):
        dataset.ESC_wave_pc(clips, y, FS, 256, bands=bank, **kw)
    with pytest.raises(ValueError, match="out of scope"):
        dataset.ESC_wave_pc(clips, y, FS, 256, **kw).with_bands(bank)
    assert dataset.ESC_wave_pc(clips, y, FS, 256, **kw).with_bands(None).F in (128, 129)


def test_dataset_refuses_the_rest():
    import dataset
    clips, y = _clips()
    bank = pca_hip.mel_bank(FS, 256, 16)
    with pytest.raises(ValueError, match="out of scope"):
        dataset.ESC_wave_pc_temp(clips, y, FS, 256, 4, bands=bank, time_masks=1, time_mask_width=1)
    with pytest.raises(ValueError, match="257"):
        dataset.ESC_wave_pc(clips, y, FS, 512, bands=bank)              # a bank of another n_fft
    with pytest.raises(TypeError, match="FilterBank"):
        dataset.ESC_wave_pc(clips, y, FS, 256, bands=16)
    with pytest.raises(ValueError, match="bands"):
        dataset.ESC_wave_pc(clips, y, FS, 256, bands=bank).with_reassign(True)
    wide = pca_hip.FilterBank.from_packed(np.zeros(8192), np.arange(8193), np.ones(8192), 129)
    with pytest.raises(ValueError, match="points per set"):
        dataset.ESC_wave_pc_temp(clips, y, FS, 256, 4, bands=wide)


def test_band_sweep_is_listed():
    import evalsweep
    assert "band_sweep" in evalsweep.__all__
    with pytest.raises(ValueError, match="no banks"):
        evalsweep.band_sweep(None, [], [], FS, 256, [])
    with pytest.raises(ValueError, match="band 0"):
        evalsweep.band_sweep(None, [], [], FS, 256, [32], htk=True)
