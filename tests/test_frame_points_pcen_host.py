"""pca_frame_points_pcen without a GPU: the symbol and its prototype, the entry point's host checks,
``pca_hip.Pcen`` and its coefficient, the host side of the datasets' ``pcen=``, and the numpy restatement
(tests/pcen_ref.py) against itself."""
import ctypes
import math
import os
import re

import numpy as np
import pytest

import pca_hip
from pca_hip import _lib

import pcen_ref

FS = 44100
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ---- the symbol -------------------------------------------------------------------------------------------
def test_symbol_is_declared_exported_and_bound():
    header = open(os.path.join(ROOT, "include", "pca_hip.h")).read()
    assert re.search(r"\bint pca_frame_points_pcen\(", header)
    assert "typedef struct PcaPcen {" in header and "#define PCA_ABI_VERSION 2" in header
    L = pca_hip.lib()
    res, args = _lib.SIGNATURES["pca_frame_points_pcen"]
    fn = L.pca_frame_points_pcen                                        # AttributeError if not exported
    assert fn.restype is res is ctypes.c_int and list(fn.argtypes) == args and len(args) == 24
    # pca_frame_points_bands' prototype with the spec, the workspace, its size and the tickets behind the bank
    bands = list(_lib.SIGNATURES["pca_frame_points_bands"][1])
    assert args == bands[:16] + [ctypes.POINTER(_lib.PcaPcen), ctypes.c_void_p, ctypes.c_int64,
                                 ctypes.c_void_p] + bands[16:]
    # the header's parameter list, type by type
    proto = re.search(r"\bint pca_frame_points_pcen\((.*?)\);", header, re.S).group(1)
    kinds = []
    for prm in proto.split(","):
        prm = " ".join(prm.split())
        kinds.append("ptr" if "*" in prm else prm.rsplit(" ", 1)[0])
    want = {ctypes.c_int: "int", ctypes.c_int64: "int64_t"}
    assert len(kinds) == 24
    for k, a in zip(kinds, args):
        assert k == want.get(a, "ptr"), (k, a)
    assert [n for n, _ in _lib.PcaPcen._fields_] == ["context", "s", "gain", "bias", "r", "eps", "scale"]
    assert ctypes.sizeof(_lib.PcaPcen) == 28
    fields = re.search(r"typedef struct PcaPcen \{(.*?)\} PcaPcen;", header, re.S).group(1)
    assert re.findall(r"(int32_t|float)\s+(\w+);", fields) == [
        ("int32_t", "context"), ("float", "s"), ("float", "gain"), ("float", "bias"), ("float", "r"),
        ("float", "eps"), ("float", "scale")]
    for name in ("Pcen", "frame_points_pcen"):
        assert hasattr(pca_hip, name), name


# ---- the entry point's refusals ---------------------------------------------------------------------------
P = 0x1000


def _call(L, bank="default", spec="default", **over):
    """pca_frame_points_pcen with valid host arguments and stand-in device addresses (a refused call never
    reads them), ``over`` replacing some; ``bank`` / ``spec`` "null": none at all."""
    aug = dict(jitter=0, gain_db=0.0, win_lengths=P, n_win=1, norm_mode=0, seed=0, draw=0, draw_dev=None)
    bk = dict(n_bands=16, nnz=227, band_lo=P, band_off=P, weights=P, power=2, amin=1e-8)
    pc = dict(context=8, s=0.025, pgain=0.98, bias=2.0, r=0.5, eps=1e-6, scale=1.0)
    a = dict(waves=P, wave_off=P, set_off=P, n_clips=2, max_len=9000, min_len=3000, clip_labels=P, idx=P,
             B=4, n_fft=256, hop=128, Nt=2, farr=P, tarr=P, out=P, labels_out=P, meta_out=None, aug="given",
             energy_ws=P, energy_ws_elems=4 * 10 * 16, tickets=P)
    for k, v in over.items():
        (aug if k in aug else bk if k in bk else pc if k in pc else a)[k] = v
    s = _lib.PcaFrameAug(aug["jitter"], aug["gain_db"], aug["win_lengths"], aug["n_win"], aug["norm_mode"],
                         aug["seed"], aug["draw"], aug["draw_dev"])
    b = _lib.PcaFrameBands(bk["n_bands"], bk["nnz"], bk["band_lo"], bk["band_off"], bk["weights"],
                           bk["power"], bk["amin"])
    p = _lib.PcaPcen(pc["context"], pc["s"], pc["pgain"], pc["bias"], pc["r"], pc["eps"], pc["scale"])
    return L.pca_frame_points_pcen(a["waves"], a["wave_off"], a["set_off"], a["n_clips"], a["max_len"],
                                   a["min_len"], a["clip_labels"], a["idx"], a["B"], a["n_fft"], a["hop"],
                                   a["Nt"], a["farr"], a["tarr"], None if a["aug"] is None else ctypes.byref(s),
                                   None if bank == "null" else ctypes.byref(b),
                                   None if spec == "null" else ctypes.byref(p), a["energy_ws"],
                                   a["energy_ws_elems"], a["tickets"], a["out"], a["labels_out"],
                                   a["meta_out"], None)


NAN, INF = float("nan"), float("inf")


@pytest.mark.parametrize("bank,spec,over,word", [
    # the spec
    ("default", "null", {}, b"null pointer"),
    ("default", "default", dict(context=-1), b"context=-1"),
    ("default", "default", dict(context=256, energy_ws_elems=1 << 40), b"context=256"),
    ("default", "default", dict(s=0.0), b"s=0 outside (0, 1]"),
    ("default", "default", dict(s=-0.5), b"s=-0.5"),
    ("default", "default", dict(s=1.5), b"s=1.5"),
    ("default", "default", dict(s=NAN), b"s="),
    ("default", "default", dict(pgain=-0.1), b"gain=-0.1"),
    ("default", "default", dict(pgain=4.5), b"gain=4.5"),
    ("default", "default", dict(pgain=NAN), b"gain="),
    ("default", "default", dict(bias=-1.0), b"bias=-1"),
    ("default", "default", dict(bias=2e6), b"bias=2e+06"),
    ("default", "default", dict(bias=NAN), b"bias="),
    ("default", "default", dict(r=0.0), b"r=0 outside (0, 1]"),
    ("default", "default", dict(r=1.25), b"r=1.25"),
    ("default", "default", dict(r=NAN), b"r="),
    ("default", "default", dict(eps=0.0), b"eps="),
    ("default", "default", dict(eps=-1e-6), b"eps="),
    ("default", "default", dict(eps=INF), b"eps="),
    ("default", "default", dict(eps=NAN), b"eps="),
    ("default", "default", dict(scale=0.0), b"scale="),
    ("default", "default", dict(scale=-2.0), b"scale="),
    ("default", "default", dict(scale=INF), b"scale="),
    ("default", "default", dict(scale=NAN), b"scale="),
    # the workspace: B = 4 slots of (8 + 2) * 16 doubles
    ("default", "default", dict(energy_ws_elems=4 * 10 * 16 - 1), b"workspace"),
    ("default", "default", dict(energy_ws_elems=10 * 16), b"workspace"),
    ("default", "default", dict(energy_ws_elems=-1), b"workspace"),
    ("default", "default", dict(context=9), b"workspace"),
    ("default", "default", dict(energy_ws=None), b"null pointer"),
    ("default", "default", dict(tickets=None), b"null pointer"),
    # what pca_frame_points_bands rejects
    ("null", "default", {}, b"null pointer"),
    ("default", "default", dict(waves=None), b"null pointer"),
    ("default", "default", dict(wave_off=None), b"null pointer"),
    ("default", "default", dict(set_off=None), b"null pointer"),
    ("default", "default", dict(idx=None), b"null pointer"),
    ("default", "default", dict(farr=None), b"null pointer"),
    ("default", "default", dict(aug=None), b"null pointer"),
    ("default", "default", dict(out=None), b"null pointer"),
    ("default", "default", dict(win_lengths=None), b"null win_lengths"),
    ("default", "default", dict(band_lo=None), b"null pointer"),
    ("default", "default", dict(band_off=None), b"null pointer"),
    ("default", "default", dict(weights=None), b"null pointer"),
    ("default", "default", dict(n_bands=0), b"n_bands=0"),
    ("default", "default", dict(n_bands=-3), b"n_bands=-3"),
    ("default", "default", dict(nnz=15), b"nnz=15"),
    ("default", "default", dict(power=0), b"power=0"),
    ("default", "default", dict(power=3), b"power=3"),
    ("default", "default", dict(amin=0.0), b"amin"),
    ("default", "default", dict(amin=NAN), b"amin"),
    ("default", "default", dict(n_bands=8193, nnz=9000, energy_ws_elems=1 << 40), b"points per set"),
    ("default", "default", dict(n_fft=384), b"n_fft=384"),
    ("default", "default", dict(n_fft=32), b"n_fft=32"),
    ("default", "default", dict(n_fft=8192), b"n_fft=8192"),
    ("default", "default", dict(hop=0), b"hop=0"),
    ("default", "default", dict(Nt=0), b"Nt=0"),
    ("default", "default", dict(B=0), b"B=0"),
    ("default", "default", dict(B=65536), b"B=65536"),
    ("default", "default", dict(n_clips=0), b"n_clips=0"),
    ("default", "default", dict(min_len=128), b"longer than n_fft/2"),
    ("default", "default", dict(max_len=2000), b"longer than n_fft/2"),
    ("default", "default", dict(max_len=1 << 31), b"int32 centres"),
    ("default", "default", dict(labels_out=None), b"go together"),
    ("default", "default", dict(clip_labels=None), b"go together"),
    ("default", "default", dict(jitter=-1), b"jitter=-1"),
    ("default", "default", dict(jitter=(1 << 30) + 1), b"jitter="),
    ("default", "default", dict(gain_db=NAN), b"gain_db"),
    ("default", "default", dict(gain_db=INF), b"gain_db"),
    ("default", "default", dict(gain_db=-1.0), b"gain_db"),
    ("default", "default", dict(n_win=0), b"n_win=0"),
    ("default", "default", dict(norm_mode=2), b"norm_mode=2"),
], ids=lambda v: None if isinstance(v, bytes) else
    ("-".join(f"{k}={x}" for k, x in v.items()) if isinstance(v, dict) else None))
def test_entry_point_refuses_without_gpu(bank, spec, over, word):
    L = pca_hip.lib()
    assert _call(L, bank, spec, **over) == -1
    msg = L.pca_last_error()
    assert msg.startswith(b"frame_points_pcen:") and word in msg, msg


def test_binding_refuses_before_any_tensor_is_read():
    bank = pca_hip.mel_bank(FS, 256, 16)
    kw = dict(max_len=1, min_len=1, fs=FS)
    with pytest.raises(TypeError, match="FilterBank"):
        pca_hip.frame_points_pcen(None, None, None, None, 256, 128, object(), None, pcen=pca_hip.Pcen(), **kw)
    with pytest.raises(TypeError, match="Pcen"):
        pca_hip.frame_points_pcen(None, None, None, None, 256, 128, bank, None, pcen=dict(context=3), **kw)
    with pytest.raises(ValueError, match="129 bins"):
        pca_hip.frame_points_pcen(None, None, None, None, 512, 256, bank, None, pcen=pca_hip.Pcen(), **kw)


# ---- Pcen -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("tc,fs,hop", [(0.4, 22050, 512), (0.06, 44100, 128), (1.0, 16000, 160)])
def test_coefficient_is_the_closed_form(tc, fs, hop):
    p = pca_hip.Pcen(time_constant=tc)
    t = tc * fs / hop
    s = p.coefficient(fs, hop)
    assert abs(s - (math.sqrt(1.0 + 4.0 * t * t) - 1.0) / (2.0 * t * t)) <= 1e-15
    # the root in (0, 1) of t^2 s^2 + s - 1 = 0: what makes the one-pole filter's time constant t frames
    assert 0.0 < s < 1.0 and abs(t * t * s * s + s - 1.0) <= 1e-12
    assert pca_hip.Pcen(time_constant=tc, s=0.25).coefficient(fs, hop) == 0.25       # a given s wins
    c = p.struct(fs, hop)
    assert c.context == 32 and c.s == np.float32(s) and c.r == 0.5 and c.bias == 2.0


def test_pcen_is_an_immutable_checked_spec():
    p = pca_hip.Pcen()
    assert p.summary() == dict(context=32, time_constant=0.4, gain=0.98, bias=2.0, power=0.5, eps=1e-6,
                               scale=1.0, s=None)
    assert abs(p.coefficient(22050, 512) - 0.05638) < 1e-5              # librosa's default framing
    with pytest.raises(AttributeError):
        p.gain = 0.5
    assert p == pca_hip.Pcen() and hash(p) == hash(pca_hip.Pcen()) and p != pca_hip.Pcen(context=8)
    for bad in (dict(context=-1), dict(context=256), dict(s=0.0), dict(s=1.5), dict(s=NAN), dict(gain=-0.1),
                dict(gain=4.5), dict(gain=NAN), dict(bias=-1.0), dict(bias=2e6), dict(power=0.0),
                dict(power=1.5), dict(eps=0.0), dict(eps=INF), dict(eps=1e-60), dict(scale=0.0),
                dict(scale=NAN), dict(time_constant=0.0), dict(time_constant=INF)):
        with pytest.raises(ValueError, match="Pcen"):
            pca_hip.Pcen(**bad)
    assert pca_hip.Pcen(context=0, s=1.0, gain=0.0, bias=0.0, power=1.0).struct(FS, 128).s == 1.0


# ---- the datasets -----------------------------------------------------------------------------------------
def _clips():
    lens = [2205, 4851, 16170]
    return [np.zeros(n, dtype=np.float32) for n in lens], [3, 1, 4]


def test_dataset_host_side():
    import dataset
    clips, y = _clips()
    bank = pca_hip.mel_bank(FS, 256, 16)
    spec = pca_hip.Pcen(context=8)
    band = dataset.ESC_wave_pc(clips, y, FS, 256, bands=bank, jitter=5)
    ds = dataset.ESC_wave_pc(clips, y, FS, 256, bands=bank, pcen=spec, jitter=5)
    assert band.pcen is None and ds.pcen is spec and ds.bands is bank
    assert (ds.F, ds.num_points, len(ds)) == (band.F, band.num_points, len(band)) == (16, 16, len(band))
    assert np.array_equal(ds.farr, band.farr) and ds.tarr is None
    assert ds.stochastic and not ds.variable_length and not ds.soft_targets
    assert not dataset.ESC_wave_pc(clips, y, FS, 256, bands=bank, pcen=spec).stochastic     # a representation
    p = ds.plain()
    assert p.pcen is spec and p.bands is bank and not p.stochastic and p._store is ds._store
    back = ds.with_pcen(None)
    assert back.pcen is None and back.bands is bank and back._store is ds._store and back.jitter == 5
    other = band.with_pcen(pca_hip.Pcen(context=3, s=0.5))
    assert other.pcen.context == 3 and band.pcen is None and other._store is band._store
    assert ds.with_bands(pca_hip.mel_bank(FS, 256, 8)).pcen is spec     # another bank keeps it
    grid = ds.with_bands(None)                                          # the bank takes it along
    assert grid.pcen is None and grid.bands is None and grid.F == 129
    t = dataset.ESC_wave_pc_temp(clips, y, FS, 256, 4, bands=bank, pcen=spec)
    assert t.F == 16 and t.num_points == 64 and t.tarr is not None and t.pcen is spec
    peaks = dataset.PeakPoints(t, 8)
    assert (peaks.F, peaks.Nt, peaks.din) == (16, 4, 3)


def test_dataset_pcen_needs_bands():
    import dataset
    clips, y = _clips()
    spec = pca_hip.Pcen()
    with pytest.raises(ValueError, match="pcen needs bands"):
        dataset.ESC_wave_pc(clips, y, FS, 256, pcen=spec)
    with pytest.raises(ValueError, match="pcen needs bands"):
        dataset.ESC_wave_pc_temp(clips, y, FS, 256, 4, pcen=spec)
    with pytest.raises(ValueError, match="pcen needs bands"):
        dataset.ESC_wave_pc(clips, y, FS, 256).with_pcen(spec)
    with pytest.raises(TypeError, match="Pcen"):
        dataset.ESC_wave_pc(clips, y, FS, 256, bands=pca_hip.mel_bank(FS, 256, 16), pcen=dict(context=3))


@pytest.mark.parametrize("kw", [
    dict(speeds=(1.0, 1.1)), dict(mix_clips="self", mix_prob=0.5), dict(mix_clips="self", mix_targets=True),
    dict(freq_masks=1, freq_mask_width=4), dict(reassign=True), dict(drop_nyquist=True),
], ids=["speeds", "mix", "mix-targets", "masks", "reassign", "drop-nyquist"])
def test_dataset_inherits_the_refusals_of_bands(kw):
    import dataset
    clips, y = _clips()
    bank = pca_hip.mel_bank(FS, 256, 16)
    with pytest.raises(ValueError, match="out of scope"):
        dataset.ESC_wave_pc(clips, y, FS, 256, bands=bank, pcen=pca_hip.Pcen(), **kw)
    with pytest.raises(ValueError, match="out of scope"):                # no bank can be put under the spec
        dataset.ESC_wave_pc(clips, y, FS, 256, **kw).with_pcen(pca_hip.Pcen())
    with pytest.raises(ValueError, match="bands"):
        dataset.ESC_wave_pc(clips, y, FS, 256, bands=bank, pcen=pca_hip.Pcen()).with_reassign(True)


def test_pcen_sweep_is_listed():
    import evalsweep
    assert "pcen_sweep" in evalsweep.__all__
    bank = pca_hip.mel_bank(FS, 256, 16)
    with pytest.raises(ValueError, match="no specs"):
        evalsweep.pcen_sweep(None, [], [], FS, 256, bank, [])
    with pytest.raises(TypeError, match="Pcen"):
        evalsweep.pcen_sweep(None, [], [], FS, 256, bank, [dict(context=3)])
    with pytest.raises(ValueError, match="one name"):
        evalsweep.pcen_sweep(None, [], [], FS, 256, bank, {"log": pca_hip.Pcen()})


# ---- the restatement against itself -----------------------------------------------------------------------
def _noise(n, seed):
    return np.random.Generator(np.random.PCG64(seed)).normal(0, 0.1, n).astype(np.float32)


def test_restatement_without_memory_ignores_the_context():
    wave = _noise(6000, 1)
    W = pca_hip.mel_bank(FS, 128, 12).dense()
    got = [pcen_ref.slot_values(wave, 5, -9, 3, 64, 128, 128, 1.0, 128, W, 2,
                                pcen_ref.spec(context=ctx, s=1.0)) for ctx in (0, 1, 7)]
    assert got[0].shape == (3, 12) and np.isfinite(got[0]).all() and np.ptp(got[0]) > 0.0
    assert np.array_equal(got[0], got[1]) and np.array_equal(got[0], got[2])
    # with memory it does not
    mem = [pcen_ref.slot_values(wave, 5, -9, 3, 64, 128, 128, 1.0, 128, W, 2,
                                pcen_ref.spec(context=ctx, s=0.2)) for ctx in (0, 7)]
    assert not np.array_equal(mem[0], mem[1])
    # the recursion itself, on numbers small enough to do by hand: s = 1/2, gain 1, bias 0, r 1, eps 1/4
    p = pcen_ref.spec(context=1, s=0.5, gain=1.0, bias=0.0, r=1.0, eps=0.25)
    y = pcen_ref.pcen(np.array([[1.0], [3.0], [0.0]]), p)             # M = 1, 2, 1
    assert np.allclose(y[:, 0], [3.0 / 2.25, 0.0], rtol=1e-15, atol=0.0)


@pytest.mark.parametrize("power", [1, 2])
def test_restatement_reaches_the_steady_state_on_a_tone(power):
    n_fft, hop = 128, 64
    one = (0.3 * np.sin(2 * np.pi * (10.0 / n_fft) * np.arange(hop))).astype(np.float32)   # bin 10: 5 periods
    wave = np.tile(one, 125)                                          # repeats exactly every hop samples
    W = pca_hip.mel_bank(FS, n_fft, 12).dense()
    p = pcen_ref.spec(context=7, s=0.3, gain=0.8, bias=2.0, r=0.5, eps=1e-6, scale=1e3)
    centres = pcen_ref.slot_centres(len(wave), 3, 0, 3, hop, 7)
    assert min(centres) >= n_fft and max(centres) <= len(wave) - n_fft       # no reflected frame
    E = pcen_ref.energies(wave, centres, n_fft, n_fft, 1.0, n_fft, W, power)
    assert np.abs(E - E[0]).max() <= 1e-9 * E.max()                   # stationary: every frame the same sums
    y = pcen_ref.pcen(E, p)
    want = pcen_ref.steady_state(np.float64(p["scale"]) * E[0], p)
    assert y.shape == (3, 12) and np.abs(y - want).max() <= 1e-9 * np.abs(want).max()
    assert want.max() > 0.1 and want.min() >= 0.0                     # the tone's bands stand out
    # rows(): the band launch's layout, rounded once
    r = pcen_ref.rows(y, np.arange(12) / 100.0, np.arange(3) / 10.0)
    assert r.shape == (36, 3) and r.dtype == np.float32
    assert r[13].tolist() == [np.float32(0.01), np.float32(0.1), np.float32(y[1, 1])]
