"""pca_frame_points_delta without a GPU: the symbol and its prototype, the entry point's host checks,
``pca_hip.Deltas``, the numpy restatement (tests/delta_ref.py) on inputs whose deltas are known in closed form,
the host side of the datasets' ``deltas=`` and ``evalsweep.delta_sweep``'s listing."""
import ctypes
import os
import re

import numpy as np
import pytest

import pca_hip
from pca_hip import _lib

import delta_ref

FS = 44100
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ---- the symbol -------------------------------------------------------------------------------------------
def test_symbol_is_declared_exported_and_bound():
    header = open(os.path.join(ROOT, "include", "pca_hip.h")).read()
    assert re.search(r"\bint pca_frame_points_delta\(", header)
    assert "typedef struct PcaDelta {" in header and "#define PCA_ABI_VERSION 2" in header
    L = pca_hip.lib()
    res, args = _lib.SIGNATURES["pca_frame_points_delta"]
    fn = L.pca_frame_points_delta                                       # AttributeError if not exported
    assert fn.restype is res is ctypes.c_int and list(fn.argtypes) == args and len(args) == 25
    # pca_frame_points' prototype with the bank, the spec, the workspace, its size and the tickets behind aug
    plain = list(_lib.SIGNATURES["pca_frame_points"][1])
    assert args == plain[:16] + [ctypes.POINTER(_lib.PcaFrameBands), ctypes.POINTER(_lib.PcaDelta),
                                 ctypes.c_void_p, ctypes.c_int64, ctypes.c_void_p] + plain[16:]
    proto = re.search(r"\bint pca_frame_points_delta\((.*?)\);", header, re.S).group(1)
    kinds = []
    for prm in proto.split(","):
        prm = " ".join(prm.split())
        kinds.append("ptr" if "*" in prm else prm.rsplit(" ", 1)[0])
    want = {ctypes.c_int: "int", ctypes.c_int64: "int64_t"}
    assert len(kinds) == 25
    for k, a in zip(kinds, args):
        assert k == want.get(a, "ptr"), (k, a)
    assert [n for n, _ in _lib.PcaDelta._fields_] == ["axes", "width"] and ctypes.sizeof(_lib.PcaDelta) == 8
    fields = re.search(r"typedef struct PcaDelta \{(.*?)\} PcaDelta;", header, re.S).group(1)
    assert re.findall(r"(int32_t|float)\s+(\w+);", fields) == [("int32_t", "axes"), ("int32_t", "width")]
    for name in ("Deltas", "frame_points_delta"):
        assert hasattr(pca_hip, name), name


# ---- the entry point's refusals ---------------------------------------------------------------------------
P = 0x1000
NAN, INF = float("nan"), float("inf")


def _call(L, bank="default", spec="default", **over):
    """pca_frame_points_delta with valid host arguments and stand-in device addresses (a refused call never
    reads them), ``over`` replacing some; ``bank`` "null": grid rows; ``spec`` "null": no spec at all."""
    aug = dict(jitter=0, gain_db=0.0, win_lengths=P, n_win=1, norm_mode=0, seed=0, draw=0, draw_dev=None)
    bk = dict(n_bands=16, nnz=227, band_lo=P, band_off=P, weights=P, power=2, amin=1e-8)
    dl = dict(axes=1, width=2)
    a = dict(waves=P, wave_off=P, set_off=P, n_clips=2, max_len=9000, min_len=3000, clip_labels=P, idx=P,
             B=4, n_fft=256, hop=128, n_bins=128, Nt=2, farr=P, tarr=P, out=P, labels_out=P, meta_out=None,
             aug="given", value_ws=P, value_ws_elems=4 * 6 * (128 if bank == "null" else 16), tickets=P)
    for k, v in over.items():
        (aug if k in aug else bk if k in bk else dl if k in dl else a)[k] = v
    s = _lib.PcaFrameAug(aug["jitter"], aug["gain_db"], aug["win_lengths"], aug["n_win"], aug["norm_mode"],
                         aug["seed"], aug["draw"], aug["draw_dev"])
    b = _lib.PcaFrameBands(bk["n_bands"], bk["nnz"], bk["band_lo"], bk["band_off"], bk["weights"],
                           bk["power"], bk["amin"])
    d = _lib.PcaDelta(dl["axes"], dl["width"])
    return L.pca_frame_points_delta(a["waves"], a["wave_off"], a["set_off"], a["n_clips"], a["max_len"],
                                    a["min_len"], a["clip_labels"], a["idx"], a["B"], a["n_fft"], a["hop"],
                                    a["n_bins"], a["Nt"], a["farr"], a["tarr"],
                                    None if a["aug"] is None else ctypes.byref(s),
                                    None if bank == "null" else ctypes.byref(b),
                                    None if spec == "null" else ctypes.byref(d), a["value_ws"],
                                    a["value_ws_elems"], a["tickets"], a["out"], a["labels_out"],
                                    a["meta_out"], None)


@pytest.mark.parametrize("bank,spec,over,word", [
    # the spec
    ("default", "null", {}, b"null pointer"),
    ("null", "null", {}, b"null pointer"),
    ("default", "default", dict(axes=0), b"axes=0"),
    ("default", "default", dict(axes=4), b"axes=4"),
    ("null", "default", dict(axes=-1), b"axes=-1"),
    ("default", "default", dict(width=0), b"width=0"),
    ("default", "default", dict(width=5, value_ws_elems=1 << 40), b"width=5"),
    ("null", "default", dict(width=-2), b"width=-2"),
    # din: a set with a time column takes one axis
    ("default", "default", dict(axes=3), b"din=5"),
    ("null", "default", dict(axes=3), b"din=5"),
    # the workspace: B = 4 slots of (2 + 2 * 2) frames of 16 bands or 128 bins
    ("default", "default", dict(value_ws_elems=4 * 6 * 16 - 1), b"workspace"),
    ("null", "default", dict(value_ws_elems=4 * 6 * 128 - 1), b"workspace"),
    ("default", "default", dict(value_ws_elems=6 * 16), b"workspace"),
    ("default", "default", dict(value_ws_elems=-1), b"workspace"),
    ("default", "default", dict(width=3), b"workspace"),
    ("default", "default", dict(value_ws=None), b"null pointer"),
    ("default", "default", dict(tickets=None), b"null pointer"),
    # what pca_frame_points rejects
    ("null", "default", dict(waves=None), b"null pointer"),
    ("null", "default", dict(wave_off=None), b"null pointer"),
    ("null", "default", dict(set_off=None), b"null pointer"),
    ("null", "default", dict(idx=None), b"null pointer"),
    ("null", "default", dict(farr=None), b"null pointer"),
    ("null", "default", dict(aug=None), b"null pointer"),
    ("null", "default", dict(out=None), b"null pointer"),
    ("null", "default", dict(win_lengths=None), b"null win_lengths"),
    ("null", "default", dict(n_bins=0), b"n_bins=0"),
    ("null", "default", dict(n_bins=130, value_ws_elems=1 << 40), b"n_bins=130"),
    ("default", "default", dict(n_bins=130), b"n_bins=130"),
    ("null", "default", dict(n_fft=384), b"n_fft=384"),
    ("null", "default", dict(n_fft=32), b"n_fft=32"),
    ("null", "default", dict(n_fft=8192), b"n_fft=8192"),
    ("null", "default", dict(hop=0), b"hop=0"),
    ("null", "default", dict(Nt=0), b"Nt=0"),
    ("null", "default", dict(B=0), b"B=0"),
    ("null", "default", dict(B=65536, value_ws_elems=1 << 40), b"B=65536"),
    ("default", "default", dict(B=65536, value_ws_elems=1 << 40), b"B=65536"),
    ("null", "default", dict(n_clips=0), b"n_clips=0"),
    ("null", "default", dict(Nt=129, value_ws_elems=1 << 40), b"points per set"),
    ("null", "default", dict(min_len=128), b"longer than n_fft/2"),
    ("null", "default", dict(max_len=2000), b"longer than n_fft/2"),
    ("null", "default", dict(max_len=1 << 31), b"int32 centres"),
    ("null", "default", dict(labels_out=None), b"go together"),
    ("null", "default", dict(clip_labels=None), b"go together"),
    ("null", "default", dict(jitter=-1), b"jitter=-1"),
    ("null", "default", dict(jitter=(1 << 30) + 1), b"jitter="),
    ("null", "default", dict(gain_db=NAN), b"gain_db"),
    ("null", "default", dict(gain_db=INF), b"gain_db"),
    ("null", "default", dict(gain_db=-1.0), b"gain_db"),
    ("null", "default", dict(n_win=0), b"n_win=0"),
    ("null", "default", dict(norm_mode=2), b"norm_mode=2"),
    # what pca_frame_points_bands adds, with a bank
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
    ("default", "default", dict(n_bands=8193, nnz=9000, value_ws_elems=1 << 40), b"points per set"),
], ids=lambda v: None if isinstance(v, bytes) else
    ("-".join(f"{k}={x}" for k, x in v.items()) if isinstance(v, dict) else v))
def test_entry_point_refuses_without_gpu(bank, spec, over, word):
    L = pca_hip.lib()
    assert _call(L, bank, spec, **over) == -1
    msg = L.pca_last_error()
    assert msg.startswith(b"frame_points_delta:") and word in msg, msg


def test_binding_refuses_before_any_tensor_is_read():
    bank = pca_hip.mel_bank(FS, 256, 16)
    kw = dict(max_len=1, min_len=1)
    with pytest.raises(TypeError, match="Deltas"):
        pca_hip.frame_points_delta(None, None, None, None, 256, 128, 129, None, deltas=dict(axes="t"), **kw)
    with pytest.raises(TypeError, match="FilterBank"):
        pca_hip.frame_points_delta(None, None, None, None, 256, 128, 129, None, deltas=pca_hip.Deltas(),
                                   bank=object(), **kw)
    with pytest.raises(ValueError, match="129 bins"):
        pca_hip.frame_points_delta(None, None, None, None, 512, 256, 257, None, deltas=pca_hip.Deltas(),
                                   bank=bank, **kw)


# ---- Deltas -----------------------------------------------------------------------------------------------
def test_deltas_is_an_immutable_checked_spec():
    d = pca_hip.Deltas()
    assert d.summary() == dict(axes="t", width=2) and (d.count, d.context) == (1, 2)
    assert (pca_hip.Deltas("f", 3).count, pca_hip.Deltas("f", 3).context) == (1, 0)
    assert (pca_hip.Deltas("tf", 4).count, pca_hip.Deltas("tf", 4).context) == (2, 4)
    with pytest.raises(AttributeError):
        d.width = 3
    assert d == pca_hip.Deltas("t", 2) and hash(d) == hash(pca_hip.Deltas("t", 2)) and d != pca_hip.Deltas("t", 1)
    for axes, code in (("t", 1), ("f", 2), ("tf", 3)):
        c = pca_hip.Deltas(axes, 4).struct()
        assert (c.axes, c.width) == (code, 4)
    for bad in (dict(axes="ft"), dict(axes=""), dict(axes="x"), dict(axes=1), dict(axes=None), dict(width=0),
                dict(width=5), dict(width=-1), dict(width=1.5), dict(width=True), dict(width=NAN)):
        with pytest.raises(ValueError, match="Deltas"):
            pca_hip.Deltas(**bad)


# ---- the restatement on inputs with known deltas ----------------------------------------------------------
@pytest.mark.parametrize("W", [1, 2, 3, 4])
def test_restatement_on_a_ramp(W):
    """v[u][m] = 3 u + 5 m: the regression slope is 3 along the frames, 5 along the rows away from the edges,
    and at the edges what replicating the first and the last row gives."""
    assert [delta_ref.divisor(w) for w in (1, 2, 3, 4)] == [2, 10, 28, 60]
    Nt, F = 3, 11
    T = Nt + 2 * W
    v = (3.0 * np.arange(T)[:, None] + 5.0 * np.arange(F)[None, :]).astype(np.float32)
    dt = delta_ref.deltas(v, Nt, "t", W)
    assert dt.shape == (Nt, F, 1) and dt.dtype == np.float32 and np.array_equal(dt, np.full((Nt, F, 1), 3.0))
    both = delta_ref.deltas(v, Nt, "tf", W)
    assert both.shape == (Nt, F, 2) and np.array_equal(both[:, :, :1], dt)
    df = delta_ref.deltas(v[:Nt], Nt, "f", W)                      # no context frames along f
    assert df.shape == (Nt, F, 1)
    assert np.array_equal(df[:, W:F - W, 0], np.full((Nt, F - 2 * W), 5.0))
    # the replicated edges, by hand: sum_n n * 5 * (min(m + n, F - 1) - max(m - n, 0)) / D
    D = delta_ref.divisor(W)
    for m in list(range(W)) + list(range(F - W, F)):
        want = sum(n * 5.0 * (min(m + n, F - 1) - max(m - n, 0)) for n in range(1, W + 1)) / D
        assert 0.0 < want < 5.0 and np.array_equal(df[:, m, 0], np.full(Nt, np.float32(want))), m
    # df of the set's own rows does not see the context frames
    assert np.array_equal(both[:, :, 1], delta_ref.deltas(v[W:W + Nt], Nt, "f", W)[:, :, 0])


@pytest.mark.parametrize("axes", ["t", "f", "tf"])
def test_restatement_on_a_constant_gives_positive_zero(axes):
    for W in (1, 4):
        Wt = delta_ref.context(axes, W)
        v = np.full((2 + 2 * Wt, 7), -18.420681, dtype=np.float32)
        d = delta_ref.deltas(v, 2, axes, W)
        assert d.shape == (2, 7, len(axes)) and not d.view(np.int32).any()       # +0.0: no bit set


def test_slot_centres_clamp_at_both_ends():
    assert delta_ref.slot_centres(1000, 0, -5, 2, 100, 2) == [0, 0, 0, 95, 195, 295]
    assert delta_ref.slot_centres(1000, 4, 7, 2, 100, 2) == [607, 707, 807, 907, 1000, 1000]
    assert delta_ref.slot_centres(1000, 3, 0, 1, 100, 0) == [300]


# ---- the datasets -----------------------------------------------------------------------------------------
def _clips():
    lens = [2205, 4851, 16170]
    return [np.zeros(n, dtype=np.float32) for n in lens], [3, 1, 4]


def test_dataset_host_side():
    import dataset
    clips, y = _clips()
    spec = pca_hip.Deltas("tf", 2)
    base = dataset.ESC_wave_pc(clips, y, FS, 256, jitter=5)
    ds = dataset.ESC_wave_pc(clips, y, FS, 256, jitter=5, deltas=spec)
    assert base.deltas is None and base.din == 2 and ds.deltas is spec and ds.din == 4
    assert (ds.F, ds.num_points, len(ds)) == (base.F, base.num_points, len(base)) == (129, 129, len(base))
    assert np.array_equal(ds.farr, base.farr) and ds.tarr is None and np.array_equal(ds.labels, base.labels)
    assert ds.stochastic and not ds.variable_length and not ds.soft_targets
    assert not dataset.ESC_wave_pc(clips, y, FS, 256, deltas=spec).stochastic           # a representation
    p = ds.plain()
    assert p.deltas is spec and p.din == 4 and not p.stochastic and p._store is ds._store
    back = ds.with_deltas(None)
    assert back.deltas is None and back.din == 2 and back._store is ds._store and back.jitter == 5
    other = base.with_deltas(pca_hip.Deltas("f", 1))
    assert other.deltas.axes == "f" and other.din == 3 and base.deltas is None and other._store is base._store
    # drop_nyquist and a bank compose; the bank's F and axis are the band dataset's
    dn = dataset.ESC_wave_pc(clips, y, FS, 256, drop_nyquist=True, deltas=pca_hip.Deltas("t", 2))
    assert (dn.F, dn.num_points, dn.din) == (128, 128, 3)
    bank = pca_hip.mel_bank(FS, 256, 16)
    band = dataset.ESC_wave_pc(clips, y, FS, 256, bands=bank)
    bd = dataset.ESC_wave_pc(clips, y, FS, 256, bands=bank, deltas=spec, win_lengths=(256, 192), norm="win")
    assert (bd.F, bd.num_points, bd.din) == (band.F, band.num_points, 4) == (16, 16, 4)
    assert np.array_equal(bd.farr, band.farr) and bd.bands is bank
    assert ds.with_bands(bank).deltas is spec and bd.with_bands(None).deltas is spec
    t = dataset.ESC_wave_pc_temp(clips, y, FS, 256, 4, bands=bank, deltas=pca_hip.Deltas("t", 4))
    t0 = dataset.ESC_wave_pc_temp(clips, y, FS, 256, 4, bands=bank)
    assert (t.F, t.num_points, t.din, t0.din) == (16, 64, 4, 3) and len(t) == len(t0)
    assert np.array_equal(t.tarr, t0.tarr) and t.plain().deltas == pca_hip.Deltas("t", 4)
    assert dataset.ESC_wave_pc_temp(clips, y, FS, 256, 4, deltas=pca_hip.Deltas("f", 1)).din == 4
    with pytest.raises(TypeError, match="Deltas"):
        dataset.ESC_wave_pc(clips, y, FS, 256, deltas=dict(axes="t"))


def test_dataset_refuses_more_than_four_columns():
    import dataset
    clips, y = _clips()
    with pytest.raises(ValueError, match="din = 5"):
        dataset.ESC_wave_pc_temp(clips, y, FS, 256, 4, deltas=pca_hip.Deltas("tf", 2))
    with pytest.raises(ValueError, match="din = 5"):
        dataset.ESC_wave_pc_temp(clips, y, FS, 256, 4).with_deltas(pca_hip.Deltas("tf", 1))
    with pytest.raises(ValueError, match="din = 5"):
        dataset.ESC_wave_pc_temp(clips, y, FS, 256, 4, bands=pca_hip.mel_bank(FS, 256, 16),
                                 deltas=pca_hip.Deltas("tf", 2))


@pytest.mark.parametrize("kw", [
    dict(speeds=(1.0, 1.1)), dict(mix_clips="self", mix_prob=0.5), dict(mix_clips="self", mix_targets=True),
    dict(freq_masks=1, freq_mask_width=4), dict(freq_masks=1, freq_mask_width=4, mask_mode="floor"),
    dict(reassign=True), dict(bands="bank", pcen=pca_hip.Pcen(context=3)),
], ids=["speeds", "mix", "mix-targets", "masks", "masks-floor", "reassign", "pcen"])
def test_dataset_refusals(kw):
    import dataset
    clips, y = _clips()
    if kw.get("bands") == "bank":
        kw = dict(kw, bands=pca_hip.mel_bank(FS, 256, 16))
    spec = pca_hip.Deltas("t", 1)
    with pytest.raises(ValueError, match="out of scope"):
        dataset.ESC_wave_pc(clips, y, FS, 256, deltas=spec, **kw)
    with pytest.raises(ValueError, match="out of scope"):
        dataset.ESC_wave_pc_temp(clips, y, FS, 256, 4, deltas=spec, **{k: v for k, v in kw.items()})
    with pytest.raises(ValueError, match="deltas"):
        dataset.ESC_wave_pc(clips, y, FS, 256, **kw).with_deltas(spec)


def test_views_of_a_delta_dataset_refuse_reassign_and_pcen():
    import dataset
    clips, y = _clips()
    bank = pca_hip.mel_bank(FS, 256, 16)
    with pytest.raises(ValueError, match="deltas"):
        dataset.ESC_wave_pc(clips, y, FS, 256, deltas=pca_hip.Deltas()).with_reassign(True)
    with pytest.raises(ValueError, match="deltas"):
        dataset.ESC_wave_pc(clips, y, FS, 256, bands=bank, deltas=pca_hip.Deltas()).with_pcen(pca_hip.Pcen())
    ds = dataset.ESC_wave_pc(clips, y, FS, 256, bands=bank, deltas=pca_hip.Deltas())
    assert ds.with_pcen(None).deltas == pca_hip.Deltas() and ds.with_reassign(None).deltas == pca_hip.Deltas()


def test_peak_points_refuses_a_delta_dataset():
    import dataset
    clips, y = _clips()
    for ds in (dataset.ESC_wave_pc(clips, y, FS, 256, deltas=pca_hip.Deltas("f", 1)),
               dataset.ESC_wave_pc_temp(clips, y, FS, 256, 4, deltas=pca_hip.Deltas("t", 1))):
        with pytest.raises(ValueError, match="PeakPoints"):
            dataset.PeakPoints(ds, 8)
        assert dataset.PeakPoints(ds.with_deltas(None), 8).din == ds.din - 1


def test_delta_sweep_is_listed():
    import evalsweep
    assert "delta_sweep" in evalsweep.__all__
    with pytest.raises(ValueError, match="no widths"):
        evalsweep.delta_sweep(None, [], [], FS, 256, [])
    with pytest.raises(ValueError, match="Deltas"):
        evalsweep.delta_sweep(None, [], [], FS, 256, [1, 5])
    with pytest.raises(ValueError, match="Deltas"):
        evalsweep.delta_sweep(None, [], [], FS, 256, [1], axes="ft")
    with pytest.raises(ValueError, match="twice"):
        evalsweep.delta_sweep(None, [], [], FS, 256, [2, 2])


def test_d128_step_promises_bits_up_to_din_3_only():
    """A delta set brings din 4 to the d = 128 step, where layer 1's fc_q gradient is added with fp32 atomics
    (k_wgrad_small): pca_st_step_reproducible must not promise bits there (tests/test_gpu_delta_dataset.py saw a
    captured and an eager run part ways)."""
    import ctypes as C
    ask = lambda din: _lib.lib().pca_st_step_reproducible(                       # noqa: E731
        C.byref(_lib.StConfig(16, 256, din, 128, 4, 16, 1, 10, _lib.MODE_BF16)), 0)
    assert [ask(din) for din in (2, 3, 4)] == [1, 1, 0]
