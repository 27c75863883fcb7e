"""pca_frame_points_multires without a GPU: the host-side geometry of the multi-resolution datasets
(dataset.multires_layout, wave_span_offsets), the entry point's host checks, and the numpy restatement of a
slot (tests/multires_ref.py) against the STFT oracle on the regular grid."""
import ctypes

import numpy as np
import pytest

import pca_hip
from pca_hip import _lib

from multires_ref import multires_ref
from oracle import st_oracle as orc

FS = 44100


# ---- layout -----------------------------------------------------------------------------------------------
def test_layout_two_levels():
    import dataset
    lay = dataset.multires_layout(FS, [dict(n_fft=256, hop=128, Ntemp=2), dict(n_fft=64, hop=32, Ntemp=8)], 256)
    assert lay["point_off"] == [0, 256] and lay["N"] == 512
    assert lay["F"] == [128, 32] and lay["Ntemp"] == [2, 8] and lay["hop"] == [128, 32]
    assert lay["offset"] == [0, 0] and lay["win_lengths"] == [(256,), (64,)]
    # the defaults: hop = n_fft / 2, Ntemp = span / hop, Nyquist dropped
    same = dataset.multires_layout(FS, [dict(n_fft=256), dict(n_fft=64)], 256)
    assert same["point_off"] == [0, 256] and same["N"] == 512 and same["Ntemp"] == [2, 8]
    for r, F in enumerate((128, 32)):
        assert np.array_equal(lay["farr"][r], np.linspace(0, FS / 2, F) / FS)
    # true frame times, one clock for both levels: frame j at j * hop samples from the anchor
    assert np.array_equal(lay["tarr"][0], np.array([0, 128]) / FS)
    assert np.array_equal(lay["tarr"][1], np.arange(8) * 32 / FS)
    assert lay["tarr"][0][1] == lay["tarr"][1][4]                        # the same instant, the same number
    assert lay["tarr"][1][7] != np.linspace(0, 32 / FS * 8, 8)[7]        # not the reference's stretched axis


def test_layout_three_levels_odd_offset_and_tarr_with_offsets():
    import dataset
    levels = [dict(n_fft=64, hop=32, Ntemp=5, drop_nyquist=False, offset=-64),
              dict(n_fft=256, hop=128, Ntemp=2, win_lengths=(256, 200)),
              dict(n_fft=128, offset=32, win_lengths=(128, 96))]
    with pytest.raises(ValueError, match="win_lengths"):                 # 1, 2 and 2 windows
        dataset.multires_layout(FS, levels, 256)
    levels[0]["win_lengths"] = (64, 48)
    lay = dataset.multires_layout(FS, levels, 256)
    assert lay["F"] == [33, 128, 64] and lay["Ntemp"] == [5, 2, 4]
    assert lay["point_off"] == [0, 165, 421] and lay["N"] == 677         # level 1 starts at an odd point
    assert np.array_equal(lay["tarr"][0], (-64 + 32 * np.arange(5)) / FS)
    assert np.array_equal(lay["tarr"][2], (32 + 64 * np.arange(4)) / FS)
    assert np.array_equal(lay["farr"][0], np.linspace(0, FS / 2, 33) / FS)
    # 2-D rows: no time axis, one frame per level
    flat = dataset.multires_layout(FS, [dict(n_fft=256, Ntemp=1), dict(n_fft=64, Ntemp=1)], 256, time_axis=False)
    assert flat["tarr"] == [None, None] and flat["N"] == 160 and flat["point_off"] == [0, 128]


def test_span_offsets():
    import dataset
    assert dataset.wave_span_offsets([2205, 4851, 16170, 22050], 256) == [0, 8, 26, 89, 175]
    assert dataset.wave_span_offsets([255, 256, 257], 256) == [0, 0, 1, 2]


@pytest.mark.parametrize("levels,span,kw,word", [
    ([], 256, {}, "levels"),
    ([dict(n_fft=64)] * 5, 256, {}, "levels"),
    ([dict(n_fft=256), dict(n_fft=64)], 100, {}, "Ntemp"),               # 100 // 128 = 0
    ([dict(n_fft=256, win_lengths=(256, 128)), dict(n_fft=64)], 256, {}, "win_lengths"),
    ([dict(n_fft=256), dict(n_fft=64, Ntemp=1)], 256, dict(time_axis=False), "time_axis"),
    ([dict(n_fft=4096, hop=64, Ntemp=9)], 1024, {}, "points per set"),   # 9 * 2048 = 18432
    ([dict(n_fft=96)], 256, {}, "power of two"),
    ([dict(n_fft=64, offset=(1 << 30) + 1)], 256, {}, "offset"),
    ([dict(n_fft=64, win_lengths=(65,))], 256, {}, "win_lengths"),
    ([dict(n_fft=64)], 0, {}, "span"),
    ([dict(n_fft=64, window=3)], 256, {}, "level 0"),
], ids=["0-levels", "5-levels", "Ntemp-0", "win-counts", "2d-Ntemp", "N-max", "n_fft", "offset", "win-range",
        "span", "unknown-key"])
def test_layout_refuses(levels, span, kw, word):
    import dataset
    with pytest.raises(ValueError, match=word):
        dataset.multires_layout(FS, levels, span, **kw)


def test_dataset_host_side():
    import dataset
    lens = [2205, 4851, 16170, 22050]
    clips = [np.zeros(n, dtype=np.float32) for n in lens]
    y = [3, 1, 4, 1]
    levels = [dict(n_fft=256, win_lengths=(256, 200)), dict(n_fft=64, win_lengths=(64, 48))]
    ds = dataset.ESC_wave_pc_multires(clips, y, FS, levels, 256)
    assert len(ds) == 175 and ds.set_off == [0, 8, 26, 89, 175] and ds.num_points == 512
    assert np.array_equal(ds.labels, np.repeat(y, [8, 18, 63, 86]))
    assert ds.batch_seq is None and not ds.variable_length and not ds.soft_targets
    assert ds.stochastic                                                 # two windows
    p = ds.plain()
    assert not p.stochastic and p.layout["win_lengths"] == [(256,), (64,)] and p._store is ds._store
    assert ds.plain(1).layout["win_lengths"] == [(200,), (48,)]
    with pytest.raises(ValueError):
        ds.plain(2)
    one = dataset.ESC_wave_pc_multires(clips, y, FS, [dict(n_fft=256), dict(n_fft=64)], 256)
    assert not one.stochastic
    for kw in (dict(jitter=1), dict(gain_db=0.5)):
        assert dataset.ESC_wave_pc_multires(clips, y, FS, [dict(n_fft=64)], 256, **kw).stochastic
    v = ds.with_levels([1])
    assert v.num_points == 256 and v.layout["point_off"] == [0] and v.layout["n_fft"] == [64]
    assert len(v) == len(ds) and v._store is ds._store and v.stochastic
    assert ds.with_levels([1, 0]).layout["point_off"] == [0, 256]
    assert ds.with_levels([1, 0]).with_levels([1]).layout["n_fft"] == [256]
    for bad in ([], [2], [0, 0]):
        with pytest.raises(ValueError):
            ds.with_levels(bad)
    with pytest.raises(ValueError, match="shortest clip"):
        dataset.ESC_wave_pc_multires(clips[:1] + [np.zeros(128, dtype=np.float32)], y[:2], FS, levels, 256)

    with pytest.raises(ValueError, match="norm"):
        dataset.ESC_wave_pc_multires(clips, y, FS, levels, 256, norm="hop")
    # PeakPoints reads one F x Nt grid
    with pytest.raises(ValueError, match="multi-resolution"):
        dataset.PeakPoints(ds, 8)


# ---- the entry point's refusals ---------------------------------------------------------------------------
P = 0x1000


def _level(**over):
    a = dict(n_fft=256, hop=128, n_bins=128, Nt=2, offset=0, farr=P, tarr=P, win_lengths=P)
    a.update(over)
    return a


def _call(L, levels=None, **over):
    """pca_frame_points_multires with valid host arguments and stand-in device addresses (a refused call
    never reads them), ``over`` replacing some; ``levels``: a list of _level(...) dicts, or "null"."""
    aug = dict(jitter=0, gain_db=0.0, n_win=1, norm_mode=0, seed=0, draw=0, draw_dev=None)
    a = dict(waves=P, wave_off=P, set_off=P, n_clips=2, max_len=9000, min_len=3000, clip_labels=P, idx=P,
             B=4, n_levels=None, span=256, out=P, labels_out=P, meta_out=None)
    for k, v in over.items():
        (aug if k in aug else a)[k] = v
    if levels is None:
        levels = [_level(), _level(n_fft=64, hop=32, n_bins=32, Nt=8)]
    arr = None
    if levels != "null":
        arr = (_lib.PcaFrameLevel * max(len(levels), 1))()
        for dst, lv in zip(arr, levels):
            for k, v in lv.items():
                setattr(dst, k, v)
    n_levels = a["n_levels"] if a["n_levels"] is not None else (2 if levels == "null" else len(levels))
    s = _lib.PcaFrameAug(aug["jitter"], aug["gain_db"], None, aug["n_win"], aug["norm_mode"], aug["seed"],
                         aug["draw"], aug["draw_dev"])
    return L.pca_frame_points_multires(a["waves"], a["wave_off"], a["set_off"], a["n_clips"], a["max_len"],
                                       a["min_len"], a["clip_labels"], a["idx"], a["B"], arr, n_levels,
                                       a["span"], ctypes.byref(s), a["out"], a["labels_out"], a["meta_out"],
                                       None)


@pytest.mark.parametrize("levels,over,word", [
    ("null", {}, b"null pointer"),
    (None, dict(waves=None), b"null pointer"),
    (None, dict(idx=None), b"null pointer"),
    (None, dict(n_levels=0), b"n_levels=0"),
    ([_level(n_fft=64, hop=32, n_bins=32, Nt=1)] * 4, dict(n_levels=5), b"n_levels=5"),
    ([_level(), _level(n_fft=384)], {}, b"level 1 n_fft=384"),
    ([_level(n_fft=8192)], {}, b"level 0 n_fft=8192"),
    ([_level(n_bins=130)], {}, b"level 0 n_bins=130"),
    ([_level(hop=0)], {}, b"level 0 hop=0"),
    ([_level(Nt=0)], {}, b"level 0 Nt=0"),
    ([_level(), _level(n_fft=64, hop=32, n_bins=32, Nt=8, tarr=None)], {}, b"tarr"),
    ([_level(tarr=None), _level(n_fft=64, hop=32, n_bins=32, Nt=8)], {}, b"tarr"),
    (None, dict(span=0), b"span=0"),
    (None, dict(span=(1 << 30) + 1), b"span=1073741825"),
    ([_level(offset=(1 << 30) + 1)], {}, b"offset=1073741825"),
    ([_level(offset=-(1 << 30) - 1)], {}, b"offset=-1073741825"),
    ([_level(), _level(n_fft=1024, hop=512, n_bins=512, Nt=1)], dict(min_len=512), b"longer than n_fft/2"),
    (None, dict(min_len=128), b"longer than n_fft/2"),
    ([_level(n_fft=1024, hop=512, n_bins=513, Nt=16)] * 2, {}, b"points per set"),      # 2 * 8208 = 16416
    ([_level(), _level(win_lengths=None)], {}, b"level 1 null win_lengths"),
    ([_level(farr=None)], {}, b"level 0 null farr"),
    (None, dict(labels_out=None), b"go together"),
    (None, dict(jitter=-1), b"jitter=-1"),
    (None, dict(jitter=(1 << 30) + 1), b"jitter="),
    (None, dict(gain_db=float("nan")), b"gain_db"),
    (None, dict(gain_db=float("inf")), b"gain_db"),
    (None, dict(gain_db=-1.0), b"gain_db"),
    (None, dict(n_win=0), b"n_win=0"),
    (None, dict(norm_mode=2), b"norm_mode=2"),
    (None, dict(B=65536), b"B=65536"),
    (None, dict(B=0), b"B=0"),
    (None, dict(max_len=1 << 31), b"int32 centres"),
], ids=lambda v: None if isinstance(v, bytes) else
    (v if isinstance(v, str) else "-".join(f"{k}={x}" for k, x in v.items()) if isinstance(v, dict) else None))
def test_entry_point_refuses_without_gpu(levels, over, word):
    L = pca_hip.lib()
    assert _call(L, levels, **over) == -1
    msg = L.pca_last_error()
    assert msg.startswith(b"frame_points_multires:") and word in msg, msg


def test_binding_refuses_before_any_tensor_is_read():
    """What the Python binding itself checks: the number of levels, tarr in all or none."""
    lv = pca_hip.FrameLevel(64, 32, 32, 1, None)
    assert lv.tarr is None and lv.win_lengths is None and lv.offset == 0
    with pytest.raises(ValueError, match="levels"):
        pca_hip.frame_points_multires(None, None, None, None, [], 256, max_len=1, min_len=1)
    with pytest.raises(ValueError, match="levels"):
        pca_hip.frame_points_multires(None, None, None, None, [lv] * 5, 256, max_len=1, min_len=1)


def test_sweep_default_subsets():
    import evalsweep
    assert "multires_sweep" in evalsweep.__all__
    assert evalsweep.default_level_subsets(1) == [(0,)]
    assert evalsweep.default_level_subsets(2) == [(0,), (1,)]
    assert evalsweep.default_level_subsets(3) == [(0,), (1,), (2,), (1, 2), (0, 2), (0, 1)]
    assert len(evalsweep.default_level_subsets(4)) == 8


# ---- the numpy restatement --------------------------------------------------------------------------------
@pytest.mark.parametrize("n_fft,win", [(64, 64), (256, 200), (1024, 1024)])
def test_multires_ref_on_the_grid_is_the_stft_oracle(n_fft, win):
    wave = orc.synth_clip(3, 7, seconds=0.1)
    hop = n_fft // 2
    want = orc.stft_logmag(wave, n_fft, win, hop)                       # [F, T]
    F, T = want.shape
    assert T == 1 + len(wave) // hop and T >= 5
    Nt = 2
    farr = np.linspace(0, FS / 2, F) / FS
    tarr = np.arange(Nt) * hop / FS
    level = dict(n_fft=n_fft, hop=hop, n_bins=F, Nt=Nt, offset=0, farr=farr, tarr=tarr, win_lengths=[17, win])
    for s in range(T // Nt):                                            # sets of Nt frames, span = Nt * hop
        got = multires_ref(wave, s, 0, 1.0, 1, [level], Nt * hop)
        assert got.shape == (Nt * F, 3) and got.dtype == np.float32
        assert np.array_equal(got[:, 2].reshape(Nt, F).T, want[:, s * Nt:(s + 1) * Nt]), s
        assert np.array_equal(got[:, 0], np.tile(farr.astype(np.float32), Nt))
        assert np.array_equal(got[:, 1], np.repeat(tarr.astype(np.float32), F))
    # 2-D rows, fewer bins (the dropped Nyquist bin), and an offset of one hop = the next frame
    flat = dict(level, n_bins=F - 1, Nt=1, tarr=None, offset=hop)
    got = multires_ref(wave, 1, 0, 1.0, 1, [flat], Nt * hop)
    assert got.shape == (F - 1, 2) and np.array_equal(got[:, 1], want[:-1, 3])
    # two levels lie back to back in the order given
    both = multires_ref(wave, 1, 0, 1.0, 1, [dict(flat, tarr=tarr), level], Nt * hop)
    assert both.shape == (F - 1 + Nt * F, 3)
    assert np.array_equal(both[F - 1:], multires_ref(wave, 1, 0, 1.0, 1, [level], Nt * hop))
