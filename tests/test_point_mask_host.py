"""pca_frame_points_masked without a GPU: the C ABI, the entry point's refusals, the numpy restatement of
the masks (tests/mask_ref.py) and the datasets' mask options."""
import ctypes
import os
import re

import numpy as np
import pytest

import pca_hip
from pca_hip import _lib

from mask_ref import DROP, FLOOR, mask_rows, masked_axes

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ---- the C ABI ---------------------------------------------------------------------------------------
def test_header_declares_and_library_exports_the_entry_point():
    txt = open(os.path.join(ROOT, "include", "pca_hip.h")).read()
    txt = re.sub(r"/\*.*?\*/", "", txt, flags=re.S)
    handle = ctypes.CDLL(_lib.LIB_PATH)
    name = "pca_frame_points_masked"
    assert re.search(r"\b%s\s*\(" % name, txt), f"{name} not declared in pca_hip.h"
    assert hasattr(handle, name), f"{name} not exported"
    assert name in _lib.SIGNATURES
    assert getattr(pca_hip.lib(), name).argtypes == _lib.SIGNATURES[name][1]
    assert callable(pca_hip.frame_points_masked)
    # every argument of pca_frame_points_ex_targets, then mask, lengths_out, mask_meta_out, stream
    soft = _lib.SIGNATURES["pca_frame_points_ex_targets"][1]
    new = _lib.SIGNATURES[name][1]
    assert new[:len(soft) - 1] == soft[:-1] and len(new) == len(soft) + 3
    assert new[len(soft) - 1] == ctypes.POINTER(_lib.PcaPointMask)
    assert re.search(r"#define\s+PCA_POINT_MASK_MAX\s+4\b", txt) and _lib.POINT_MASK_MAX == 4
    assert re.search(r"#define\s+PCA_ABI_VERSION\s+2\b", txt)
    assert pca_hip.lib().pca_abi_version() == 2


def test_struct_layouts():
    m = _lib.PcaPointMask
    assert ctypes.sizeof(m) == 20
    assert [n for n, _ in m._fields_] == ["n_freq", "freq_width", "n_time", "time_width", "mode"]
    assert [getattr(m, n).offset for n, _ in m._fields_] == [0, 4, 8, 12, 16]
    txt = open(os.path.join(ROOT, "include", "pca_hip.h")).read()
    body = re.search(r"typedef struct PcaPointMask \{(.*?)\} PcaPointMask;", txt, flags=re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    assert re.findall(r"int32_t\s+(\w+)\s*;", body) == [n for n, _ in m._fields_]
    # the structs before it are what they were
    assert ctypes.sizeof(_lib.PcaFrameAug) == 48
    assert ctypes.sizeof(_lib.PcaFrameAugEx) == 200


# ---- the entry point's refusals ------------------------------------------------------------------------
P = 0x1000


def _call(L, mask=(1, 8, 0, 0, 0), lengths_out=P, no_mask=False, **over):
    """pca_frame_points_masked with valid host arguments and stand-in device addresses (a refused call
    never reads them): 4 frames of 129 bins per set, every augmentation of the ex launch off."""
    a = dict(waves=P, wave_off=P, set_off=P, n_clips=2, max_len=9000, min_len=3000, clip_labels=P, idx=P,
             B=4, n_fft=256, hop=128, n_bins=129, Nt=4, farr=P, tarr=P, out=P, labels_out=P, meta_out=None,
             samples_out=None)
    a.update(over)
    s = _lib.PcaFrameAugEx(0, 0.0, P, 1, 0, 0, 0, None, 1, 0, 0, 0, (ctypes.c_double * 8)(*([1.0] * 8)),
                           None, None, None, None, None, 0, 0.0, 0.0, 0.0)
    mk = None if no_mask else ctypes.byref(_lib.PcaPointMask(*mask))
    return L.pca_frame_points_masked(a["waves"], a["wave_off"], a["set_off"], a["n_clips"], a["max_len"],
                                     a["min_len"], a["clip_labels"], a["idx"], a["B"], a["n_fft"], a["hop"],
                                     a["n_bins"], a["Nt"], a["farr"], a["tarr"], ctypes.byref(s), a["out"],
                                     a["labels_out"], a["meta_out"], a["samples_out"], None, None, None,
                                     mk, lengths_out, None, None)


@pytest.mark.parametrize("kw,word", [
    (dict(mask=(5, 8, 0, 0, 0)), b"n_freq=5"),
    (dict(mask=(-1, 8, 0, 0, 0)), b"n_freq=-1"),
    (dict(mask=(0, 0, 5, 1, 0)), b"n_time=5"),
    (dict(mask=(0, 0, -2, 1, 0)), b"n_time=-2"),
    (dict(mask=(1, -1, 0, 0, 0)), b"freq_width=-1"),
    (dict(mask=(0, 0, 1, -3, 0)), b"time_width=-3"),
    (dict(mask=(3, 43, 0, 0, 0)), b"one bin must survive"),             # 3 * 43 = 129 = n_bins
    (dict(mask=(1, 129, 0, 0, 0)), b"one bin must survive"),
    (dict(mask=(4, 200, 0, 0, 0)), b"one bin must survive"),
    (dict(mask=(0, 0, 2, 2, 0)), b"one frame must survive"),           # 2 * 2 = 4 = Nt
    (dict(mask=(0, 0, 1, 4, 0)), b"one frame must survive"),
    (dict(mask=(0, 0, 1, 1, 0), Nt=1, tarr=None), b"one frame must survive"),
    (dict(mask=(1, 8, 0, 0, 2)), b"mode=2"),
    (dict(mask=(1, 8, 0, 0, -1)), b"mode=-1"),
    (dict(mask=(1, 8, 0, 0, 0), lengths_out=None), b"drop mode needs lengths_out"),
    (dict(mask=(0, 0, 1, 1, 0), lengths_out=None), b"drop mode needs lengths_out"),
    (dict(mask=(1, 8, 1, 1, 1)), b"lengths_out must be NULL"),
    (dict(mask=(0, 0, 0, 0, 1)), b"lengths_out must be NULL"),
], ids=lambda v: None if isinstance(v, bytes) else "-".join(f"{k}={x}" for k, x in v.items()))
def test_entry_point_refuses_without_gpu(kw, word):
    L = pca_hip.lib()
    assert _call(L, **kw) == -1
    msg = L.pca_last_error()
    assert msg.startswith(b"frame_points_masked:") and word in msg, msg


def test_the_ex_launch_checks_come_first_and_keep_their_messages():
    L = pca_hip.lib()
    for kw, word in ((dict(waves=None), b"null pointer"), (dict(n_fft=384), b"power of two"),
                     (dict(B=65536), b"B=65536")):
        for no_mask in (False, True):
            assert _call(L, no_mask=no_mask, **kw) == -1
            msg = L.pca_last_error()
            assert msg.startswith(b"frame_points_ex:") and word in msg, msg


# ---- the numpy restatement ---------------------------------------------------------------------------
NB, NT = 8, 4


def _dense(din=3):
    """Point p = j * NB + f carries (f, j, 100 j + f): every row names its point."""
    j, f = np.divmod(np.arange(NB * NT), NB)
    rows = np.stack([f, j, 100 * j + f], axis=1).astype(np.float32)
    return rows if din == 3 else rows[:, [0, 2]]


def _meta(bands=(), stripes=()):
    m = np.zeros((2, 4, 2), dtype=np.int32)
    for k, iv in enumerate(bands):
        m[0, k] = iv
    for k, iv in enumerate(stripes):
        m[1, k] = iv
    return m.reshape(16)


def _points(rows, n):
    return [int(v) for v in rows[:n, -1]]


def _expect(bins_gone, frames_gone):
    return [100 * j + f for j in range(NT) if j not in frames_gone for f in range(NB) if f not in bins_gone]


@pytest.mark.parametrize("bands,stripes,bins_gone,frames_gone", [
    (((2, 3), (3, 3)), (), {2, 3, 4, 5}, set()),                        # overlapping bands: their union
    (((2, 4), (3, 1)), (), {2, 3, 4, 5}, set()),                        # one band inside another
    (((0, 2),), (), {0, 1}, set()),                                     # a band at bin 0
    (((5, 3),), (), {5, 6, 7}, set()),                                  # a band ending at n_bins
    (((4, 0), (8, 0), (0, 0)), ((4, 0),), set(), set()),               # width 0, wherever it starts
    ((), ((0, 1),), set(), {0}),                                        # a stripe on the first frame
    ((), ((3, 1),), set(), {3}),                                        # a stripe on the last frame
    ((), ((0, 2), (1, 2)), set(), {0, 1, 2}),                           # overlapping stripes
    (((6, 1), (0, 1), (3, 2)), ((2, 1),), {0, 3, 4, 6}, {2}),           # both kinds, bands out of order
], ids=["overlap", "nested", "bin0", "to-n_bins", "width0", "first-frame", "last-frame", "stripes-overlap",
        "both"])
@pytest.mark.parametrize("din", [2, 3])
def test_mask_rows(bands, stripes, bins_gone, frames_gone, din):
    dense = _dense(din)
    meta = _meta(bands, stripes)
    bins, frames = masked_axes(meta, NB, NT)
    assert set(np.nonzero(bins)[0]) == bins_gone and set(np.nonzero(frames)[0]) == frames_gone
    rows, n = mask_rows(dense, meta, NB, NT, DROP)
    want = _expect(bins_gone, frames_gone)
    assert n == len(want) == (NB - len(bins_gone)) * (NT - len(frames_gone))
    assert _points(rows, n) == want                                     # compaction in point order
    assert rows.shape == dense.shape and rows.dtype == dense.dtype
    assert (rows[n:] == 0).all()                                        # the zero tail
    # a kept frame of rank r owns rows [r * kept_bins, (r + 1) * kept_bins)
    kb = NB - len(bins_gone)
    for r, j in enumerate(j for j in range(NT) if j not in frames_gone):
        assert (rows[r * kb:(r + 1) * kb, -1] // 100 == j).all()
        if din == 3:
            assert (rows[r * kb:(r + 1) * kb, 1] == j).all()
    # floor: rows in place, coordinates kept, the value of the masked points replaced
    floored, nf = mask_rows(dense, meta, NB, NT, FLOOR, floor_value=np.float32(-18.5))
    assert nf == NB * NT
    gone = np.array([(p // NB) in frames_gone or (p % NB) in bins_gone for p in range(NB * NT)])
    assert np.array_equal(floored[:, :-1], dense[:, :-1])
    assert (floored[gone, -1] == np.float32(-18.5)).all()
    assert np.array_equal(floored[~gone], dense[~gone])


def test_mask_rows_with_everything_off_is_the_identity():
    dense = _dense()
    for mode in (DROP, FLOOR):
        rows, n = mask_rows(dense, _meta(), NB, NT, mode, floor_value=np.float32(-1.0))
        assert n == NB * NT and np.array_equal(rows, dense) and rows is not dense


# ---- the datasets ------------------------------------------------------------------------------------
def test_dataset_options_on_the_host():
    import dataset
    lens = [2205, 4851, 16170]
    clips = [np.zeros(n, dtype=np.float32) for n in lens]
    y = [3, 1, 4]
    flat = lambda **kw: dataset.ESC_wave_pc(clips, y, 44100, 64, **kw)              # noqa: E731  F = 33
    temp = lambda **kw: dataset.ESC_wave_pc_temp(clips, y, 44100, 64, 4, **kw)      # noqa: E731  F = 32
    for mk in (flat, temp):
        off = mk()
        assert not off.stochastic and not off.variable_length
        assert (off.freq_masks, off.freq_mask_width, off.time_masks, off.time_mask_width) == (0, 0, 0, 0)
        assert off.mask_mode == "drop"
        # a count without a width, or a width without a count, masks nothing
        for kw in (dict(freq_masks=2), dict(freq_mask_width=8), dict(time_mask_width=1),
                   dict(freq_masks=2, mask_mode="floor")):
            d = mk(**kw)
            assert not d.stochastic and not d.variable_length
        for mode in ("drop", "floor"):
            d = mk(freq_masks=2, freq_mask_width=8, mask_mode=mode, jitter=3)
            assert d.stochastic and d.variable_length == (mode == "drop")
            v = d.plain()
            assert not v.stochastic and not v.variable_length and v._store is d._store
            assert d.stochastic and d.variable_length == (mode == "drop")          # the view switched nothing off here
    d = temp(time_masks=1, time_mask_width=2)
    assert d.stochastic and d.variable_length and not d.plain().variable_length
    assert temp(time_masks=1, time_mask_width=3, mask_mode="floor").stochastic
    # one bin and one frame must survive
    with pytest.raises(ValueError):
        flat(freq_masks=3, freq_mask_width=11)                                      # 33 = F
    assert flat(freq_masks=4, freq_mask_width=8).variable_length                   # 32 = F - 1
    with pytest.raises(ValueError):
        temp(freq_masks=4, freq_mask_width=8)                                       # 32 = F
    assert temp(freq_masks=1, freq_mask_width=31).variable_length
    with pytest.raises(ValueError):
        temp(time_masks=2, time_mask_width=2)                                       # 4 = Ntemp
    assert temp(time_masks=3, time_mask_width=1).variable_length
    with pytest.raises(ValueError):
        flat(time_masks=1, time_mask_width=1)                                       # Nt = 1: no stripe fits
    for kw in (dict(freq_masks=5, freq_mask_width=1), dict(freq_masks=-1, freq_mask_width=1),
               dict(time_masks=5, time_mask_width=0), dict(freq_masks=1, freq_mask_width=-1),
               dict(time_masks=1, time_mask_width=-1), dict(mask_mode="zero"), dict(mask_mode=0),
               dict(freq_masks=1, freq_mask_width=4, mask_mode="Floor")):
        for mk in (flat, temp):
            with pytest.raises(ValueError):
                mk(**kw)
