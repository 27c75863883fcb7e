"""Silence trimming without a GPU: the numpy restatement (tests/trim_ref.py) on cases whose answer
follows by hand, the C ABI of pca_trim_bounds / pca_trim_ws_bytes (declared, exported, arguments
checked before any device call), and the decision margin of every waveform tests/test_gpu_trim.py
compares exactly."""
import ctypes
import math
import os
import re

import numpy as np
import pytest
import torch

from conftest import ROOT

import pca_hip
import trim_ref as tr
from pca_hip import _lib


# ---- the restatement on hand-worked cases ---------------------------------------------------------
def test_rectangular_burst_between_digital_silence():
    """y = 1 on [5000, 9000), 0 elsewhere, L = 16000; frame t (2048 / 512) is centred on t*512 and
    covers samples [t*512 - 1024, t*512 + 1024) - far enough from both ends that the reflection adds
    nothing.  A frame with k burst samples has mse = k / 2048 and the full frames set the maximum 1,
    so db = 10 log10(k / 2048).
    k >= 1 <=> t*512 + 1024 > 5000 and t*512 - 1024 < 9000 <=> 8 <= t <= 19 (k = 120 at t = 8, 296 at
    t = 19).  top_db = 60 and 30 keep every k >= 1 (k = 1 is -33.1 dB; k >= 3 clears -30 dB):
    (8 * 512, 20 * 512).  top_db = 10 needs k >= 205: t = 8 falls out (t = 9 has k = 632), t = 19 stays."""
    y = np.zeros(16000, np.float32)
    y[5000:9000] = 1.0
    mse = tr.frame_mse(y)
    assert mse.shape == (1 + 16000 // 512,)
    assert mse[8] == 120 / 2048 and mse[19] == 296 / 2048 and mse[7] == 0 and mse[20] == 0
    assert mse[12] == 1.0
    assert tr.trim_ref(y, 60) == (4096, 10240)
    assert tr.trim_ref(y, 30) == (4096, 10240)
    assert tr.trim_ref(y, 10) == (4608, 10240)
    # the silent frames sit on the amin floor: 10 log10(1e-10) - 0 = -100 dB
    assert tr.frame_db(y)[0] == -100.0


def test_all_zero_clip_is_kept_whole():
    y = np.zeros(5000, np.float32)
    assert np.all(tr.frame_db(y) == 0.0)                 # every frame equals the (floored) maximum
    assert tr.trim_ref(y, 60) == (0, 5000)
    assert tr.trim_ref(y, 1e-3) == (0, 5000)
    assert tr.trim_ref(y, 0) == (0, 0)                   # strict comparison: 0 > -0 fails everywhere


def test_clip_without_silence_is_kept_whole():
    y = tr.synth(4, 5, 25000)
    assert tr.trim_ref(y, 60) == (0, 25000)
    y = np.full(4096 + 100, 0.25, np.float32)            # last frame index 8: (8 + 1) * 512 > L
    assert tr.trim_ref(y, 60) == (0, 4196)


def test_loud_last_partial_hop_is_clamped_to_the_length():
    """L = 19207 = 37 * 512 + 263: the last frame is t = 37, centred on 18944.  Only the last 5 samples
    are loud; they lie in frames 36 (covers up to 19455) and 37, and - reflected about L - 1 - twice in
    each, so both tie for the maximum.  start = 36 * 512, end = min(L, 38 * 512) = L."""
    y = dict(tr.gpu_cases(2048, 512))["loud_tail"]
    assert y.size == 19207 and np.count_nonzero(y) == 5
    db = tr.frame_db(y)
    assert db.size == 38 and db[36] == 0.0 and db[37] == 0.0
    mse = tr.frame_mse(y)
    assert abs(mse[37] - 9 * 0.25 / 2048) < 1e-18          # 5 samples + 4 reflected (edge not repeated)
    # every other frame is digital silence: the floor, 70.4 dB below these two
    assert np.allclose(db[:36], -100.0 - 10 * math.log10(9 * 0.25 / 2048), rtol=0, atol=1e-9)
    assert tr.trim_ref(y, 60) == (18432, 19207)
    assert tr.trim_ref(y, 80) == (0, 19207)


def test_large_top_db_trims_nothing():
    for name, y in tr.gpu_cases(2048, 512):
        assert tr.trim_ref(y, 200) == (0, y.size), name     # the floor is -100 dB below full scale


def test_restatement_equals_frame_by_frame_loop():
    for fl, hop in tr.CONFIGS + ((64, 7),):
        for name, y in tr.gpu_cases(fl, hop):
            if y.size > 100000:
                y = y[690000:760000]
            yp = np.pad(y.astype(np.float64), fl // 2, mode="reflect")
            T = 1 + y.size // hop
            mse = np.array([np.mean(yp[t * hop:t * hop + fl] ** 2) for t in range(T)])
            got = tr.frame_mse(y, fl, hop)
            assert got.shape == mse.shape
            assert np.max(np.abs(got - mse)) <= 1e-14 * max(1e-300, mse.max()), (fl, hop, name)
            for top_db in tr.TOP_DBS:
                db = 10 * np.log10(np.maximum(1e-10, mse)) - 10 * np.log10(max(1e-10, mse.max()))
                first = last = None
                for t in range(T):
                    if db[t] > -top_db:
                        first = t if first is None else first
                        last = t
                want = (0, 0) if first is None else (first * hop, min(y.size, (last + 1) * hop))
                assert tr.trim_ref(y, top_db, fl, hop) == want, (fl, hop, name, top_db)


# ---- the GPU test's inputs: a condition on the inputs, not a tolerance on the kernel ---------------
MARGIN_DB = 1e-6    # fp64 sums of exact squares differ by ~1e-12 dB between summation orders


def test_every_gpu_waveform_has_a_decision_margin():
    for fl, hop in tr.CONFIGS:
        for name, y in tr.gpu_cases(fl, hop):
            assert y.dtype == np.float32 and y.size > fl // 2
            for top_db in tr.TOP_DBS:
                m = tr.decision_margin(y, top_db, fl, hop)
                assert m >= MARGIN_DB, (fl, hop, name, top_db, m)
    clips, labels = tr.sweep_clips()
    assert len(clips) == len(labels)
    for c, y in enumerate(clips):
        assert tr.decision_margin(y, 60) >= MARGIN_DB, c
        s, e = tr.trim_ref(y, 60)
        assert 0 <= s < e <= y.size and e - s > 1024 and (s > 0 or e < y.size), (c, s, e)


def test_gpu_cases_cover_the_lengths_asked_for():
    for fl, hop in tr.CONFIGS:
        cases = dict(tr.gpu_cases(fl, hop))
        assert cases["half_plus_one"].size == fl // 2 + 1
        assert cases["minute"].size > 59 * tr.FS
        assert any(y.size % hop == 0 for y in cases.values())
        assert any(y.size % hop != 0 for y in cases.values())


# ---- the C ABI ---------------------------------------------------------------------------------------
def test_header_declares_and_library_exports_the_trim_entry_points():
    txt = open(os.path.join(ROOT, "include", "pca_hip.h")).read()
    txt = re.sub(r"/\*.*?\*/", "", txt, flags=re.S)
    handle = ctypes.CDLL(_lib.LIB_PATH)
    for name in ("pca_trim_bounds", "pca_trim_ws_bytes"):
        assert re.search(r"\b%s\s*\(" % name, txt), f"{name} not declared in pca_hip.h"
        assert hasattr(handle, name), f"{name} not exported"
        assert name in _lib.SIGNATURES
    assert pca_hip.lib().pca_abi_version() == 2


def test_trim_ws_bytes():
    L = pca_hip.lib()
    # 8 clips of 220500 samples, 2048 / 512: floor(1764000 / 512) + 8 * 4 segment sums of 8 bytes
    n = L.pca_trim_ws_bytes(8 * 220500, 8, 2048, 512)
    assert n >= (1764000 // 512 + 8 * 4) * 8 and n % 256 == 0 and n < 64 * 1024
    # 2048 / 300 takes the direct form: one sum per frame
    n = L.pca_trim_ws_bytes(8 * 220500, 8, 2048, 300)
    assert (1764000 // 300 + 8) * 8 <= n < (1764000 // 300 + 8) * 8 + 256
    assert L.pca_trim_ws_bytes(1000, 1, 2047, 512) == 0
    assert L.pca_trim_ws_bytes(1000, 0, 2048, 512) == 0
    assert L.pca_trim_ws_bytes(1000, 1, 2048, 0) == 0
    assert L.pca_trim_ws_bytes(1000, 1, 16384, 512) == 0


def test_trim_bounds_refuses_bad_arguments_without_a_gpu():
    L = pca_hip.lib()
    p = 4096          # a non-null value that is never dereferenced: the checks come before any launch

    def call(waves=p, woff=p, n=2, mx=5000, mn=3000, fl=2048, hop=512, top_db=60.0, bounds=p, ws=p):
        rc = L.pca_trim_bounds(waves, woff, n, mx, mn, fl, hop, top_db, bounds, ws, None)
        return rc, L.pca_last_error()

    for kw in (dict(waves=None), dict(woff=None), dict(bounds=None), dict(ws=None)):
        rc, msg = call(**kw)
        assert rc == -1 and b"null pointer" in msg, (kw, msg)
    for n in (0, -1, 65536):
        rc, msg = call(n=n)
        assert rc == -1 and b"n_clips" in msg
    for fl in (2047, 0, 8194):
        rc, msg = call(fl=fl)
        assert rc == -1 and b"frame_length" in msg and b"even" in msg
    rc, msg = call(hop=0)
    assert rc == -1 and b"hop_length" in msg
    for mn in (1024, 0):
        rc, msg = call(mn=mn)
        assert rc == -1 and b"frame_length/2" in msg
    rc, msg = call(mx=2000)                       # longest below shortest
    assert rc == -1
    for v in (float("nan"), float("inf"), float("-inf")):
        rc, msg = call(top_db=v)
        assert rc == -1 and b"finite" in msg


def test_trim_on_cpu_tensor_raises():
    x = torch.zeros(5000)
    with pytest.raises(pca_hip.PcaHipError):
        pca_hip.trim(x, 60)
    with pytest.raises(pca_hip.PcaHipError):
        pca_hip.trim_batch([x, x])


def test_sweeps_take_trim_dB_and_default_to_none():
    import inspect

    import evalsweep
    for name in ("reframe_sweep", "reframe_sweep_temporal", "baseline_reframe_sweep",
                 "baseline_reframe_sweep_temporal"):
        p = inspect.signature(getattr(evalsweep, name)).parameters
        assert "trim_dB" in p and p["trim_dB"].default is None, name
    assert evalsweep.trim_dB_of({"trim_dB": 60}) == 60.0
    assert evalsweep.trim_dB_of({}) is None
