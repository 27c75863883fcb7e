"""pca_frame_points_reassigned without a GPU: the numpy restatement (tests/reassign_ref.py) pinned by
physics - a click collapses onto its time, a stationary partial onto its frequency, a chirp onto its
instantaneous-frequency line - and the entry point's host checks."""
import ctypes

import numpy as np
import pytest

import pca_hip
from pca_hip import _lib

import reassign_ref
from frame_ref import frame_ref

LOG10 = np.float32(np.log(10.0))


@pytest.mark.parametrize("n_fft,win", [(256, 256), (256, 200), (1024, 1024)])
def test_an_impulse_collapses_onto_its_sample_in_every_bin(n_fft, win):
    """X_h[k] = h[n] e^{-i w n}, X_dh and X_th are dh[n] / h[n] and (n - n_fft/2) times it: real ratios, so
    db = 0 and the reassigned time is the impulse's sample, up to rounding (measured: 1.5e-13 samples,
    3e-16 bins).  Bars 1e-9."""
    hop, n0 = n_fft // 2, 1700
    wave = np.zeros(4000, dtype=np.float32)
    wave[n0] = 1.0
    for centre in (n0 - win // 5, n0 + win // 3, n0):
        db, dt, p = reassign_ref.shifts(wave, centre, n_fft, win, 1.0, hop, n_fft // 2 + 1)
        assert (p > 0).all()
        et, eb = np.abs(centre + dt * hop - n0).max(), np.abs(db).max()
        print(f"impulse n_fft {n_fft} win {win} centre {centre}: |t - n0| {et:.2e} samples, |db| {eb:.2e}")
        assert et <= 1e-9 and eb <= 1e-9


@pytest.mark.parametrize("n_fft,win", [(256, 256), (256, 200), (1024, 1024), (256, 201), (1024, 999)])
def test_a_cosine_collapses_onto_its_frequency(n_fft, win):
    """Every bin within log(10) of the frame's maximum lands within 1e-3 bin of the true frequency (measured
    <= 1e-4 at the even cases, 4e-4 at (256, 201): the negative-frequency image is what is left).  The raw
    bins are up to 1.4 bins off.  The time shift is the window's centre of gravity against n_fft/2: 0 with
    n_fft - w even, -1/2 sample with it odd (lpad rounds down), to 1e-3 sample (measured 5e-6)."""
    k0 = n_fft / 4 + 0.37
    n = np.arange(6000, dtype=np.float64)
    wave = np.cos(2.0 * np.pi * k0 / n_fft * n + 0.3).astype(np.float32)
    hop, F, centre = n_fft // 2, n_fft // 2 + 1, 3000
    v = frame_ref(wave, centre, n_fft, win, 1.0, n_fft, F)
    db, dt, _ = reassign_ref.shifts(wave, centre, n_fft, win, 1.0, hop, F)
    ok = v >= v.max() - LOG10
    bins = np.flatnonzero(ok)
    assert bins.size >= 3 and np.abs(bins - k0).max() > 1.0
    err = np.abs(bins + db[ok] - k0).max()
    want_dt = -0.5 if (n_fft - win) % 2 else 0.0
    err_t = np.abs(dt[ok] * hop - want_dt).max()
    print(f"cosine n_fft {n_fft} win {win}: {bins.size} bins, |f - f0| {err:.2e} bins, "
          f"|dt hop - {want_dt}| {err_t:.2e} samples")
    assert err <= 1e-3 and err_t <= 1e-3
    # the same through the coordinate rules: farr in cycles per sample, the clamp wide enough
    farr = (np.arange(F) / n_fft).astype(np.float32)
    f, t, moved, sdb = reassign_ref.reassign_frame(wave, centre, n_fft, win, 1.0, hop, v, farr, None, 0,
                                                   axes="f", rel_floor=LOG10, max_df=2.0)
    assert t is None and np.array_equal(moved, ok) and np.array_equal(f[~ok], farr[~ok])
    assert np.abs(f[ok].astype(np.float64) * n_fft - k0).max() <= 1e-3 + n_fft * 2.0 ** -25


@pytest.mark.parametrize("n_fft", [256, 512, 1024])
def test_a_linear_chirp_lands_on_its_instantaneous_frequency_line(n_fft):
    """0.2 -> 0.25 cycles per sample over 6000 samples: (t, f) of every bin within log(10) of its frame's
    maximum satisfies f = f_inst(t) to 1e-2 bin (measured 5e-4 / 7e-5 / 3e-5 bins at n_fft 256 / 512 / 1024:
    for a linear chirp the reassigned point lies on the line whatever the window, the residue is the
    negative-frequency image and the edges of the window)."""
    n = np.arange(6000, dtype=np.float64)
    rate = 0.05 / 6000
    wave = np.cos(2.0 * np.pi * (0.2 * n + 0.5 * rate * n * n)).astype(np.float32)
    hop, F, worst = n_fft // 2, n_fft // 2 + 1, 0.0
    for centre in range(1024, 5000, hop):
        v = frame_ref(wave, centre, n_fft, n_fft, 1.0, n_fft, F)
        db, dt, _ = reassign_ref.shifts(wave, centre, n_fft, n_fft, 1.0, hop, F)
        ok = v >= v.max() - LOG10
        f_hat = np.flatnonzero(ok) + db[ok]
        t_hat = centre + dt[ok] * hop
        worst = max(worst, float(np.abs(f_hat - (0.2 + rate * t_hat) * n_fft).max()))
    print(f"chirp n_fft {n_fft}: |f - f_inst(t)| {worst:.2e} bins")
    assert worst <= 1e-2


def test_restatement_rules_on_a_hand_made_frame():
    """Floors, clamps, strength and the exact-zero rule of the coordinate step."""
    n_fft, hop, F = 64, 32, 33
    rng = np.random.default_rng(3)
    wave = rng.normal(0, 0.1, 2000).astype(np.float32)
    wave += np.cos(2 * np.pi * 0.2031 * np.arange(2000)).astype(np.float32)
    v = frame_ref(wave, 640, n_fft, n_fft, 1.0, n_fft, F)
    farr = np.linspace(0, 0.5, F).astype(np.float32)
    tarr = np.linspace(0, 0.01, 4).astype(np.float32)
    kw = dict(rel_floor=np.inf, max_df=0.25, max_dt=0.5)
    f, t, ok, sdb = reassign_ref.reassign_frame(wave, 640, n_fft, n_fft, 1.0, hop, v, farr, tarr, 0,
                                                axes="ft", **kw)
    assert ok.all() and np.abs(sdb).max() == 0.25 and (np.abs(sdb) == 0.25).sum() > 3
    assert f.min() >= farr[0] and f.max() <= farr[-1] and np.isfinite(t).all()
    assert t.min() >= np.float32(-0.5 * float(tarr[1])) and t.min() < 0       # extrapolated before tarr[0]
    f0, t0, _, s0 = reassign_ref.reassign_frame(wave, 640, n_fft, n_fft, 1.0, hop, v, farr, tarr, 2,
                                                axes="ft", strength=0.0, **kw)
    assert np.array_equal(f0, farr) and np.array_equal(t0, np.full(F, tarr[2])) and not s0.any()
    f1, t1, _, _ = reassign_ref.reassign_frame(wave, 640, n_fft, n_fft, 1.0, hop, v, farr, tarr, 2,
                                               axes="f", **kw)
    assert np.array_equal(t1, np.full(F, tarr[2])) and not np.array_equal(f1, farr)
    _, _, ok2, _ = reassign_ref.reassign_frame(wave, 640, n_fft, n_fft, 1.0, hop, v, farr, tarr, 2,
                                               axes="ft", rel_floor=1.0)
    assert np.array_equal(ok2, v >= v.max() - np.float32(1.0)) and 0 < ok2.sum() < F
    # a frame of zeros: p = 0 everywhere, nothing moves
    z = np.zeros(2000, dtype=np.float32)
    vz = frame_ref(z, 640, n_fft, n_fft, 1.0, n_fft, F)
    fz, tz, okz, _ = reassign_ref.reassign_frame(z, 640, n_fft, n_fft, 1.0, hop, vz, farr, tarr, 1,
                                                 axes="ft", **kw)
    assert not okz.any() and np.array_equal(fz, farr) and np.array_equal(tz, np.full(F, tarr[1]))


# ---- the C ABI ------------------------------------------------------------------------------------------
def test_symbol_is_exported_with_its_prototype():
    L = pca_hip.lib()
    fn = L.pca_frame_points_reassigned
    assert fn.restype is ctypes.c_int and len(fn.argtypes) == 21
    assert ctypes.sizeof(_lib.PcaReassignSpec) == 24
    assert callable(pca_hip.frame_points_reassigned)


def _call(L, **over):
    """pca_frame_points_reassigned with valid host arguments and stand-in device addresses (a refused call
    never reads them), ``over`` replacing some; spec=None passes a NULL spec."""
    P = 0x1000
    aug = dict(jitter=0, gain_db=0.0, win_lengths=P, n_win=1, norm_mode=0, seed=0, draw=0,
               draw_dev=None)
    spec = dict(axes=1, rel_floor=6.9, abs_floor=-np.inf, max_df=2.0, max_dt=1.0, strength=1.0)
    a = dict(waves=P, wave_off=P, set_off=P, n_clips=2, max_len=9000, min_len=3000, clip_labels=P,
             idx=P, B=4, n_fft=256, hop=128, n_bins=129, Nt=1, farr=P, tarr=None, out=P,
             labels_out=P, meta_out=None, spec=True)
    for k, v in over.items():
        (aug if k in aug else spec if k in spec else a)[k] = v
    s = _lib.PcaFrameAug(aug["jitter"], aug["gain_db"], aug["win_lengths"], aug["n_win"],
                         aug["norm_mode"], aug["seed"], aug["draw"], aug["draw_dev"])
    r = _lib.PcaReassignSpec(spec["axes"], spec["rel_floor"], spec["abs_floor"], spec["max_df"],
                             spec["max_dt"], spec["strength"])
    return L.pca_frame_points_reassigned(
        a["waves"], a["wave_off"], a["set_off"], a["n_clips"], a["max_len"], a["min_len"],
        a["clip_labels"], a["idx"], a["B"], a["n_fft"], a["hop"], a["n_bins"], a["Nt"], a["farr"],
        a["tarr"], ctypes.byref(s), ctypes.byref(r) if a["spec"] else None, a["out"], a["labels_out"],
        a["meta_out"], None)


NAN, INF = float("nan"), float("inf")


@pytest.mark.parametrize("over,word", [
    # every refusal of pca_frame_points
    (dict(waves=None), b"null pointer"),
    (dict(idx=None), b"null pointer"),
    (dict(win_lengths=None), b"win_lengths"),
    (dict(labels_out=None), b"go together"),
    (dict(n_clips=0), b"n_clips=0"),
    (dict(n_fft=384), b"power of two"),
    (dict(n_fft=32, n_bins=17), b"power of two"),
    (dict(n_fft=8192, n_bins=129), b"power of two"),
    (dict(min_len=128), b"longer than n_fft/2"),
    (dict(max_len=1 << 31), b"int32 centres"),
    (dict(jitter=-1), b"jitter=-1"),
    (dict(gain_db=NAN), b"gain_db"),
    (dict(gain_db=INF), b"gain_db"),
    (dict(gain_db=-1.0), b"gain_db"),
    (dict(n_win=0), b"n_win=0"),
    (dict(norm_mode=2), b"norm_mode=2"),
    (dict(Nt=128, tarr=0x1000), b"points per set"),
    (dict(B=65536), b"B=65536"),
    (dict(B=0), b"B=0"),
    (dict(hop=0), b"hop=0"),
    (dict(n_bins=130), b"n_bins=130"),
    # its own
    (dict(spec=False), b"null spec"),
    (dict(axes=0), b"axes=0"),
    (dict(axes=4), b"axes=4"),
    (dict(axes=2), b"time axis"),                                  # bit 1 without tarr
    (dict(axes=3, tarr=0x1000, Nt=1), b"time axis"),               # bit 1 with Nt < 2
    (dict(n_bins=1), b"n_bins=1"),
    (dict(rel_floor=NAN), b"rel_floor"),
    (dict(rel_floor=-0.5), b"rel_floor"),
    (dict(abs_floor=NAN), b"abs_floor"),
    (dict(max_df=NAN), b"max_df"),
    (dict(max_df=0.0), b"max_df"),
    (dict(max_df=64.5), b"max_df"),
    (dict(max_df=INF), b"max_df"),
    (dict(max_dt=NAN), b"max_dt"),
    (dict(max_dt=0.0), b"max_dt"),
    (dict(max_dt=4.5), b"max_dt"),
    (dict(strength=NAN), b"strength"),
    (dict(strength=-0.1), b"strength"),
    (dict(strength=1.5), b"strength"),
], ids=lambda v: None if isinstance(v, bytes) else "-".join(f"{k}={x}" for k, x in v.items()))
def test_entry_point_refuses_without_gpu(over, word):
    L = pca_hip.lib()
    assert _call(L, **over) == -1
    msg = L.pca_last_error()
    assert msg.startswith(b"frame_points_reassigned:") and word in msg, msg


def test_binding_and_datasets_refuse_on_the_host():
    """ValueError before any launch: no tensor is touched."""
    import dataset
    for kw in (dict(axes="x"), dict(rel_floor=-1.0), dict(rel_floor=NAN), dict(abs_floor=NAN),
               dict(max_df=0.0), dict(max_df=65.0), dict(max_dt=5.0), dict(strength=2.0),
               dict(strength=NAN)):
        with pytest.raises(ValueError):
            pca_hip.ops.reassign_spec(**kw)
        with pytest.raises(ValueError):
            pca_hip.frame_points_reassigned(None, None, None, None, 256, 128, 129, None, max_len=9000,
                                            min_len=3000, **kw)
    with pytest.raises(ValueError):                                 # the time axis without tarr
        pca_hip.frame_points_reassigned(None, None, None, None, 256, 128, 129, None, max_len=9000,
                                        min_len=3000, axes="ft")
    with pytest.raises(ValueError):
        pca_hip.frame_points_reassigned(None, None, None, None, 256, 128, 1, None, max_len=9000,
                                        min_len=3000)
    s = pca_hip.ops.reassign_spec()
    assert (s.axes, s.max_df, s.max_dt, s.strength) == (1, 2.0, 1.0, 1.0)
    assert s.rel_floor == np.float32(np.log(1e3)) and s.abs_floor == -INF

    clips = [np.zeros(n, dtype=np.float32) for n in (2205, 4851)]
    y = [3, 1]
    d2 = dataset.ESC_wave_pc(clips, y, 44100, 64, reassign=True)
    assert d2.reassign == dict(axes="f", rel_floor=np.log(1e3), abs_floor=-INF, max_df=2.0, max_dt=1.0,
                               strength=1.0)
    assert not d2.stochastic and not d2.variable_length and d2.num_points == 33
    d3 = dataset.ESC_wave_pc_temp(clips, y, 44100, 64, 4, jitter=3, reassign=dict(max_df=1.0))
    assert d3.reassign["axes"] == "ft" and d3.reassign["max_df"] == 1.0 and d3.stochastic
    assert d3.plain().reassign == d3.reassign and not d3.plain().stochastic
    assert d3.with_reassign(None).reassign is None and d3.with_reassign(None)._store is d3._store
    assert dataset.ESC_wave_pc(clips, y, 44100, 64).reassign is None
    assert dataset.ESC_wave_pc(clips, y, 44100, 64).with_reassign(True).reassign == d2.reassign
    for kw in (dict(speeds=(1.0, 1.1)), dict(mix_clips="self", mix_prob=0.5),
               dict(mix_clips="self", mix_targets=True), dict(freq_masks=1, freq_mask_width=4),
               dict(freq_masks=1, freq_mask_width=4, mask_mode="floor")):
        with pytest.raises(ValueError, match="reassign"):
            dataset.ESC_wave_pc(clips, y, 44100, 64, reassign=True, **kw)
        with pytest.raises(ValueError, match="reassign"):
            dataset.ESC_wave_pc(clips, y, 44100, 64, **kw).with_reassign(True)
    with pytest.raises(ValueError):
        dataset.ESC_wave_pc(clips, y, 44100, 64, reassign=dict(axes="ft"))       # 2-D sets carry no time
    with pytest.raises(ValueError):
        dataset.ESC_wave_pc(clips, y, 44100, 64, reassign=dict(radius=3))
    with pytest.raises(ValueError):
        dataset.ESC_wave_pc_temp(clips, y, 44100, 64, 4, reassign=dict(strength=1.5))
