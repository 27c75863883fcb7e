"""pca_peak_points without a GPU: the numpy restatement (tests/peak_ref.py) on sinusoids and hand-made
rows, and the entry point's argument validation."""
import ctypes

import numpy as np
import pytest

import pca_hip
from pca_hip import _lib

import peak_ref

N_FFT = 1024


def _sinusoid_logmag(k_true, phase):
    """One frame of cos(2 pi k_true n / n_fft + phase), n_fft = win = 1024, periodic Hann,
    log(1e-8 + |.| / n_fft) in fp32: the 513 bins."""
    n = np.arange(N_FFT, dtype=np.float64)
    win = 0.5 - 0.5 * np.cos(2.0 * np.pi * n / N_FFT)
    x = np.cos(2.0 * np.pi * k_true * n / N_FFT + phase)
    mag = np.abs(np.fft.rfft(x * win)).astype(np.float32)
    return np.log(np.float32(1e-8) + mag / np.float32(N_FFT)).astype(np.float32)


def test_refined_frequency_of_a_sinusoid_is_within_a_fiftieth_of_a_bin():
    """The bar, 0.02 bin, is a condition: the parabola through the log-magnitudes of a Hann main lobe is off
    by 0.016 bin at the worst offset, and the fp32 log adds a little.  The raw bin centre is off by up to half
    a bin, so an unrefined output fails."""
    F = N_FFT // 2 + 1
    bins = np.arange(F, dtype=np.float32)
    worst, raw_off, cases = 0.0, 0, 0
    for k0 in (20, 100, 300):
        for off in np.linspace(-0.5, 0.5, 41):
            for phase in (0.0, 1.0, 2.5):
                v = _sinusoid_logmag(k0 + off, phase)
                X = np.stack((bins, v), axis=1)[None]
                r = peak_ref.peak_points(X, F, 1, 1)
                assert r["count"][0] >= 1
                err = abs(float(r["out"][0, 0, 0]) - (k0 + off))
                worst = max(worst, err)
                assert err <= 0.02, (k0, off, phase, err)
                raw = X[0, r["sel"][0, 0], 0]                  # what refine = 0 writes: the bin centre
                raw_off += abs(float(raw) - (k0 + off)) > 0.02
                cases += 1
    print(f"worst refined error {worst:.4f} bin; raw bin off by > 0.02 in {raw_off} of {cases} cases")
    assert cases == 3 * 41 * 3 and 2 * raw_off >= cases


def test_reference_order_is_the_stable_argsort_over_its_mask():
    rng = np.random.default_rng(5)
    F, Nt = 61, 4
    v = np.clip(rng.normal(-9.0, 3.0, F * Nt), -18.4, 0.0).astype(np.float32)
    v[rng.integers(0, F * Nt, 40)] = np.float32(-18.4)            # ties
    f = np.tile(np.linspace(0, 0.5, F), Nt)
    t = np.repeat(np.arange(Nt), F)
    X = np.stack((f, t, v), axis=1).astype(np.float32)[None]
    for rf, rt in ((1, 0), (2, 1)):
        r = peak_ref.peak_points(X, F, Nt, F * Nt, rf, rt, refine_on=False)
        order = np.argsort(-v, kind="stable")
        want = order[r["mask"][0][order]]
        n = int(r["count"][0])
        assert n == len(want) == int(r["lengths"][0]) and n > 0
        assert np.array_equal(r["sel"][0, :n], want) and np.all(r["sel"][0, n:] == -1)
        assert np.array_equal(r["out"][0, :n], X[0, want]) and not r["out"][0, n:].any()
        vs = r["out"][0, :n, 2]
        assert np.all(vs[:-1] >= vs[1:])


def _row(vals):
    v = np.asarray(vals, dtype=np.float32)
    return np.stack((np.arange(len(v), dtype=np.float32), v), axis=1)[None], len(v)


def test_plateau_and_nan_rules_on_hand_made_rows():
    nan = np.nan
    # a plateau: the lowest index wins, and only where it rises from the left
    X, F = _row([0, 1, 1, 1, 0, 2, 2, 0])
    assert list(np.flatnonzero(peak_ref.peak_points(X, F, 1, F)["mask"][0])) == [1, 5]
    # a plateau that starts on the edge bin: bin 0 is a neighbour only, and bin 1 ties with it and loses
    X, F = _row([1, 1, 1, 0, 0, 3, 0])
    assert list(np.flatnonzero(peak_ref.peak_points(X, F, 1, F)["mask"][0])) == [5]
    # equal values two bins apart: both are peaks at radius 1, the lower index alone at radius 2
    X, F = _row([0, 5, 0, 5, 0])
    assert list(np.flatnonzero(peak_ref.peak_points(X, F, 1, F, 1)["mask"][0])) == [1, 3]
    assert list(np.flatnonzero(peak_ref.peak_points(X, F, 1, F, 2)["mask"][0])) == [1]
    # NaN is never a peak and loses as a neighbour; the refinement next to it is the raw row
    X, F = _row([0, nan, 4, nan, 1, 2, 1])
    r = peak_ref.peak_points(X, F, 1, F)
    assert list(np.flatnonzero(r["mask"][0])) == [2, 5]
    assert r["sel"][0, :2].tolist() == [2, 5]
    assert r["out"][0, 0].tolist() == [2.0, 4.0]
    assert abs(float(r["out"][0, 1, 0]) - 5.0) < 1e-6 and float(r["out"][0, 1, 1]) == 2.0
    # edge bins are neighbours only; a constant or all-NaN set falls back to max-K's first point
    X, F = _row([9, 1, 2, 1, 9])
    assert list(np.flatnonzero(peak_ref.peak_points(X, F, 1, F)["mask"][0])) == [2]
    for vals, first in (([3, 3, 3, 3], 0), ([nan, nan, nan], 0), ([1, 2, 3, 4], 3)):
        X, F = _row(vals)
        r = peak_ref.peak_points(X, F, 1, 2)
        assert r["count"][0] == 0 and r["lengths"][0] == 1 and r["sel"][0].tolist() == [first, -1]
    # for every peak v[f] > v[f-1] and v[f] >= v[f+1]; the floors cut by value
    X, F = _row([0, 5, 0, 3, 0, 1, 0])
    assert list(np.flatnonzero(peak_ref.peak_points(X, F, 1, F, rel_floor=2.0)["mask"][0])) == [1, 3]
    assert list(np.flatnonzero(peak_ref.peak_points(X, F, 1, F, abs_floor=4.0)["mask"][0])) == [1]
    assert peak_ref.peak_points(X, F, 1, F, abs_floor=6.0)["count"][0] == 0


def _spec(radius_f=1, radius_t=0, rel_floor=np.inf, abs_floor=-np.inf, refine=1):
    return _lib.PcaPeakSpec(radius_f, radius_t, rel_floor, abs_floor, refine)


@pytest.mark.parametrize("B,F,Nt,din,K,spec,word", [
    (2, 2, 1, 2, 1, _spec(), b"F=2"),
    (2, 64, 1, 2, 0, _spec(), b"K=0"),
    (2, 64, 2, 3, 129, _spec(), b"K=129"),                 # K > N
    (2, 512, 33, 3, 10, _spec(), b"16384"),                # N > 16384
    (2, 64, 2, 2, 10, _spec(), b"Nt=2"),                   # din = 2 carries no time
    (2, 64, 1, 2, 10, _spec(radius_f=0), b"radius_f=0"),
    (2, 64, 1, 2, 10, _spec(radius_f=17), b"radius_f=17"),
    (2, 64, 4, 3, 10, _spec(radius_t=5), b"radius_t=5"),
    (2, 64, 1, 2, 10, _spec(rel_floor=-1.0), b"rel_floor"),
    (2, 64, 1, 2, 10, _spec(abs_floor=np.nan), b"abs_floor"),
    (2, 64, 1, 2, 10, _spec(refine=2), b"refine=2"),
    (0, 64, 1, 2, 10, _spec(), b"B=0"),
    (2, 64, 1, 4, 10, _spec(), b"din=4"),
])
def test_peak_points_argument_errors(B, F, Nt, din, K, spec, word):
    """Refused before anything is enqueued, the argument named - with NULL pointers too."""
    L = pca_hip.lib()
    one = ctypes.c_void_p(256)            # non-null, never dereferenced: the arguments are refused first
    for X, out, ln in ((None, None, None), (one, ctypes.c_void_p(1 << 40), one)):
        rc = L.pca_peak_points(X, None, B, F, Nt, din, ctypes.byref(spec), K, out, ln, None, None, None)
        assert rc == -1 and word in L.pca_last_error(), L.pca_last_error()


def test_peak_points_null_pointers_and_aliasing_are_errors():
    L = pca_hip.lib()
    one = ctypes.c_void_p(256)
    far = ctypes.c_void_p(1 << 40)
    s = _spec()
    assert L.pca_peak_points(None, None, 2, 64, 1, 2, ctypes.byref(s), 10, far, one, None, None, None) == -1
    assert b"null" in L.pca_last_error()
    assert L.pca_peak_points(one, None, 2, 64, 1, 2, None, 10, far, one, None, None, None) == -1
    assert b"spec" in L.pca_last_error()
    assert L.pca_peak_points(one, None, 2, 64, 1, 2, ctypes.byref(s), 10, one, one, None, None, None) == -1
    assert b"overlaps" in L.pca_last_error()
    with pytest.raises(ValueError):
        pca_hip.ops.peak_spec(radius_f=0)
    with pytest.raises(ValueError):
        pca_hip.ops.peak_spec(rel_floor=float("nan"))
