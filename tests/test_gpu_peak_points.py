"""pca_peak_points on the device against the numpy restatement tests/peak_ref.py.

sel, lengths and count are exact; out is exact with refine = 0 and within one fp32 ulp with refine = 1 (one
fp32 rounding of an fp64 result, whichever way the multiply-adds are contracted); padding rows are exact
zeros and sel is -1 behind the last peak.  The reference is computed once per (shape, radius, input, floors,
lengths) at K = N; a smaller K is its prefix."""
import functools

import numpy as np
import pytest
import torch

from util import T

import peak_ref

pytestmark = pytest.mark.gpu

SHAPES = [(37, 1, 2),      # N below one wave per thread-pass
          (37, 3, 3),      # N = 111
          (257, 5, 3),     # N = 1285: more than one point per thread
          (512, 32, 3)]    # N = 16384: LDS at its limit
RADII = [(1, 0), (2, 1), (16, 4)]
SHAPE_IDS = ["%dx%dx%d" % s for s in SHAPES]
RADIUS_IDS = ["r%d_%d" % r for r in RADII]


@pytest.fixture(scope="module")
def dev():
    return torch.device("cuda", 0)


def most_peaks(F, Nt):
    return (F - 1) // 2 * Nt            # ceil((F - 2) / 2) per frame


def _coords(F, Nt, din):
    """Frequency and time columns of every point; the (37, 3) shape has a non-uniform frequency axis."""
    farr = np.linspace(0.0, 0.5, F)
    if (F, Nt) == (37, 3):
        farr = 0.5 * (np.arange(F) / (F - 1)) ** 1.7
    cols = [np.tile(farr, Nt)]
    if din == 3:
        cols.append(np.repeat(np.linspace(0.0, 0.1, Nt), F))
    return [c.astype(np.float32) for c in cols]


def _bench_values(rng, n):
    """The benchmark's synthetic log-magnitude distribution."""
    return np.clip(rng.normal(-9.0, 3.0, n), -18.4, 0.0).astype(np.float32)


def _ramp(F, Nt):
    """Strictly descending along frequency, the same in every frame: no peak at any radius."""
    return np.tile(-1.0 - 0.01 * np.arange(F), Nt).astype(np.float32)


def _spikes(rng, F, Nt, n):
    """Exactly n peaks at radius (1, 0): n spikes of distinct heights on odd bins, frame after frame, over
    the ramp."""
    v = _ramp(F, Nt)
    per = (F - 1) // 2
    assert n <= per * Nt
    heights = (1.0 + rng.permutation(n)).astype(np.float32)
    for i in range(n):
        v[(i // per) * F + 1 + 2 * (i % per)] = heights[i]
    return v


def _plateaus(rng, F, Nt):
    """Runs of equal values of every length from 1 to past the widest window, out of four levels; every
    second frame repeats the one before it, so ties also run along time."""
    v = np.empty(F * Nt, dtype=np.float32)
    for t in range(Nt):
        if t % 2 == 1:
            v[t * F:(t + 1) * F] = v[(t - 1) * F:t * F]
            continue
        row, f = [], 0
        while f < F:
            run = int(rng.choice([1, 2, 3, 4, 5, 16, 17, 18, 33, 34]))
            row += [float(rng.integers(0, 4))] * run
            f += run
        v[t * F:(t + 1) * F] = row[:F]
    return v


def _nans(rng, F, Nt):
    v = _bench_values(rng, F * Nt)
    v[rng.random(F * Nt) < 0.15] = np.nan
    if Nt > 1:
        v[F:2 * F] = np.nan                       # a frame without a number
    v[0] = np.nan
    return v


def _tail(rng, F, Nt):
    """Peaks in the last sixteenth of the points only: most waves compact nothing."""
    v = _ramp(F, Nt) - 20.0
    n = F * Nt
    v[n - n // 16:] = _bench_values(rng, n // 16)
    return v


KINDS = ["bench", "constant", "plateaus", "nans", "tail", "peaks1", "peaks2", "peaks64", "peaks65",
         "peaksmax", "negzero"]


def _values(kind, F, Nt, seed):
    rng = np.random.default_rng(seed)
    if kind == "bench":
        return _bench_values(rng, F * Nt)
    if kind == "constant":
        return np.full(F * Nt, -7.25, dtype=np.float32)
    if kind == "plateaus":
        return _plateaus(rng, F, Nt)
    if kind == "nans":
        return _nans(rng, F, Nt)
    if kind == "tail":
        return _tail(rng, F, Nt)
    if kind == "negzero":                         # -0 == +0: a tie, the lower index wins
        v = np.where(rng.random(F * Nt) < 0.5, -1.0, np.where(rng.random(F * Nt) < 0.5, 0.0, -0.0))
        return v.astype(np.float32)
    n = most_peaks(F, Nt) if kind == "peaksmax" else min(int(kind[5:]), most_peaks(F, Nt))
    return _spikes(rng, F, Nt, n)


@functools.lru_cache(maxsize=None)
def _batch(shape, kinds):
    """X float32 [len(kinds), N, din] (read-only): one set per kind."""
    F, Nt, din = shape
    X = np.stack([np.stack(_coords(F, Nt, din) + [_values(k, F, Nt, 100 + i)], axis=1)
                  for i, k in enumerate(kinds)])
    X.setflags(write=False)
    return X


@functools.lru_cache(maxsize=None)
def _ref(shape, kinds, radius, rel_floor=np.inf, abs_floor=-np.inf, refine=True, lengths=None):
    """The restatement at K = N, computed once and shared."""
    F, Nt, _ = shape
    X = _batch(shape, kinds)
    if lengths is not None:                      # what lies beyond a set's frames must never be looked at
        X = X.copy()
        for b, L in enumerate(lengths):
            X[b, L:, -1] = 100.0
    r = peak_ref.peak_points(X, F, Nt, F * Nt, radius[0], radius[1], rel_floor, abs_floor, refine, lengths)
    for a in r.values():
        a.setflags(write=False)
    return X, r


def _run(dev, X, F, Nt, K, radius, **kw):
    import pca_hip
    lengths = kw.pop("lengths", None)
    if lengths is not None:
        lengths = torch.tensor(list(lengths), dtype=torch.int32, device=dev)
    Xd = T(np.array(X), dev)                      # a copy: the cached inputs are read-only
    out, lens, sel, count = pca_hip.peak_points(Xd, F, Nt, K, radius[0], radius[1], lengths=lengths,
                                                want_sel=True, want_count=True, **kw)
    torch.cuda.synchronize()
    return out.cpu().numpy(), lens.cpu().numpy(), sel.cpu().numpy(), count.cpu().numpy()


def _ulp_ok(got, want):
    """Every element equal, or both finite and within one fp32 ulp of the reference."""
    got, want = np.asarray(got, np.float32), np.asarray(want, np.float32)
    same = (got == want) | (np.isnan(got) & np.isnan(want))
    with np.errstate(invalid="ignore"):
        near = np.abs(got.astype(np.float64) - want.astype(np.float64)) <= np.spacing(np.abs(want))
    return bool(np.all(same | (np.isfinite(want) & near)))


def _check(got, r, K, refine, what):
    """One device result at K against the K = N reference ``r``."""
    out, lens, sel, count = got
    want_len = np.clip(r["count"], 1, K)
    assert np.array_equal(count, r["count"]), (what, count, r["count"])
    assert np.array_equal(lens, want_len), (what, lens, want_len)
    for b in range(len(lens)):
        n = int(want_len[b])
        assert np.array_equal(sel[b, :n], r["sel"][b, :n]) and np.all(sel[b, n:] == -1), (what, b)
        assert not out[b, n:].any() and not np.signbit(out[b, n:]).any(), (what, b, "padding rows")
        if refine:
            assert _ulp_ok(out[b, :n], r["out"][b, :n]), (what, b)
            if out.shape[2] == 3:
                assert np.array_equal(out[b, :n, 1], r["out"][b, :n, 1]), (what, b, "time is copied")
        else:
            np.testing.assert_array_equal(out[b, :n], r["out"][b, :n], err_msg=f"{what} set {b}")


def _raw(X, r):
    """The refine = 0 reference of the same call: the rows of the selected points themselves."""
    out = np.zeros_like(r["out"])
    for b in range(len(out)):
        n = max(1, int(r["count"][b]))
        out[b, :n] = X[b, r["sel"][b, :n]]
    return dict(r, out=out)


def _K_list(counts, N):
    """K below, at and above every set's peak count."""
    ks = {1, N}
    for c in counts:
        ks.update((int(c) - 1, int(c), int(c) + 1))
    return sorted(k for k in ks if 1 <= k <= N)


def _groups(shape):
    B = 2 if shape == (512, 32, 3) else 3
    return [tuple(KINDS[i:i + B]) for i in range(0, len(KINDS), B)]


@pytest.mark.parametrize("radius", RADII, ids=RADIUS_IDS)
@pytest.mark.parametrize("shape", SHAPES, ids=SHAPE_IDS)
def test_peaks_match_the_restatement(dev, shape, radius):
    F, Nt, _ = shape
    N = F * Nt
    for kinds in _groups(shape):
        X, r = _ref(shape, kinds, radius)
        if radius == (1, 0):                     # the inputs are what they claim to be
            for b, k in enumerate(kinds):
                if k.startswith("peaks"):
                    n = most_peaks(F, Nt) if k == "peaksmax" else min(int(k[5:]), most_peaks(F, Nt))
                    assert r["count"][b] == n, (k, r["count"][b])
                if k == "constant":
                    assert r["count"][b] == 0
        for K in _K_list(r["count"], N):
            _check(_run(dev, X, F, Nt, K, radius), r, K, True, f"{kinds} K={K}")
        K = max(1, int(r["count"].max()))
        _check(_run(dev, X, F, Nt, K, radius, refine=False), _raw(X, r), K, False, f"{kinds} raw K={K}")


@pytest.mark.parametrize("radius", RADII, ids=RADIUS_IDS)
@pytest.mark.parametrize("shape", SHAPES[1:], ids=SHAPE_IDS[1:])
def test_lengths_in_one_some_and_all_frames(dev, shape, radius):
    F, Nt, _ = shape
    kinds = ("bench", "plateaus", "nans")
    lengths = (F, F * ((Nt + 1) // 2), F * Nt)
    if shape == (512, 32, 3):
        kinds, lengths = kinds[:2], lengths[:2]
    X, r = _ref(shape, kinds, radius, lengths=lengths)
    for K in (1, max(1, int(r["count"].min())), F * Nt):
        _check(_run(dev, X, F, Nt, K, radius, lengths=lengths), r, K, True, f"lengths {lengths} K={K}")


@pytest.mark.parametrize("shape", SHAPES, ids=SHAPE_IDS)
def test_floors_cut_some_and_all_peaks(dev, shape):
    F, Nt, _ = shape
    kinds = ("bench", "peaksmax")
    full = _ref(shape, kinds, (1, 0))[1]["count"]
    seen = set()
    for rel, ab in ((6.0, -np.inf), (0.0, -np.inf), (np.inf, -9.0), (np.inf, 1.0e5), (3.0, -4.0)):
        X, r = _ref(shape, kinds, (1, 0), rel, ab)
        K = max(1, int(r["count"].max()))
        _check(_run(dev, X, F, Nt, K, (1, 0), rel_floor=rel, abs_floor=ab), r, K, True, f"floors {rel} {ab}")
        for b in range(2):
            seen.add("all" if r["count"][b] == 0 else "some" if r["count"][b] < full[b] else "none")
        if ab == 1.0e5:
            assert not r["count"].any()
    assert {"all", "some"} <= seen
    # rel_floor = 0 with the set's maximum on an edge bin: every peak is cut, the fallback row is that bin
    X = _batch(shape, kinds).copy()
    X[:, 0, -1] = 1.0e4
    r = peak_ref.peak_points(X, F, Nt, 4, rel_floor=0.0)
    assert not r["count"].any() and np.all(r["sel"][:, 0] == 0)
    _check(_run(dev, X, F, Nt, 4, (1, 0), rel_floor=0.0), r, 4, True, "max on the edge")


@pytest.mark.parametrize("shape", SHAPES, ids=SHAPE_IDS)
def test_prefix_select_order_and_determinism(dev, shape):
    import pca_hip
    F, Nt, din = shape
    N = F * Nt
    kinds = ("bench", "plateaus")
    radius = (2, 1) if Nt > 1 else (2, 0)
    X, r = _ref(shape, kinds, radius, refine=False)
    cmax = int(r["count"].max())
    K2 = min(N, cmax + 3)
    big = _run(dev, X, F, Nt, K2, radius)
    for K1 in sorted({1, max(1, cmax // 2), max(1, int(r["count"].min()) - 1)}):
        if K1 >= K2:
            continue
        small = _run(dev, X, F, Nt, K1, radius)
        assert np.array_equal(small[0].view(np.uint32), big[0][:, :K1].view(np.uint32))
        assert np.array_equal(small[2], np.where(np.arange(K1)[None] < small[1][:, None], big[2][:, :K1], -1))
        assert np.array_equal(small[1], np.minimum(np.maximum(r["count"], 1), K1))
    # the order is select_points' over the peaks: key = the value on a peak, NaN elsewhere
    key = np.where(r["mask"], X[:, :, -1], np.nan).astype(np.float32)
    Xd = T(np.array(X), dev)
    _, sel_all = pca_hip.select_points(Xd, T(key, dev), N)
    raw = _run(dev, X, F, Nt, max(1, cmax), radius, refine=False)
    for b in range(len(kinds)):
        n = int(r["count"][b])
        assert n > 0 and np.array_equal(sel_all[b, :n].cpu().numpy(), raw[2][b, :n])
    # two calls are bit-equal, and a graph replay equals the eager call
    a = pca_hip.peak_points(Xd, F, Nt, K2, *radius, want_sel=True, want_count=True)
    b2 = pca_hip.peak_points(Xd, F, Nt, K2, *radius, want_sel=True, want_count=True)
    for u, w in zip(a, b2):
        assert torch.equal(u.view(torch.int32), w.view(torch.int32))
    out = torch.full((len(kinds), K2, din), 7.0, device=dev)
    lens = torch.full((len(kinds),), -5, dtype=torch.int32, device=dev)
    s = torch.cuda.Stream(dev)
    s.wait_stream(torch.cuda.current_stream(dev))
    with torch.cuda.stream(s):
        pca_hip.peak_points(Xd, F, Nt, K2, *radius, out=out, lengths_out=lens)      # warm-up
    torch.cuda.current_stream(dev).wait_stream(s)
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        pca_hip.peak_points(Xd, F, Nt, K2, *radius, out=out, lengths_out=lens)
    out.fill_(7.0)
    lens.fill_(-5)
    g.replay()
    torch.cuda.synchronize()
    assert torch.equal(out.view(torch.int32), a[0].view(torch.int32)) and torch.equal(lens, a[1])
