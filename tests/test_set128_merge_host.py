"""csrc/softmax_merge.hpp on the host (pca_debug_merge_factor: the library's host build of the header the
set-resident forward merges its softmax partials with).  A partial is (m, l, t): running max in the log2
domain, sum and weighted sum relative to it; the partial over no keys is (-inf, 0, 0) and must be the
identity of the merge - on either side, and merged with another empty one, without a NaN."""
import ctypes
import math

import numpy as np
import pytest

import pca_hip
from pca_hip import _lib

INF = float("inf")
EMPTY = (-INF, 0.0, 0.0)


def factor(m, M, guarded=1):
    return float(pca_hip.lib().pca_debug_merge_factor(m, M, guarded))


def merge(p0, p1):
    """What every merge of the kernel does: the max is left alone, the factors are guarded."""
    M = max(p0[0], p1[0])
    f0, f1 = np.float32(factor(p0[0], M)), np.float32(factor(p1[0], M))
    return (M, float(f0 * np.float32(p0[1]) + f1 * np.float32(p1[1])),
            float(f0 * np.float32(p0[2]) + f1 * np.float32(p1[2])))


def test_the_entry_point_is_a_debug_export():
    assert "pca_debug_merge_factor" in _lib.DEBUG_SIGNATURES and "pca_debug_merge_factor" not in _lib.SIGNATURES
    assert hasattr(ctypes.CDLL(_lib.LIB_PATH), "pca_debug_merge_factor")


@pytest.mark.parametrize("p", [(0.0, 1.0, 0.5), (-3.25, 17.5, -2.0), (88.0, 1e-3, 4.0), (-126.5, 3.0, 1.0)])
def test_an_empty_partial_is_the_identity_on_either_side(p):
    for got in (merge(p, EMPTY), merge(EMPTY, p)):
        assert got == tuple(float(np.float32(v)) for v in p), got
    assert factor(-INF, p[0]) == 0.0 and factor(p[0], p[0]) == 1.0


def test_two_empty_partials_merge_to_an_empty_one():
    assert math.isnan(factor(-INF, -INF, guarded=0))            # what the bare expression gives
    assert factor(-INF, -INF) == 0.0
    got = merge(EMPTY, EMPTY)
    assert got == EMPTY and not any(math.isnan(v) for v in got)


def test_non_empty_partials_get_the_unguarded_factors_bit_for_bit():
    rng = np.random.default_rng(11)
    m = np.concatenate([rng.normal(0, 30, 400), [0.0, -0.0, 127.0, -149.0, 1e-30, -1e30]]).astype(np.float32)
    o = np.concatenate([rng.normal(0, 30, 400), [0.0, 3.0, -127.0, 149.0, -1e-30, 1e30]]).astype(np.float32)
    for a, b in zip(m, o):
        M = max(float(a), float(b))
        for x in (float(a), float(b)):
            g, u = np.float32(factor(x, M)), np.float32(factor(x, M, guarded=0))
            assert g.tobytes() == u.tobytes(), (x, M, g, u)
            assert 0.0 <= float(u) <= 1.0
