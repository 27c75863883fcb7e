"""set128_shape_ok (csrc/set128_fwd.hip) on the host, through pca_debug_set128_shape_ok, which takes the number of
compute units as an argument: the rule the set-resident forward is launched by, plus the refusal of a shape whose
largest per-launch tensor - a [B N, 128] bf16 activation - would reach 2^31 bytes from its base, the range of the
kernel's unsigned 32-bit lane offsets.  No GPU needed."""
import itertools

import pca_hip
from pca_hip import _lib


def _ok(B, N, din, cus, d=128, h=4, m=16, k=1):
    return bool(pca_hip.lib().pca_debug_set128_shape_ok(B, N, din, d, h, m, k, cus))


def _rule_before(B, N, din, cus):
    """What set128_shape_ok accepted before the refusal: N in {256, 512}, 1 <= din <= 4, and the 16 cdiv(B, 8)
    workgroups of the pairs resident at once, one per compute unit."""
    return N in (256, 512) and 1 <= din <= 4 and 16 * ((B + 7) // 8) <= cus


def test_is_a_debug_entry_point():
    assert "pca_debug_set128_shape_ok" in _lib.DEBUG_SIGNATURES and "pca_debug_set128_shape_ok" not in _lib.SIGNATURES


def test_accepts_what_it_accepted():
    for cus in (256, 304, 64):
        for B, N, din in itertools.product(range(1, 129), (256, 512), range(1, 5)):
            assert _ok(B, N, din, cus) == _rule_before(B, N, din, cus), (B, N, din, cus)
    assert _ok(128, 512, 2, 256) and _ok(128, 256, 4, 256)          # the benchmark's shape and its neighbour
    assert not _ok(129, 512, 2, 256)                                # one more set: a pair without a unit


def test_other_shapes_stay_refused():
    assert not _ok(8, 128, 2, 256) and not _ok(8, 1024, 2, 256) and not _ok(8, 384, 2, 256)
    assert not _ok(8, 256, 0, 256) and not _ok(8, 256, 5, 256)
    assert not _ok(8, 256, 2, 256, d=64) and not _ok(8, 256, 2, 256, h=8)
    assert not _ok(8, 256, 2, 256, m=32) and not _ok(8, 256, 2, 256, k=2)
    assert not _ok(8, 256, 2, 0)                                    # no device


def test_refuses_2_to_the_31_bytes():
    """B N 256 bytes >= 2^31 <=> B N >= 2^23; on a device large enough to hold the pairs the room rule alone
    would accept such a shape."""
    big = 1 << 30                                                   # compute units of a device that does not exist
    for N in (256, 512):
        edge = (1 << 23) // N                                       # first B whose tensor reaches 2^31 bytes
        assert _ok(edge - 1, N, 2, big) and _rule_before(edge - 1, N, 2, big)
        assert not _ok(edge, N, 2, big) and _rule_before(edge, N, 2, big)
        assert not _ok(edge + 1, N, 2, big)
        assert not _ok((1 << 31) - 1, N, 2, big)                    # (the products are formed in 64 bits)
