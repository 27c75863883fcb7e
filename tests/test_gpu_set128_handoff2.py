"""k_set128_fwd (csrc/set128_fwd.hip) with round B of layer 2's quad merge, the publish of pair hand-off 2, the fetch
of the partner's partial and the cross-half merge on all sixteen waves (two feature tiles per wave) where quad 0
carried all eight.  Only WHICH thread evaluates an element changed, and when a request is issued: no expression,
operand order, contraction or order of summation, so no bit may move.  The cases (tests/set128_handoff2_cases.py)
are whole eager train steps on the set-resident path.  Per case:

* one k_set128_fwd per eager step, the LEN instantiation exactly where there are lengths;
* two passes are bitwise equal and the hand-off counter stays zero (checked inside every step);
* logits, loss and the 45 gradients have the SHA-256 that the parent commit's build produced
  (tests/golden/set128_handoff2_sha256.json, recorded by scripts/set128_handoff2_golden.py from a library built
  from the parent, never from this tree's)."""
import functools
import json
import os

import pytest
import torch

import mab1_bwd_loads_cases as lc
import set128_handoff2_cases as hc
from util import T

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "set128_handoff2_sha256.json")
KEYS = list(hc.CASES)
assert KEYS[0] == "dense-B1-N256-din2"          # a B = 1 case runs first


@functools.lru_cache(maxsize=None)
def _golden():
    with open(GOLDEN) as f:
        return json.load(f)


@pytest.fixture(scope="module")
def dev():
    import pca_hip
    pca_hip.lib()
    return torch.device("cuda", 0)


@functools.lru_cache(maxsize=None)
def _case(key):
    """The case's two steps, run once and shared by the tests of the case."""
    dev = torch.device("cuda", 0)
    net = hc.engine_net(dev, key)
    Xn, yn = hc.engine_inputs(key)
    X, y = T(Xn, dev), T(yn, dev)
    r1, names = hc.run(net, key, X, y, witness=True)
    r2, _ = hc.run(net, key, X, y)
    return r1, r2, names


def test_every_case_was_recorded():
    assert sorted(_golden()["cases"]) == sorted(hc.CASES)


@pytest.mark.parametrize("key", KEYS)
def test_path_and_two_passes(dev, key):
    r1, r2, names = _case(key)
    B, N, din, lengths, C, extra = hc.CASES[key]
    fwd = [n for n in names if "k_set128_fwd" in n]
    assert len(fwd) == 1, names                                    # one launch carries the three blocks
    plain = fwd[0].replace(" ", "")
    want_len = lengths is not None
    assert (f"ILi{din}ELi{N // 256}ELb{int(want_len)}E" in plain
            or f"<{din},{N // 256},{'true' if want_len else 'false'}>" in plain), fwd
    assert r1.keys() == r2.keys() and len(r1) == hc.N_OUT
    for k in r1:
        assert torch.isfinite(r1[k]).all(), (key, k)
        if k not in hc.UNPINNED.get(key, ()):
            assert torch.equal(r1[k], r2[k]), f"{key}, second pass: {k} differs"


@pytest.mark.parametrize("key", KEYS)
def test_parent_hashes(dev, key):
    r1, _, _ = _case(key)
    want = _golden()["cases"][key]
    free = hc.UNPINNED.get(key, ())
    got = lc.hashes({k: v for k, v in r1.items() if k not in free})
    assert len(want) == hc.N_OUT - len(free) and got.keys() == want.keys(), (sorted(got), sorted(want))
    moved = [k for k in want if got[k] != want[k]]
    assert not moved, (key, moved)
