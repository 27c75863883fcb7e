"""k_set128_fwd (csrc/set128_fwd.hip) after its global accesses went from per-lane 64-bit addresses to a scalar
base plus an unsigned 32-bit lane offset, the saved Qp from 8-byte accumulator pieces to 16-byte chunks exchanged
between lane groups, and the ReLU mask from one byte per lane and head to whole words through an LDS image.  No
arithmetic, barrier or hand-off changed, so none of it may move a bit.  The cases (tests/set128_addr_cases.py) are
whole eager train steps on the set-resident path.  Per case:

* one k_set128_fwd per eager step (kernel names of a step), the LEN instantiation exactly where there are lengths;
* two passes are bitwise equal and the hand-off counter stays zero;
* logits, loss, the 45 gradients (at din = 4 all but layer 1's fc_q weight and bias, which atomics sum and the
  parent's own passes do not repeat: set128_addr_cases.UNPINNED) and the saved tensors - Qp of layer 2 (and of
  layer 1 at din = 4), both O, both ReLU masks, the output of layer 1 - have the SHA-256 that the parent commit's
  build produced
  (tests/golden/set128_addr_sha256.json, recorded by scripts/set128_addr_golden.py from a library built from the
  parent, never from this tree's).

Two dense cases then run again in two surroundings and must give the same hashes: X as a slice in the middle of a
larger tensor that is NaN directly before and after it, and the engine's workspace filled with 0xFF bytes before the
step, the hand-off counter word apart.  An access that uses a byte outside its tensor, or a word the step has not
written, then shows as a changed hash.  (The recorder checked that the parent's build gives the same hashes in
both surroundings.)"""
import functools
import json
import os

import pytest
import torch

import mab1_bwd_loads_cases as lc
import set128_addr_cases as sc
from util import T

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "set128_addr_sha256.json")
KEYS = list(sc.CASES)
assert KEYS[0] == "dense-B1-N256-din1"          # the B = 1 case runs first


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
    """The case's network and its two steps, run once and shared by the tests of the case."""
    dev = torch.device("cuda", 0)
    net = sc.engine_net(dev, key)
    Xn, yn = sc.engine_inputs(key)
    X, y = T(Xn, dev), T(yn, dev)
    r1, names = sc.run(net, key, X, y, witness=True)
    r2, _ = sc.run(net, key, X, y)
    return net, Xn, yn, r1, r2, names


def _parent_hashes(key, out, what):
    want = _golden()["cases"][key]
    free = sc.UNPINNED.get(key, ())
    got = lc.hashes({k: v for k, v in out.items() if k not in free})
    n_saved = 6 + (1 if sc.CASES[key][2] == 4 else 0)
    assert len(want) == sc.N_OUT + n_saved - len(free) and got.keys() == want.keys(), (sorted(got), sorted(want))
    moved = [k for k in want if got[k] != want[k]]
    assert not moved, (key, what, moved)


def test_every_case_was_recorded():
    assert sorted(_golden()["cases"]) == sorted(sc.CASES)


@pytest.mark.parametrize("key", KEYS)
def test_path_and_two_passes(dev, key):
    _, _, _, r1, r2, names = _case(key)
    fwd = [n for n in names if "k_set128_fwd" in n]
    assert len(fwd) == 1, names                                    # one launch carries the three blocks
    B, N, din, lengths = sc.CASES[key]
    plain = fwd[0].replace(" ", "")
    want_len = lengths is not None
    assert (f"ILi{din}ELi{N // 256}ELb{int(want_len)}E" in plain
            or f"<{din},{N // 256},{'true' if want_len else 'false'}>" in plain), fwd
    assert r1.keys() == r2.keys()
    for k in r1:
        if not k.startswith("saved."):
            assert torch.isfinite(r1[k]).all(), (key, k)
        if k not in sc.UNPINNED.get(key, ()):
            assert torch.equal(r1[k], r2[k]), f"{key}, second pass: {k} differs"


@pytest.mark.parametrize("key", KEYS)
def test_parent_hashes(dev, key):
    _, _, _, r1, _, _ = _case(key)
    _parent_hashes(key, r1, "plain")


@pytest.mark.parametrize("key", sc.SURROUNDED)
def test_x_surrounded_by_nan(dev, key):
    net, Xn, yn, _, _, _ = _case(key)
    X, whole = sc.surrounded(Xn, dev)
    out, _ = sc.run(net, key, X, T(yn, dev))
    assert bool(torch.isnan(whole[:sc.PAD]).all()) and bool(torch.isnan(whole[-sc.PAD:]).all())
    _parent_hashes(key, out, "X surrounded by NaN")


@pytest.mark.parametrize("key", sc.SURROUNDED)
def test_workspace_filled(dev, key):
    net, Xn, yn, _, _, _ = _case(key)
    out, _ = sc.run(net, key, T(Xn, dev), T(yn, dev), fill_ws=True)
    _parent_hashes(key, out, "workspace filled with 0xFF")
