"""k_mab1_bwd (csrc/mab1_bwd_bf16.hip) after its bf16 tile operands - dY and the saved Qp in, dZ, dQp and dX out -
went from 8-byte accumulator fragments to 16-byte chunks exchanged between lane groups, and the reductions behind
the tiles to barriers that order LDS only.  No arithmetic changed, so none of it may move a bit.  The cases
(tests/mab1_bwd_wide_cases.py) are whole eager train steps, d = 128, h = 4, m = 16, C = 50, bf16 mode, on the
per-block path (PCA_SET128=0) but for the last: a last tile with one live row and dZ materialised (N = 129), one
16-row group plus one row with three components per point (N = 33), a set of one 16-row group (N = 16), one
component per point (N = 40, din = 1: the parent's library takes it, so the case is in), and B = 5, N = 256 behind
the set-resident forward, which hands bf16 tensors to both launches.  Per case:

* both expected instances of k_mab1_bwd ran, once each (kernel names of a step);
* two passes are bitwise equal;
* the CPU oracle is met at the bf16 mode's bars (tests/grad_bars.py) and the tolerances of
  tests/test_gpu_mab1_bwd_loads.py;
* all 47 outputs have the SHA-256 that the parent commit's build produced
  (tests/golden/mab1_bwd_wide_sha256.json, recorded by scripts/mab1_bwd_wide_golden.py from a library built from
  the parent, never from this tree's).

The N = 129 and N = 33 cases then run again in two surroundings and must give the same hashes: X as a slice in
the middle of a larger tensor that is NaN directly before and after it, and the engine's workspace filled with
0xFF bytes before the step, the word the host initialises by contract apart - the hand-off counter of the
set-resident forward; there is no other.  A widened or clamped load that uses a byte outside its tile, or a row
the step has not written, then shows as a changed hash.  (The recorder checked that the parent's build gives the
same hashes in both surroundings.)"""
import functools
import json
import os

import pytest
import torch

import grad_bars as gb
import mab1_bwd_loads_cases as lc
import mab1_bwd_wide_cases as wc
from util import T, close, close_robust

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "mab1_bwd_wide_sha256.json")


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
    net = wc.engine_net(dev, key)
    Xn, yn = wc.engine_inputs(key)
    X, y = T(Xn, dev), T(yn, dev)
    r1, names = wc.run(net, key, X, y, witness=True)
    r2, _ = wc.run(net, key, X, y)
    return net, Xn, yn, r1, r2, names


def _parent_hashes(key, out, what):
    want = _golden()["cases"][key]
    got = lc.hashes(out)
    assert len(want) == 47 and got.keys() == want.keys(), (sorted(got), sorted(want))
    moved = [k for k in want if got[k] != want[k]]
    assert not moved, (key, what, moved)


def test_every_case_was_recorded():
    assert sorted(_golden()["cases"]) == sorted(wc.CASES) and not _golden()["refused"]


@pytest.mark.parametrize("key", list(wc.CASES))
def test_path_and_two_passes(dev, key):
    _, _, _, r1, r2, names = _case(key)
    for args in wc.CASES[key][4]:
        assert lc.ran(names, args), (key, args, [n for n in names if "mab1_bwd" in n])
    assert sum("k_mab1_bwd" in n for n in names) == 2, names       # one launch per ISAB
    assert any("k_set128_fwd" in n for n in names) == wc.CASES[key][3], names
    assert r1.keys() == r2.keys()
    for k in r1:
        assert torch.isfinite(r1[k]).all(), (key, k)
        assert torch.equal(r1[k], r2[k]), f"{key}, second pass: {k}: max |diff| {float((r1[k] - r2[k]).abs().max()):.3e}"


@pytest.mark.parametrize("key", list(wc.CASES))
def test_parent_hashes(dev, key):
    _, _, _, r1, _, _ = _case(key)
    assert len(r1) == 47                                           # logits, loss, 45 gradients
    _parent_hashes(key, r1, "plain")


@pytest.mark.parametrize("key", list(wc.CASES))
def test_oracle(dev, key):
    net, Xn, yn, r1, _, _ = _case(key)
    ref_loss, ref_lg, ref_g = wc.oracle(net, key, Xn, yn)
    e = close(r1["logits"], ref_lg, 3e-2, "logits")
    print(f"{key}: logits {e:.3e}, loss {float(r1['loss']):.5f} (oracle {ref_loss:.5f})")
    assert abs(float(r1["loss"]) - ref_loss) < 3e-2 * max(1.0, abs(ref_loss))
    flat = []
    for k, prm in net.named_parameters():
        w = close_robust(r1[k], ref_g[k], 5e-2, k, outlier_frac=5e-3)
        flat.append(r1[k].reshape(-1))
        print(f"  {k}: worst {w:.3e}")
    gb.judge(torch.cat(flat), ref_g, gb.BF16_VS_ORACLE, gb.shapes_of(net), f"{key} vs oracle")


@pytest.mark.parametrize("key", wc.SURROUNDED)
def test_x_surrounded_by_nan(dev, key):
    net, Xn, yn, _, _, _ = _case(key)
    X, whole = wc.surrounded(Xn, dev)
    out, _ = wc.run(net, key, X, T(yn, dev))
    assert bool(torch.isnan(whole[:wc.PAD]).all()) and bool(torch.isnan(whole[-wc.PAD:]).all())
    _parent_hashes(key, out, "X surrounded by NaN")


@pytest.mark.parametrize("key", wc.SURROUNDED)
def test_workspace_filled(dev, key):
    net, Xn, yn, _, _, _ = _case(key)
    out, _ = wc.run(net, key, T(Xn, dev), T(yn, dev), fill_ws=True)
    _parent_hashes(key, out, "workspace filled with 0xFF")
