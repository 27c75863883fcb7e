"""k_mab1_bwd (csrc/mab1_bwd_bf16.hip) after its loads were rebuilt - one batch of requests per tile, the weight
and K / V images stored to LDS under it, the saved Qp requested a head ahead - on the paths the pins of
tests/test_gpu_mid_prologue.py do not reach (tests/mab1_bwd_loads_cases.py): a ragged last tile, the materialised
dZ, a saved Qp in layer 1, a set smaller than a tile, padded variable-size sets, waves without a tile and, as
single modules, the three m = 16 instances that take fp32 activations and m = 32 (fp32 activations, the grid-stride
form, a workgroup that moves on to another set).  None of it may move a bit.  Per case:

* the instances of k_mab1_bwd that mab1_bf16_bwd_ex dispatches to are the ones that ran (kernel names of a step);
* two passes are bitwise equal;
* the CPU oracle is met at the tolerances tests/test_gpu_midfuse.py uses (a single block: with the outlier
  allowance widened by the bf16 emulation's own distance from the exact oracle, and tightly against that
  emulation - see test_module_oracle);
* every output has the SHA-256 that the parent commit's build produced (tests/golden/mab1_bwd_loads_sha256.json,
  recorded by scripts/mab1_bwd_loads_golden.py from a library built from the parent, never from this tree's).

Some outputs are left out of the bitwise checks (mab1_bwd_loads_cases.UNPINNED): weight gradients that the library
sums by fp32 atomics over several workgroups, where the parent's own passes differ - the fc_q gradient at dq <= 4
outside the fused layer-1 reduction, and every weight gradient of the 33280-row block.  The oracle judges them all
the same, and a one-workgroup twin of each small case pins every output.

The three m = 16 instances with bf16 activations (with dX, with the fc_q recomputation, with a saved Qp) are
reached through the engine.  The three m = 16 instances with fp32 activations and both m = 32 instances are
reached through modules.MAB.  No instance is left without a public route."""
import functools
import json
import os

import pytest
import torch

import grad_bars as gb
import mab1_bwd_loads_cases as lc
from util import T, close, close_robust

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "mab1_bwd_loads_sha256.json")


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
def _engine(key):
    """The case's network and its two steps, run once and shared by the tests of the case."""
    dev = torch.device("cuda", 0)
    net = lc.engine_net(dev, key)
    Xn, yn = lc.engine_inputs(key)
    X, y = T(Xn, dev), T(yn, dev)
    r1, names = lc.engine_run(net, key, X, y, witness=True)
    r2, _ = lc.engine_run(net, key, X, y)
    return net, Xn, yn, r1, r2, names


@functools.lru_cache(maxsize=None)
def _module(key):
    dev = torch.device("cuda", 0)
    r1, names = lc.module_run(dev, key, witness=True)
    r2, _ = lc.module_run(dev, key)
    return r1, r2, names


def _same_bits(a, b, what, free=()):
    assert a.keys() == b.keys()
    for k in a:
        assert torch.isfinite(a[k]).all(), (what, k)
        if k in free:
            continue
        assert torch.equal(a[k], b[k]), f"{what}: {k}: max |diff| {float((a[k] - b[k]).abs().max()):.3e}"


def _parent_hashes(key, out):
    want = _golden()["cases"][key]
    got = {k: v for k, v in lc.hashes(out).items() if k not in lc.UNPINNED.get(key, ())}
    assert got.keys() == want.keys(), (sorted(got), sorted(want))
    moved = [k for k in want if got[k] != want[k]]
    assert not moved, (key, moved)


@pytest.mark.parametrize("key", list(lc.ENGINE))
def test_engine_path_and_two_passes(dev, key):
    net, _, _, r1, r2, names = _engine(key)
    for args in lc.ENGINE[key][6]:
        assert lc.ran(names, args), (key, args, [n for n in names if "mab1_bwd" in n])
    assert sum("k_mab1_bwd" in n for n in names) == 2, names       # one launch per ISAB
    _same_bits(r1, r2, f"{key}, second pass", lc.UNPINNED.get(key, ()))


@pytest.mark.parametrize("key", list(lc.ENGINE))
def test_engine_parent_hashes(dev, key):
    _, _, _, r1, _, _ = _engine(key)
    assert len(r1) == 47                                           # logits, loss, 45 gradients
    _parent_hashes(key, r1)


@pytest.mark.parametrize("key", list(lc.ENGINE))
def test_engine_oracle(dev, key):
    B, N, din = lc.ENGINE[key][:3]
    net, Xn, yn, r1, _, _ = _engine(key)
    ref_loss, ref_lg, ref_g = lc.engine_oracle(net, key, Xn, yn)
    e = close(r1["logits"], ref_lg, 3e-2, "logits")
    print(f"{key}: logits {e:.3e}, loss {float(r1['loss']):.5f} (oracle {ref_loss:.5f})")
    assert abs(float(r1["loss"]) - ref_loss) < 3e-2 * max(1.0, abs(ref_loss))
    flat = []
    for k, prm in net.named_parameters():
        w = close_robust(r1[k], ref_g[k], 5e-2, k, outlier_frac=5e-3)
        flat.append(r1[k].reshape(-1))
        print(f"  {k}: worst {w:.3e}")
    gb.judge(torch.cat(flat), ref_g, gb.BF16_VS_ORACLE, gb.shapes_of(net), f"{key} vs oracle")


@pytest.mark.parametrize("key", list(lc.MODULE))
def test_module_path_and_two_passes(dev, key):
    r1, r2, names = _module(key)
    assert lc.ran(names, lc.MODULE[key][4]), (key, [n for n in names if "mab1_bwd" in n])
    assert sum("k_mab1_bwd" in n for n in names) == 1, names
    _same_bits(r1, r2, f"{key}, second pass", lc.UNPINNED.get(key, ()))


@pytest.mark.parametrize("key", list(lc.MODULE))
def test_module_parent_hashes(dev, key):
    _parent_hashes(key, _module(key)[0])


def _beyond(a, b, tol):
    """Fraction of the elements of a further than tol * max(1, max|b|) from b."""
    a, b = a.detach().cpu().double(), b.detach().cpu().double()
    return float(((a - b).abs() / max(1.0, float(b.abs().max())) > tol).double().mean())


@pytest.mark.parametrize("key", list(lc.MODULE))
def test_module_oracle(dev, key):
    """A single block under a random upstream gradient, judged twice.

    Against autograd of the bf16 operand emulation (oracle/st_oracle.py), which has the kernels' ReLU masks, at
    the bars tests/test_gpu_dispatch_edges.py sets for one block (1.5e-2, 2e-4 of the elements beyond it): a wrong
    tile cannot hide there.

    Against the exact oracle at the tolerance of tests/test_gpu_midfuse.py (5e-2 of the largest element, rms half
    of that), with that test's 5e-3 of outliers PLUS the fraction of the emulation's own elements beyond 5e-2,
    computed here on the CPU.  Without that term no build passes: the emulation alone - no kernel involved - lies
    as far from the exact oracle as the kernels do (fc_o.bias: rms 2.0e-2 / 2.4e-2 / 2.2e-2 in f32act-dx,
    m32-pt-1wg, m32-newset, where the kernels measured 2.045e-2 / 2.409e-2 / 2.212e-2; 7.8e-3 to 7.8e-2 of
    fc_o's gradient beyond 5e-2, the worst element 0.27), because a pre-activation of fc_o's ReLU within bf16
    rounding of zero moves one summand of a 128- to 272-row column sum by a whole |G|.  The parent's library
    gives these very bits (test_module_parent_hashes)."""
    r1, _, _ = _module(key)
    ref = lc.module_oracle(key)
    emu = lc.module_emulation(key)
    e = close(r1["Y"], ref["Y"], 3e-2, "Y")
    print(f"{key}: Y {e:.3e}")
    for k, v in r1.items():
        if k == "Y":
            continue
        if k == "fc_k.bias":
            # identically 0 (softmax is shift invariant): rounding noise, on the scale of d/d(Wk)
            sc = max(1.0, float(ref["fc_k.weight"].abs().max()))
            assert float((v.cpu() - ref[k]).abs().max()) <= 5e-2 * sc, k
            continue
        own = _beyond(emu[k], ref[k], 5e-2)
        w = close_robust(v, emu[k], 1.5e-2, f"{k} vs emulation", outlier_frac=2e-4)
        x = close_robust(v, ref[k], 5e-2, f"{k} vs oracle", outlier_frac=5e-3 + own)
        print(f"  {k}: worst {w:.3e} vs emulation, {x:.3e} vs oracle (emulation's own outliers {own:.2e})")
