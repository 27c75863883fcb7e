"""The per-set backward mid chain (csrc/mid_bwd_body.hpp) after its prologue was rebuilt: every global operand
requested in one go, the partial sums as batches of four with +0.f in place of a branch, dH split over the four
waves with the masked dZ tiles exchanged through LDS.  None of it may move a bit.  d = 128, h = 4, m = 16, bf16
mode; per case and path (per-block launches; set-resident forward where N allows it):

* the number of dKp / dVp partials per set is read from the library (pca_debug_mid_nparts) and pinned, so
  that a later change of the tiles-per-workgroup rule cannot quietly empty a case: the cases cover 1, 2, 3, 4,
  6 and 16 partials - one partial, a group that is not full, a full group, several groups, and a last group
  that is not full;
* two passes are bitwise equal;
* PCA_D128_MIDFUSE=0 (the stand-alone k_mid_bwd launches) and the default are bitwise equal;
* the CPU oracle is met at the tolerances tests/test_gpu_midfuse.py uses;
* logits, loss and each of the 45 gradients have the SHA-256 that the parent commit's build produced
  (tests/golden/mid_prologue_sha256.json, recorded by scripts/mid_prologue_golden.py)."""
import functools
import json
import os

import pytest
import torch

import grad_bars as gb
import mid_prologue_cases as mc
from util import T, close, close_robust

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "mid_prologue_sha256.json")
ALL = [(B, N, din, s) for (B, N, din) in mc.CASES + mc.EXTRA for s in mc.paths(N)]
IDS = [mc.key(*c) for c in ALL]


def test_partials_per_set_cover_every_path_of_the_sum():
    import pca_hip
    L = pca_hip.lib()
    seen = set()
    for (B, N, din), want in mc.NPARTS.items():
        got = (L.pca_debug_mid_nparts(B, N, 1), L.pca_debug_mid_nparts(B, N, 0))     # layer 2, layer 1
        assert got == want, (B, N, din, got, want)
        seen.update(got)
    assert {1, 2} <= seen, seen
    assert any(n % 4 == 0 for n in seen) and any(n % 4 != 0 and n > 4 for n in seen), seen
    assert any(n > 4 for n in seen), seen
    assert L.pca_debug_mid_nparts(0, 256, 1) == -1


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
def _steps(B, N, din, set128):
    """The case's network and its three steps (fused, fused again, stand-alone launches), run once and shared
    by the three tests of the case (a few small tensors per case)."""
    dev = torch.device("cuda", 0)
    net = mc.net_of(dev, din, 900 + N + din)
    Xn, yn = mc.inputs_of(B, N, din)
    X, y = T(Xn, dev), T(yn, dev)
    r1 = mc.run(net, X, y, B, N, fuse=True, set128=set128)
    r2 = mc.run(net, X, y, B, N, fuse=True, set128=set128)
    r0 = mc.run(net, X, y, B, N, fuse=False, set128=set128)
    return net, r1, r2, r0


def _same_bits(net, a, b, what):
    assert torch.isfinite(a[2]).all()
    assert torch.equal(a[0], b[0]), f"{what}: logits moved"
    assert torch.equal(a[1], b[1]), (what, float(a[1]), float(b[1]))
    off = 0
    for k, prm in net.named_parameters():
        u, v = a[2][off:off + prm.numel()], b[2][off:off + prm.numel()]
        off += prm.numel()
        assert torch.equal(u, v), f"{what}: {k}: max |diff| {float((u - v).abs().max()):.3e}"
    assert off == a[2].numel()


@pytest.mark.gpu
@pytest.mark.parametrize("B,N,din,set128", ALL, ids=IDS)
def test_two_passes_and_the_launches_have_the_same_bits(dev, B, N, din, set128):
    net, r1, r2, r0 = _steps(B, N, din, set128)
    _same_bits(net, r2, r1, "fused, second pass")
    _same_bits(net, r1, r0, "fused vs PCA_D128_MIDFUSE=0")


@pytest.mark.gpu
@pytest.mark.parametrize("B,N,din,set128", ALL, ids=IDS)
def test_parent_hashes(dev, B, N, din, set128):
    net, r1, _, r0 = _steps(B, N, din, set128)
    want = _golden()["cases"][mc.key(B, N, din, set128)]
    for name, r in (("fused", r1), ("launches", r0)):
        got = mc.hashes(net, r)
        assert got["logits"] == want["logits"], (name, "logits")
        assert got["loss"] == want["loss"], (name, "loss")
        moved = [k for k in want["grads"] if got["grads"][k] != want["grads"][k]]
        assert not moved and len(want["grads"]) == 45, (name, moved)


@pytest.mark.gpu
@pytest.mark.parametrize("B,N,din,set128", ALL, ids=IDS)
def test_oracle(dev, B, N, din, set128):
    from oracle import st_oracle as orc
    net, r1, _, _ = _steps(B, N, din, set128)
    p = {k: v.detach().cpu().clone() for k, v in net.state_dict().items()}
    Xn, yn = mc.inputs_of(B, N, din)
    ref_loss, ref_lg, ref_g = orc.st_grads(torch.from_numpy(Xn), torch.from_numpy(yn), p, 4)
    lg, loss, g = r1
    close(lg, ref_lg.reshape(B, mc.C), 3e-2, "logits")
    assert abs(float(loss) - ref_loss) < 3e-2 * max(1.0, abs(ref_loss))
    off = 0
    for k, prm in net.named_parameters():
        close_robust(g[off:off + prm.numel()].view_as(prm), ref_g[k], 5e-2, k, outlier_frac=5e-3)
        off += prm.numel()
    gb.judge(g, ref_g, gb.BF16_VS_ORACLE, gb.shapes_of(net), f"B={B} N={N} din={din} mid prologue vs oracle")
