"""The gradient bars of tests/grad_bars.py held to the arithmetic they judge, on the CPU.

At the d = 128 set-resident train step (the shape and seeds of test_gpu_set128.py's
test_set128_train_step_vs_oracle) and at one d = 256 step, the exact oracle's gradients
(oracle/st_oracle.py:st_grads) and the bf16 / fp8 operand-rounding emulation's (tests/emu.py) give:

* a positive control: the emulation passes the "vs oracle" bars of its mode against the exact gradients, so
  those bars ask no more than the mode's arithmetic allows;
* negative controls: every wrong result a whole-step reduction could plausibly produce - all zeros, x2,
  x(1 +- 3 tol_n), a sign flip, x B (a lost 1/B), a quarter of the rows zeroed, permuted rows, a
  same-shaped sibling's gradient - is rejected by the "vs oracle" and the "vs emulation" bars for every
  tensor outside grad_bars.NOISE, and all but the thinly spread ones by the per-element criteria alone
  (so that a floor on the scale fails here even though the norm criterion would still object).  NOISE
  tensors get the mutations their rule can see;
* the gap this closes: tests/util.py's ``close_robust(., 5e-2)``, relative to max(1, max|ref|), accepts an
  all-zero gradient for more than half of the 45 tensors at the set-resident shape (28 / 45 measured).
"""
import functools

import numpy as np
import pytest
import torch

import grad_bars as gb
from util import close_robust

import inputs as gi

CASES = {   # B, N, din, d, h, m, C, model seed, input seed
    "set128": (6, 256, 2, 128, 4, 16, 50, 200 + 256, 7100 + 256),
    "d256": (4, 300, 3, 256, 8, 32, 50, 5, 11),
}


@functools.lru_cache(maxsize=None)
def _case(name):
    """(name, parameter shapes, B, exact gradients, {"bf16": emulation, "fp8": emulation}) of one case."""
    import models
    from emu import st_forward_emu
    from oracle import st_oracle as orc
    B, N, din, d, h, m, C, seed, xs = CASES[name]
    torch.manual_seed(seed)
    net = models.ST(dim_input=din, num_outputs=1, dim_output=C, num_inds=m, dim_hidden=d, num_heads=h)
    p = {k: v.detach().clone() for k, v in net.state_dict().items()}
    X, y = torch.from_numpy(gi.pc_input(xs, B, N, din)), torch.from_numpy(gi.labels(xs + 1, B, C))
    _, _, exact = orc.st_grads(X, y, p, h)
    emu = {}
    for mode in ("bf16", "fp8"):
        leaves = {k: v.clone().requires_grad_(True) for k, v in p.items()}
        orc.cross_entropy(st_forward_emu(X, leaves, h, fp8=mode == "fp8"), y).backward()
        emu[mode] = {k: v.grad if v.grad is not None else torch.zeros_like(v) for k, v in leaves.items()}
    exact = {k: v.numpy().astype(np.float64) for k, v in exact.items()}
    return name, gb.shapes_of(net), B, exact, emu


@pytest.fixture(params=list(CASES))
def grads(request):
    return _case(request.param)


def _passes(got, ref, bar, shapes):
    try:
        gb.judge(got, ref, bar, shapes, quiet=True)
        return True
    except AssertionError:
        return False


@pytest.mark.parametrize("mode", ["bf16", "fp8"])
def test_emulation_passes_oracle_bars(grads, mode):
    """Positive control: the mode's emulation is within its "vs oracle" bar of the exact gradients."""
    _, shapes, _, exact, emu = grads
    bar = gb.BF16_VS_ORACLE if mode == "bf16" else gb.FP8_VS_ORACLE
    gb.judge(emu[mode], exact, bar, shapes, f"{mode} emulation vs exact")


def _siblings(name, shapes):
    """Same-shaped siblings whose gradient a wrong index could return instead: fc_q <-> fc_v of a block,
    enc.0 <-> enc.1, fc_k.bias <-> fc_q.bias.  Not: two NOISE tensors (both ~0 on the same scale), and a
    block's fc_q.bias <-> fc_v.bias - with O = Qp + A Vp and the rows of A summing to 1 both are the column
    sum of dO up to the score term, which is small (in the many-queries blocks the near-equal keys cancel
    it: the fc_k.weight reason); the fp8 bar cannot tell them apart."""
    shp = dict(shapes)
    out = []
    for a, b in ((".fc_q.", ".fc_v."), (".fc_v.", ".fc_q."), ("enc.0.", "enc.1."), ("enc.1.", "enc.0.")):
        if a in name:
            out.append(name.replace(a, b))
    if name.endswith(".fc_k.bias"):
        out.append(name[:-len("fc_k.bias")] + "fc_q.bias")
    if name.endswith((".fc_q.bias", ".fc_v.bias")):
        out = [s for s in out if not s.endswith((".fc_q.bias", ".fc_v.bias")) or s[:6] != name[:6]]
    if gb.noise_class(name) is not None:
        out = [s for s in out if gb.noise_class(s) is None]
    return [s for s in out if s in shp and shp[s] == shp[name]]


def _mutations(name, ref, all_ref, B, shapes, bar):
    r = ref
    rows = r.reshape(-1, r.shape[-1]) if r.ndim > 1 else r.reshape(-1, 1)
    out = {"zeros": np.zeros_like(r), "x2": 2 * r, "flip": -r, "xB": B * r,
           "up3n": r * (1 + 3 * bar.tol_n), "down3n": r * (1 - 3 * bar.tol_n)}
    q = rows.copy()
    q[::4] = 0                      # every 4th row (bias: element) zeroed
    out["quarter_rows"] = q.reshape(r.shape)
    if rows.shape[0] > 1 and r.ndim > 1 and not name.endswith(".I"):
        # (not dI: its m rows are nearly equal - the inducing points see nearly the same keys)
        perm = np.roll(np.arange(rows.shape[0]), 1)
        out["permute_rows"] = rows[perm].reshape(r.shape)
    for s in _siblings(name, shapes):
        out["swap:" + s] = all_ref[s]
    return out


# mutations spread thin over a tensor, left to the norm criterion: every other one must also fail the
# per-element criteria on their own (which a floor of 1 on the scale would defeat)
NORM_ONLY = ("up3n", "down3n", "quarter_rows")


def _elementwise_rejects(name, val, exact, bar):
    """The per-element criteria alone (max, rms, outliers; no norm) reject ``val``."""
    nc = gb.noise_class(name)
    scale = None if nc is None else float(np.abs(exact[nc[1]]).max())
    return bool(gb.verdict(gb.errors(val, exact[name], scale), bar, norm=False))


@pytest.mark.parametrize("kind", ["oracle_bf16", "oracle_fp8", "emu"])
def test_mutations_are_rejected(grads, kind):
    """Negative controls: one mutated tensor of the exact gradients at a time, judged against the exact
    gradients with the "vs oracle" (bf16, fp8) and "vs emulation" bars.  Every mutation of every regular
    tensor must fail.  NOISE tensors are judged on a sibling's scale, where only a sibling-sized error
    shows: a swap with a same-shaped regular tensor (fc_k.bias <-> fc_q.bias, mab1.fc_k.weight <->
    fc_v.weight) must fail."""
    case, shapes, B, exact, _ = grads
    bar = {"oracle_bf16": gb.BF16_VS_ORACLE, "oracle_fp8": gb.FP8_VS_ORACLE, "emu": gb.BF16_VS_EMU}[kind]
    assert _passes(exact, exact, bar, shapes)
    missed = []
    for name, _ in shapes:
        nc = gb.noise_class(name)
        own = nc is None
        for mut, val in _mutations(name, exact[name], exact, B, shapes, bar).items():
            if not own and not mut.startswith("swap:"):
                continue
            if np.array_equal(val, exact[name]):
                continue
            if _passes(dict(exact, **{name: val}), exact, bar, shapes):
                missed.append(f"{name}:{mut}")
            elif mut not in NORM_ONLY and not _elementwise_rejects(name, val, exact, bar):
                missed.append(f"{name}:{mut} (norm criterion only)")
    assert not missed, f"{case} {kind}: accepted mutations {missed}"


def test_noise_table_is_principled(grads):
    """The NOISE tensors are what their reasons say: the "zero" class is ~0 against its sibling in exact
    arithmetic, the "cancel" class orders of magnitude below its sibling; nothing else is that small."""
    _, shapes, _, exact, _ = grads
    n = {"zero": 0, "cancel": 0}
    for name, _ in shapes:
        nc = gb.noise_class(name)
        S = float(np.abs(exact[name]).max())
        if nc is None:
            continue
        n[nc[0]] += 1
        sib = float(np.abs(exact[nc[1]]).max())
        assert S < (1e-6 if nc[0] == "zero" else 1e-2) * sib, (name, S, nc[1], sib)
    assert n == {"zero": 5, "cancel": 2}, n


def test_floor_of_one_accepts_zeros():
    """Today's gap: relative to max(1, max|ref|), close_robust(., 5e-2, outlier_frac=5e-3) - the bar of
    test_set128_train_step_vs_oracle - takes an all-zero gradient for most tensors of the set-resident
    step; grad_bars' own-scale judge takes it for none outside NOISE (test_mutations_are_rejected)."""
    _, shapes, _, exact, _ = _case("set128")
    accepted = 0
    for name, _ in shapes:
        try:
            close_robust(np.zeros_like(exact[name]), exact[name], 5e-2, name, outlier_frac=5e-3)
            accepted += 1
        except AssertionError:
            pass
    assert accepted > len(shapes) // 2, (accepted, len(shapes))
