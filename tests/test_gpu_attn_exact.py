"""The fused attention blocks on exact-operand inputs (attn_exact_cases.py): softmax rows that are one-hot
or exact 2- / 4-way ties, scores of 64 .. 540 nats, planted keys at the tile, group and split edges, masked
would-be winners behind every length, and a +-96-nat offset on all scores of a row.  test_attn_exact_host.py
shows on the CPU that no operand rounding takes part on these inputs and that a wrong max, a missing
rescale, a wrong merge, an unskipped empty range, an off-by-one or per-tile mask and swapped heads each
move the result by more than 100 x the bar below.

Forward, against the fp64 oracle on the truncated sets: 2^-16 max(1, max|ref|).  No operand is rounded
(host condition 1), so what is left is fp32 arithmetic on exactly representable values and a handful of
<= 1-ulp hardware approximations per output (v_exp_f32 at 0 or below -64 nats, one reciprocal of l, the
per-tile and per-range rescale products): a dozen factors of (1 +- 2^-23), <= 2^-19; the bar allows 8 x
that.  It is not measured on the kernel.

Backward, against autograd of the fp64 oracle: 1.5e-2 max(1, max|ref tensor|) (the emulation bar of
test_gpu_bf16.py / EMU_BWD_TOL of test_gpu_sab.py) as a plain max error, no outlier allowance: min|Z| is
1/8 on these inputs, so no ReLU derivative can flip.  fc_k.bias.grad is judged on the scale of
fc_k.weight.grad; rows of dK (self-attention: dX) behind a set's length are exact zeros.

Measured on the MI355X: see MEASURED below."""
import pytest
import torch

import attn_exact_cases as ax
from dispatch import launches
from mab1_bwd_loads_cases import kernel_names
from test_gpu_bf16 import _guard_workspaces  # noqa: F401  (autouse: guard regions behind every workspace)

pytestmark = pytest.mark.gpu

# worst figures per family over the cases below, relative to the bars' scales (forward: of max(1, max|ref|);
# gradients: of max(1, max|ref tensor|), the worst tensor named)
MEASURED = """
on the tree of this change (parent 8a712db), worst over the family's cases:
  Mab1_128           forward 1.2e-08   gradients fc_k.weight 3.2e-03, dK 1.7e-03, fc_q.weight 2.4e-03 (layer 1)
  Mab1_256           forward 1.5e-08   gradients dK 3.0e-03, fc_k.weight 2.7e-03
  Mab0_128           forward 1.5e-08   gradients fc_k.weight 3.3e-03, dK 1.9e-03; layer 1: dQ 3.1e-06
  Mab0_256           forward 1.2e-08   gradients dK 2.8e-03, fc_k.weight 2.4e-03; layer 1: dQ 4.7e-06
  ExactCore          forward 1.5e-08   gradients fc_k.weight 1.9e-03, dX 1.4e-03
  Sd64 (inference)   forward 9.0e-56
every other gradient below 1e-5.  Before k_mab0_bwd_small dropped the dS of a chunk's padding point
(mab0_bwd_small_body.hpp) the two Mab0_128 layer-1 cases returned NaN in dQ and d fc_q / d fc_k."""


@pytest.fixture(scope="module")
def dev():
    import pca_hip
    pca_hip.lib()
    yield torch.device("cuda", 0)
    pca_hip.set_mode("f32")


@pytest.fixture
def bf16():
    import pca_hip
    pca_hip.set_mode("bf16")
    try:
        yield
    finally:
        pca_hip.set_mode("f32")


def _block(case, dev):
    """(module, call(no_grad) -> (Y, {name: leaf tensor}))"""
    import modules
    c = ax.build(case)
    d, h = case.d, case.h
    p = ax.f32(c["p"])
    kl = None if c["lengths"] is None else torch.tensor(c["lengths"], dtype=torch.int32, device=dev)
    K = c["K"].float().to(dev)
    if case.kind == "sab":
        mod = modules.SAB(d, d, h)
        mab = mod.mab
    else:
        mod = mab = modules.MAB(c["Q"].shape[-1], c["K"].shape[-1], d, h)
    mab.load_state_dict(p)
    mod.to(dev)
    Q = c["Q"].float().to(dev)

    def call(train):
        mod.zero_grad()
        Kd = K.clone().requires_grad_(train and not (case.kind == "fq" and case.layer1))
        if case.kind == "sab":
            return mod(Kd, kl), {"dX": Kd}
        Qd = Q.clone().requires_grad_(train and not (case.kind == "mq" and case.layer1))
        if case.kind == "fq":
            return mab(Qd, Kd, q_shared=True, key_lengths=kl), {"dQ": Qd, "dK": Kd}
        return mab(Qd, Kd), {"dQ": Qd, "dK": Kd}

    return mab, call


def _fwd_err(case, Y, ref):
    """max|Y - ref| / max(1, max|ref|) over the valid rows; Y must be finite there."""
    Y = Y.detach().cpu().double()
    if case.kind == "sab":
        for b, L in enumerate(ax._lens(case)):
            Y[b, L:] = 0
    assert bool(torch.isfinite(Y).all()), f"{case.key}: non-finite output"
    return float((Y - ref).abs().max()) / max(1.0, float(ref.abs().max()))


def _witness(case, step, infer):
    if case.family == "Sd64":
        names = kernel_names(infer)
        want = "k_sd_fq" if case.kind == "fq" else "k_sd_mq"
        assert any(want in n for n in names) and not any("gemm" in n for n in names), names
        return
    if case.family == "ExactCore":
        names = kernel_names(step)
        stem = "k_attn32" if case.d // case.h == 32 else "k_attnc"
        for part in ("_fwd", "_bwd_q", "_bwd_kv"):
            assert any(stem + part in n for n in names), (stem + part, names)
        n = launches(step, ("gemm_f32", "mab1_fwd", "mab0_fwd"))
        assert n == {"gemm_f32": 0, "mab1_fwd": 0, "mab0_fwd": 0}, n
        return
    kind = "mab1" if case.family.startswith("Mab1") else "mab0"
    other = "mab0" if kind == "mab1" else "mab1"
    if case.kind == "fq" and case.layer1:        # the layer-1 few-queries kernels have no launch counter
        names = kernel_names(step)
        for want in ("k_mab0_attn_small", "k_mab0_bwd_small"):
            assert any(want in n for n in names), (want, names)
        assert launches(step, ("mab1_fwd",)) == {"mab1_fwd": 0}
        return
    n = launches(step, (f"{kind}_fwd", f"{kind}_bwd", f"{other}_fwd"))
    assert n[f"{kind}_fwd"] > 0 and n[f"{kind}_bwd"] > 0 and n[f"{other}_fwd"] == 0, n


@pytest.mark.parametrize("case", ax.CASES, ids=[c.key for c in ax.CASES])
def test_exact_operands(dev, bf16, case):
    c = ax.build(case)
    ref = ax.oracle_forward(case)
    mab, call = _block(case, dev)
    G = c["G"].float().to(dev)

    def infer():
        with torch.no_grad():
            return call(False)[0]

    def step():
        Y, leaves = call(True)
        (Y * G).sum().backward()
        return Y, leaves

    e_inf = _fwd_err(case, infer(), ref)
    line = f"\n{case.key}: forward (inference) {e_inf:.2e}"
    errs = {}
    if case.train:
        Y, leaves = step()
        torch.cuda.synchronize()
        e_fwd = _fwd_err(case, Y, ref)
        line += f" (training) {e_fwd:.2e}"
        gr = ax.oracle_grads(case)
        got = {k: v.grad for k, v in leaves.items() if v.requires_grad}
        for k, prm in mab.named_parameters():
            got[k] = prm.grad if prm.grad is not None else torch.zeros_like(prm)
        for k, v in got.items():
            v = v.detach().cpu().double()
            assert bool(torch.isfinite(v).all()), f"{case.key}: non-finite {k}"
            sc = max(1.0, float(gr["fc_k.weight" if k == "fc_k.bias" else k].abs().max()))
            errs[k] = float((v - gr[k]).abs().max()) / sc
            if k in ("dK", "dX") and case.lengths is not None:
                for b, L in enumerate(case.lengths):
                    assert bool((v[b, L:] == 0).all()), f"{case.key}: {k} rows behind length {L} of set {b}"
        line += " gradients " + " ".join(f"{k} {v:.1e}" for k, v in errs.items())
    print(line)
    _witness(case, step, infer)
    assert e_inf <= ax.FWD_BAR, (case.key, "inference forward", e_inf)
    if case.train:
        assert e_fwd <= ax.FWD_BAR, (case.key, "training forward", e_fwd)
        for k, e in errs.items():
            assert e <= ax.BWD_BAR, (case.key, k, e)
