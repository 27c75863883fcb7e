"""Self-attention blocks (SAB, set_transformer-master/modules.py:35-41) in bf16 at any set size: kind 4
of the C ABI, the bf16-operand chain with its attention on the fused core (head dim 32: k_attn32_*;
head dims 8 / 16: k_attnc_*), which never builds the N x N score matrix.

Each case is checked against the fp32 oracle with Q = K = X (dX = dQ + dK) at the bars of
test_gpu_bf16.py (forward max error, gradients in rms: ReLU ties), and against a bf16-operand emulation
below at tighter bars (EMU_FWD_TOL / EMU_BWD_TOL, max error)."""
import numpy as np
import pytest
import torch

from dispatch import launches
from util import close

pytestmark = pytest.mark.gpu

FWD_TOL = 1.5e-2          # test_gpu_bf16.py
BWD_TOL = 3e-2
# against _emu_forward (the kernel's operand roundings, fp32 everything else), max error relative to
# max(1, max|emu|); measured on the MI355X over CASES: Y <= 3.3e-4, gradients <= 1.05e-2 (fc_k.weight at
# din = 3), <= 6e-3 otherwise
EMU_FWD_TOL = 1e-3
EMU_BWD_TOL = 1.5e-2


@pytest.fixture(scope="module")
def dev():
    import pca_hip
    pca_hip.lib()
    return torch.device("cuda", 0)


@pytest.fixture
def bf16():
    import pca_hip
    pca_hip.set_mode("bf16")
    try:
        yield
    finally:
        pca_hip.set_mode("f32")


def _params(din, d, seed):
    g = torch.Generator().manual_seed(seed)
    p = {}
    for nm, k in (("fc_q", din), ("fc_k", din), ("fc_v", din), ("fc_o", d)):
        bound = 1.0 / np.sqrt(k)
        p[nm + ".weight"] = (torch.rand(d, k, generator=g) * 2 - 1) * bound
        p[nm + ".bias"] = (torch.rand(d, generator=g) * 2 - 1) * bound
    return p


def _sab(p, din, d, h, dev):
    import modules
    m = modules.SAB(din, d, h).to(dev)
    m.mab.load_state_dict(p)
    return m


def _rb(x):
    return x.bfloat16().float()


def _emu_forward(X, p, h):
    """modules.py:19-33 with the kernel's roundings: every GEMM operand (X, W, Qp, Kp, Vp, P, O) in
    bf16, products and softmax in fp32.  Differentiable: autograd through a rounding x.bfloat16().float()
    rounds the gradient that passes it to bf16 as well, so the backward carries bf16 roundings at the same
    points (not necessarily the kernel's own: EMU_BWD_TOL allows for the difference)."""
    def lin(x, nm):
        return _rb(x) @ _rb(p[nm + ".weight"]).t() + p[nm + ".bias"]
    B, N, _ = X.shape
    d = p["fc_q.weight"].shape[0]
    dh = d // h
    Qp, Kp, Vp = lin(X, "fc_q"), lin(X, "fc_k"), lin(X, "fc_v")
    sp = lambda t: t.view(B, N, h, dh).permute(0, 2, 1, 3)      # noqa: E731
    S = _rb(sp(Qp)) @ _rb(sp(Kp)).transpose(-1, -2) / np.sqrt(d)
    E = torch.exp(S - S.amax(-1, keepdim=True))
    O = sp(Qp) + (_rb(E) @ _rb(sp(Vp))) / E.sum(-1, keepdim=True)
    O = O.permute(0, 2, 1, 3).reshape(B, N, d)
    return O + torch.relu(lin(O, "fc_o"))


def _grads(m, X, G):
    """Y, dX and the parameter gradients of one training call of SAB m."""
    Xd = X.clone().requires_grad_(True)
    m.zero_grad()
    Y = m(Xd)
    (Y * G).sum().backward()
    out = {"Y": Y.detach(), "dX": Xd.grad.detach()}
    for k, prm in m.mab.named_parameters():
        out[k] = prm.grad.detach().clone()
    return out


CASES = [   # B, N, din, d, h
    (3, 200, 128, 128, 4),
    (2, 517, 3, 128, 4),
    (2, 300, 256, 256, 8),
    (4, 1025, 64, 64, 8),        # head dim 8 (the dh <= 16 core)
    (2, 1, 128, 128, 4),
    (8, 4, 128, 128, 4),         # a decoder-sized SAB over four PMA seeds
    (1, 4096, 128, 128, 4),
    (2, 130, 128, 128, 16),      # head dim 8 at d = 128
    (2, 200, 128, 128, 8),       # head dim 16 at d = 128 (78 KB of LDS in k_attnc_bwd_kv<8>)
    (3, 90, 64, 64, 4),          # head dim 16 at d = 64
    (3, 70, 64, 64, 2),          # head dim 32 at d = 64
]


@pytest.mark.parametrize("case", CASES, ids=[str(c) for c in CASES])
def test_sab_bf16_against_oracle(dev, bf16, case):
    from oracle import st_oracle as orc
    B, N, din, d, h = case
    p = _params(din, d, seed=sum(case))
    g = torch.Generator().manual_seed(7 + sum(case))
    X = torch.randn(B, N, din, generator=g)
    if din <= 4:
        X[..., -1] = X[..., -1] * 3 - 9
    G = torch.randn(B, N, d, generator=g)
    m = _sab(p, din, d, h, dev)
    got = _grads(m, X.to(dev), G.to(dev))
    with torch.no_grad():
        Yi = m(X.to(dev))
    # the oracle: Q = K = X, dX = dQ + dK
    ref = orc.mab_forward(X, X, p, h)
    rb = orc.mab_backward(G, X, X, p, h)
    close(got["Y"], ref, FWD_TOL, f"Y {case}")
    assert torch.equal(Yi, got["Y"]), "inference and training forwards differ"
    # gradients in rms against the exact oracle (test_gpu_bf16.py: a ReLU pre-activation within rounding
    # distance of 0 flips its derivative, and here a whole row of dX with it)
    exact = dict(rb, dX=rb["dQ"] + rb["dK"])
    for k in exact:
        if k in ("dQ", "dK"):
            continue
        sc = max(1.0, float(exact["fc_k.weight" if k == "fc_k.bias" else k].abs().max()))
        rms = float((got[k].cpu() - exact[k]).pow(2).mean().sqrt()) / sc
        assert rms < BWD_TOL, (k, rms)
    # the bf16-operand emulation at tighter bars, on parameters that keep fc_o's pre-activation away
    # from the ReLU kink (Z ~ 1 +- 0.1), so that the two share the ReLU mask
    p["fc_o.weight"] = p["fc_o.weight"] * 0.1
    p["fc_o.bias"] = p["fc_o.bias"] * 0.1 + 1.0
    m.mab.load_state_dict(p)
    got = _grads(m, X.to(dev), G.to(dev))
    Xe = X.clone().requires_grad_(True)
    pe = {k: v.clone().requires_grad_(True) for k, v in p.items()}
    Ye = _emu_forward(Xe, pe, h)
    (Ye * G).sum().backward()
    emu = {k: v.grad for k, v in pe.items()}
    emu["dX"] = Xe.grad
    errs = {"Y": close(got["Y"], Ye.detach(), EMU_FWD_TOL, f"Y vs emulation {case}") /
            max(1.0, float(Ye.abs().max()))}
    for k in emu:
        sc = max(1.0, float(emu["fc_k.weight" if k == "fc_k.bias" else k].abs().max()))
        errs[k] = float((got[k].cpu() - emu[k]).abs().max()) / sc
    print(f"\n{case}: max relative error against the emulation " +
          " ".join(f"{k} {v:.2e}" for k, v in errs.items()))
    for k, e in errs.items():
        assert e <= (EMU_FWD_TOL if k == "Y" else EMU_BWD_TOL), (k, e)


def test_sab_runs_on_the_core(dev, bf16):
    """Kind 4 runs no exact fp32 GEMM and no fused mab1 kernel; SAB at N = 16 without lengths keeps
    mab1_bf16 (kinds 1-3 take precedence), with lengths it moves to the core."""
    B, din, d, h = 2, 128, 128, 4
    p = _params(din, d, seed=3)
    m = _sab(p, din, d, h, dev)
    G = torch.randn(B, 200, d, device=dev)

    def step(N, lengths=None):
        X = torch.randn(B, N, din, device=dev, requires_grad=True)
        return lambda: (m(X, lengths) * G[:, :N]).sum().backward()

    n = launches(step(200), ("gemm_f32", "mab1_fwd", "mab1_bwd"))
    assert n == {"gemm_f32": 0, "mab1_fwd": 0, "mab1_bwd": 0}, n
    n = launches(step(16), ("mab1_fwd", "mab1_bwd"))
    assert n["mab1_fwd"] > 0 and n["mab1_bwd"] > 0, n
    n = launches(step(16, torch.tensor([16, 9])), ("gemm_f32", "mab1_fwd", "mab1_bwd"))
    assert n == {"gemm_f32": 0, "mab1_fwd": 0, "mab1_bwd": 0}, n


@pytest.mark.parametrize("case", [(200, [200, 1, 77], 128, 128, 4), (16, [16, 5, 11], 128, 128, 4),
                                  (300, [300, 64, 129], 256, 256, 8), (130, [1, 130, 65], 64, 64, 8)],
                         ids=lambda c: str(c))
def test_sab_lengths_equal_truncation(dev, bf16, case):
    """Padded variable-size sets: valid rows equal the truncated set's; with dY zero on padding rows,
    dX padding rows are exact zeros."""
    N, lens, din, d, h = case
    B = len(lens)
    p = _params(din, d, seed=N + d)
    g = torch.Generator().manual_seed(N)
    X = torch.randn(B, N, din, generator=g).to(dev)
    G = torch.randn(B, N, d, generator=g).to(dev)
    for b, L in enumerate(lens):
        G[b, L:] = 0
    m = _sab(p, din, d, h, dev)
    Xd = X.clone().requires_grad_(True)
    Y = m(Xd, torch.tensor(lens))
    (Y * G).sum().backward()
    torch.cuda.synchronize()
    for b, L in enumerate(lens):
        Xb = X[b:b + 1, :L].clone().requires_grad_(True)
        Yb = m(Xb, torch.tensor([L]))       # (the same kernels: N = 16 without lengths is mab1_bf16's)
        (Yb * G[b:b + 1, :L]).sum().backward()
        close(Y[b:b + 1, :L], Yb, 1e-5, f"Y set {b} length {L}")
        close(Xd.grad[b:b + 1, :L], Xb.grad, 1e-5, f"dX set {b} length {L}")
        assert bool((Xd.grad[b, L:] == 0).all()), f"dX padding rows of set {b}"


def _same(a, b, k):
    """Every output bitwise: the attention core writes each element once, the dX GEMMs do not split K, and
    the weight gradients sum per-workgroup slabs in a fixed order (wgrad_rows.hip)."""
    assert torch.equal(a, b), k


@pytest.mark.parametrize("case", [(3, 300, 128, 128, 4), (2, 517, 3, 256, 8)], ids=lambda c: str(c))
def test_sab_reproducible_and_graph_replay(dev, bf16, case):
    B, N, din, d, h = case
    p = _params(din, d, seed=11)
    m = _sab(p, din, d, h, dev)
    X = torch.randn(B, N, din, device=dev)
    G = torch.randn(B, N, d, device=dev)
    a, b = _grads(m, X, G), _grads(m, X, G)
    for k in a:
        _same(a[k], b[k], k)
    # a captured forward + backward replays what the eager call computes
    Xs = X.clone().requires_grad_(True)
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        for _ in range(2):                                 # warm-up outside the capture
            Xs.grad = None
            (m(Xs) * G).sum().backward()
    torch.cuda.current_stream().wait_stream(s)
    graph = torch.cuda.CUDAGraph()
    Xs.grad = None
    m.zero_grad(set_to_none=False)
    with torch.cuda.graph(graph):
        Yg = m(Xs)
        (Yg * G).sum().backward()
    Xs.grad.zero_()
    for prm in m.parameters():
        prm.grad.zero_()
    graph.replay()
    torch.cuda.synchronize()
    _same(Yg.detach(), a["Y"], "Y")
    _same(Xs.grad, a["dX"], "dX")
    for k, prm in m.mab.named_parameters():
        _same(prm.grad, a[k], k)


def test_sab_nan_reaches_its_set(dev, bf16):
    B, N, din, d, h = 3, 150, 128, 128, 4
    m = _sab(_params(din, d, seed=5), din, d, h, dev)
    X = torch.randn(B, N, din, device=dev)
    X[1, 37, 5] = float("nan")
    with torch.no_grad():
        Y = m(X)
    assert bool(torch.isnan(Y[1]).all()), "a NaN key reaches every query of its set"
    assert bool(torch.isfinite(Y[0]).all() and torch.isfinite(Y[2]).all())
