"""The C-ABI primitives of the exact fp32 path (PCA_MODE_F32) against float64: pca_gemm_f32,
pca_softmax_rows / pca_softmax_bwd_rows, pca_colsum, pca_linear_fwd / pca_linear_bwd and
pca_cross_entropy, at every dispatch arm, ragged edge, layout and accumulate / split combination.
Run with ``-m gpu``.

Reference: the same fp32 inputs promoted to float64 on the CPU.  Every tolerance is either one of the
project's named bars or an a-priori rounding bound, evaluated per element in float64 (u = 2^-24, the unit
roundoff of fp32):

* a sum of K products in fp32, in any order (split-K and atomics only reorder it): every term passes through
  at most K fused multiply-adds of its K chunk, one scaling by alpha, the additions of the bias and of C0 and
  one atomic addition per split, and kchunk + splits + 3 <= K + 8 for every shape here, so
      |err_ij| <= (K + 8) u (|alpha| |A| @ |B| + |bias| + |C0|)_ij ;
* a column sum of R rows, in any order: (R + 8) u (sum_i |x_ij| + |out0_j|);
* softmax, its backward and the gradient of the cross-entropy: the project's bar 1e-6 max(1, max|ref|)
  (tests/test_gpu_parity.py), and every softmax row sums to 1 within n 2^-23 (tests/test_gpu_pool_attn.py);
* the mean cross-entropy: 2^-22 max(1, max|logits|) + 1e-6 - the kernel forms (m + logf(s)) - x_y, so one
  rounding at the magnitude of the row maximum m enters (at most 2^-24 |m|; the bar is four of them), next
  to the errors of logf and of the last subtraction (the 1e-6).  The bar bounds that step of one sample; the
  mean over B samples is a sum of fp32 atomics on top of it, which stays well inside the bar as long as the
  sample losses are of the size of a logit gap (see test_cross_entropy_hard on its choice of wrong label).
None of them is a number read off the kernels' output."""
import ctypes as C

import numpy as np
import pytest
import torch

from util import close

pytestmark = pytest.mark.gpu

U = 2.0 ** -24


@pytest.fixture(scope="module")
def dev():
    import pca_hip
    pca_hip.lib()                     # fail loudly if the extension is missing
    pca_hip.set_mode("f32")
    return torch.device("cuda", 0)


def _lib():
    from pca_hip import _lib as L
    return L, L.lib()


def _d(t):
    return t.detach().double().cpu()


def within(got, ref, bound, what):
    """|got - ref| <= bound per element (float64); returns the worst error / bound ratio."""
    g, r, b = _d(got).numpy(), np.asarray(ref, dtype=np.float64), np.asarray(bound, dtype=np.float64)
    assert g.shape == r.shape == b.shape, (what, g.shape, r.shape, b.shape)
    assert np.all(np.isfinite(g)), f"{what}: non-finite values"
    err = np.abs(g - r)
    bad = err > b
    ratio = float(np.max(err / np.maximum(b, 1e-300))) if g.size else 0.0
    assert not bad.any(), (f"{what}: {int(bad.sum())} of {g.size} elements beyond the rounding bound, "
                           f"worst err {float(err[bad].max()):.3e}, worst err / bound {ratio:.2f}")
    return ratio


def dev_at(x, dev, off=0):
    """x on the device, its first element `off` floats behind a 16-byte boundary."""
    buf = torch.empty(x.numel() + 4, device=dev)
    v = buf[off:off + x.numel()].view(x.shape)
    v.copy_(x)
    assert v.data_ptr() % 16 == 4 * off and v.is_contiguous()
    return v


# ----------------------------------------------------------------------------- #
# pca_gemm_f32                                                                   #
# ----------------------------------------------------------------------------- #
GEMM_LAYOUTS = ["nt", "nn", "tn", "tt", "strided", "odd_nt", "odd_tn"]
# straddling the 64 x 64 tile and the K step of 16
GEMM_SHAPES = [(1, 1, 1), (63, 65, 15), (64, 64, 16), (65, 63, 17), (70, 33, 19), (5, 130, 300),
               (130, 5, 33), (17, 9, 80), (128, 128, 1000)]
ALPHA = 0.5


def _gemm_operands(layout, M, N, K, g, dev):
    """A and B as test_gemm_bf16_tile_variants builds them: A as [M, K] (k contiguous) or [K, M] (rows
    contiguous), B as [N, K] / [K, N]; "strided": neither stride is 1; "odd_*": odd leading dimensions."""
    pad = 1 if layout.startswith("odd") else 0
    a_t = layout in ("tn", "tt", "odd_tn")
    b_t = layout in ("nn", "tn", "odd_tn")
    Ms, Ks, Ns = M + (-M) % 4, K + (-K) % 4, N + (-N) % 4
    if layout == "strided":
        Abuf = torch.randn(M, K, 2, generator=g).to(dev); sa_m, sa_k = 2 * K, 2
        Aref = Abuf[:, :, 0]
        Bbuf = torch.randn(N, K, 2, generator=g).to(dev); sb_n, sb_k = 2 * K, 2
        Bref = Bbuf[:, :, 0]
    else:
        if a_t:
            Abuf = torch.randn(K, Ms + pad, generator=g).to(dev); sa_m, sa_k = 1, Ms + pad
            Aref = Abuf[:, :M].t()
        else:
            Abuf = torch.randn(M, Ks + pad, generator=g).to(dev); sa_m, sa_k = Ks + pad, 1
            Aref = Abuf[:, :K]
        if b_t:
            Bbuf = torch.randn(K, Ns + pad, generator=g).to(dev); sb_n, sb_k = 1, Ns + pad
            Bref = Bbuf[:, :N].t()
        else:
            Bbuf = torch.randn(N, Ks + pad, generator=g).to(dev); sb_n, sb_k = Ks + pad, 1
            Bref = Bbuf[:, :K]
    ldc = Ns + pad + 4                  # always > N: the columns [N, ldc) must come back untouched
    return Abuf, Bbuf, _d(Aref), _d(Bref), (sa_m, sa_k, sb_k, sb_n, ldc)


@pytest.mark.parametrize("layout", GEMM_LAYOUTS)
def test_gemm_f32_layouts_edges_splits(dev, layout):
    """Every layout x ragged shape x (accumulate, split_k): bias added exactly once, alpha applied to the
    product only, split_k = 64 clamped to the K steps, K = 80 with split_k = 4 re-split to 3 by the chunk
    rounding, nothing written in the columns [N, ldc)."""
    L, lib = _lib()
    g = torch.Generator().manual_seed(101)
    worst = 0.0
    for (M, N, K) in GEMM_SHAPES:
        Abuf, Bbuf, A64, B64, (sa_m, sa_k, sb_k, sb_n, ldc) = _gemm_operands(layout, M, N, K, g, dev)
        bias = torch.randn(N, generator=g).to(dev)
        C0 = torch.randn(M, ldc, generator=g).to(dev)
        prod = ALPHA * (A64 @ B64.t()) + _d(bias)
        mag = ALPHA * (A64.abs() @ B64.abs().t()) + _d(bias).abs()
        c0 = _d(C0)[:, :N]
        for acc, split in ((0, 1), (1, 1), (1, 0), (1, 2), (1, 4), (1, 64), (0, 4)):
            zero_c = (acc, split) == (0, 4)       # the header's contract: split_k > 1 adds into C
            Cout = torch.zeros_like(C0) if zero_c else C0.clone()
            start = torch.zeros_like(C0) if zero_c else C0
            d = L.GemmDesc(M, N, K, sa_m, sa_k, sb_k, sb_n, ldc, 1, 1, 0, 0, 0, 0, 0, 0, acc, split, ALPHA)
            L.check(lib.pca_gemm_f32(C.byref(d), Abuf.data_ptr(), Bbuf.data_ptr(), bias.data_ptr(),
                                     Cout.data_ptr(), None))
            what = f"gemm {layout} {M}x{N}x{K} acc={acc} split={split}"
            ref = prod + (c0 if acc else 0.0)
            bound = (K + 8) * U * (mag + (c0.abs() if acc else 0.0))
            worst = max(worst, within(Cout[:, :N], ref.numpy(), bound.numpy(), what))
            assert torch.equal(Cout[:, N:], start[:, N:]), f"{what}: wrote past N"
    print(f"gemm_f32 {layout}: worst err / bound {worst:.3f}")


def test_gemm_f32_own_split(dev):
    """split_k = 0 with accumulate: the library splits a long K over a small output itself (atomics into a
    random C0); without accumulate it must not (C0 is not an initial value then)."""
    L, lib = _lib()
    g = torch.Generator().manual_seed(102)
    for (M, N, K) in [(70, 33, 1000), (5, 130, 300), (17, 9, 4096), (64, 64, 256)]:
        A = torch.randn(M, K, generator=g).to(dev)
        Bm = torch.randn(N, K, generator=g).to(dev)
        bias = torch.randn(N, generator=g).to(dev)
        C0 = torch.randn(M, N, generator=g).to(dev)
        prod = ALPHA * (_d(A) @ _d(Bm).t()) + _d(bias)
        mag = ALPHA * (_d(A).abs() @ _d(Bm).abs().t()) + _d(bias).abs()
        for acc in (1, 0):
            Cout = C0.clone()
            d = L.GemmDesc(M, N, K, K, 1, 1, K, N, 1, 1, 0, 0, 0, 0, 0, 0, acc, 0, ALPHA)
            L.check(lib.pca_gemm_f32(C.byref(d), A.data_ptr(), Bm.data_ptr(), bias.data_ptr(),
                                     Cout.data_ptr(), None))
            ref = prod + (_d(C0) if acc else 0.0)
            bound = (K + 8) * U * (mag + (_d(C0).abs() if acc else 0.0))
            within(Cout, ref.numpy(), bound.numpy(), f"gemm own split {M}x{N}x{K} acc={acc}")


def test_gemm_f32_degenerate_extents(dev):
    """K = 0: C becomes the bias (C0 + bias with accumulate); M = 0 or N = 0: PCA_OK, C untouched."""
    L, lib = _lib()
    g = torch.Generator().manual_seed(103)
    M, N = 5, 7
    A = torch.randn(M, 4, generator=g).to(dev)
    Bm = torch.randn(N, 4, generator=g).to(dev)
    bias = torch.randn(N, generator=g).to(dev)
    C0 = torch.randn(M, N, generator=g).to(dev)
    for split in (1, 0, 4):
        for acc in (0, 1):
            Cout = C0.clone()
            d = L.GemmDesc(M, N, 0, 4, 1, 1, 4, N, 1, 1, 0, 0, 0, 0, 0, 0, acc, split, ALPHA)
            L.check(lib.pca_gemm_f32(C.byref(d), A.data_ptr(), Bm.data_ptr(), bias.data_ptr(),
                                     Cout.data_ptr(), None))
            if not acc:      # alpha * 0 + bias is exact
                assert torch.equal(Cout, bias.expand(M, N)), f"K=0 split={split}"
            else:            # one fp32 addition
                ref = _d(C0) + _d(bias)
                within(Cout, ref.numpy(), (8 * U * (_d(C0).abs() + _d(bias).abs())).numpy(),
                       f"K=0 accumulate split={split}")
    for (m, n) in ((0, N), (M, 0), (0, 0)):
        for acc in (0, 1):
            Cout = C0.clone()
            d = L.GemmDesc(m, n, 4, 4, 1, 1, 4, N, 1, 1, 0, 0, 0, 0, 0, 0, acc, 1, ALPHA)
            assert lib.pca_gemm_f32(C.byref(d), A.data_ptr(), Bm.data_ptr(), bias.data_ptr(),
                                    Cout.data_ptr(), None) == 0
            assert torch.equal(Cout, C0), f"M={m} N={n}: C touched"


def test_gemm_f32_batched_head_slices(dev):
    """nb1 = 3 sets x nb2 = 8 heads with the strides of the three attention products of the exact chain
    (scores, A.V, A^T.dO), and the A^T B + accumulate batch of test_gemm_strided_batched_splitk."""
    L, lib = _lib()
    g = torch.Generator().manual_seed(104)
    Bn, h, nq, nk, dh = 3, 8, 300, 32, 32
    dmodel = h * dh
    Q = torch.randn(Bn, nq, dmodel, generator=g).to(dev)
    Kx = torch.randn(Bn, nk, dmodel, generator=g).to(dev)
    Qh = _d(Q).view(Bn, nq, h, dh).permute(0, 2, 1, 3)
    Kh = _d(Kx).view(Bn, nk, h, dh).permute(0, 2, 1, 3)
    # S[b, j] = Q[b, :, j*dh:(j+1)*dh] . K[b, :, j*dh:(j+1)*dh]^T
    S = torch.zeros(Bn, h, nq, nk, device=dev)
    d = L.GemmDesc(nq, nk, dh, dmodel, 1, 1, dmodel, nk, Bn, h, nq * dmodel, dh, nk * dmodel, dh,
                   h * nq * nk, nq * nk, 0, 1, 1.0)
    L.check(lib.pca_gemm_f32(C.byref(d), Q.data_ptr(), Kx.data_ptr(), None, S.data_ptr(), None))
    within(S, (Qh @ Kh.transpose(-1, -2)).numpy(),
           ((dh + 8) * U * (Qh.abs() @ Kh.abs().transpose(-1, -2))).numpy(), "head scores")
    # O[b, :, j*dh:(j+1)*dh] = S[b, j] . V[b, :, j*dh:(j+1)*dh]
    S64 = _d(S)
    O = torch.zeros(Bn, nq, dmodel, device=dev)
    d = L.GemmDesc(nq, dh, nk, nk, 1, dmodel, 1, dmodel, Bn, h, h * nq * nk, nq * nk, nk * dmodel, dh,
                   nq * dmodel, dh, 0, 1, 1.0)
    L.check(lib.pca_gemm_f32(C.byref(d), S.data_ptr(), Kx.data_ptr(), None, O.data_ptr(), None))
    merge = lambda t, n: t.permute(0, 2, 1, 3).reshape(Bn, n, dmodel)      # noqa: E731
    within(O, merge(S64 @ Kh, nq).numpy(), ((nk + 8) * U * merge(S64.abs() @ Kh.abs(), nq)).numpy(), "A.V")
    # dV[b, :, j*dh:(j+1)*dh] = S[b, j]^T . dO[b, :, j*dh:(j+1)*dh]  (few rows, reduction over the points)
    dV = torch.zeros(Bn, nk, dmodel, device=dev)
    d = L.GemmDesc(nk, dh, nq, 1, nk, dmodel, 1, dmodel, Bn, h, h * nq * nk, nq * nk, nq * dmodel, dh,
                   nk * dmodel, dh, 0, 1, 1.0)
    L.check(lib.pca_gemm_f32(C.byref(d), S.data_ptr(), Q.data_ptr(), None, dV.data_ptr(), None))
    within(dV, merge(S64.transpose(-1, -2) @ Qh, nk).numpy(),
           ((nq + 8) * U * merge(S64.abs().transpose(-1, -2) @ Qh.abs(), nk)).numpy(), "A^T.dO")
    # batched + transposed A + accumulate: C[z] += 0.5 A[z]^T B[z]
    nb1, nb2, M, N, K = 3, 2, 17, 9, 40
    A = torch.randn(nb1, nb2, K, M, generator=g).to(dev)
    Bm = torch.randn(nb1, nb2, K, N, generator=g).to(dev)
    C0 = torch.randn(nb1, nb2, M, N, generator=g).to(dev)
    Cout = C0.clone()
    d = L.GemmDesc(M, N, K, 1, M, N, 1, N, nb1, nb2, nb2 * K * M, K * M, nb2 * K * N, K * N,
                   nb2 * M * N, M * N, 1, 1, 0.5)
    L.check(lib.pca_gemm_f32(C.byref(d), A.data_ptr(), Bm.data_ptr(), None, Cout.data_ptr(), None))
    ref = _d(C0) + 0.5 * (_d(A).transpose(-1, -2) @ _d(Bm))
    bound = (K + 8) * U * (_d(C0).abs() + 0.5 * (_d(A).abs().transpose(-1, -2) @ _d(Bm).abs()))
    within(Cout, ref.numpy(), bound.numpy(), "batched A^T B accumulate")


def test_gemm_f32_grid_refusal(dev):
    """nb1 * nb2 * split > 65535 is refused on the host: an error code, pca_last_error() set, C unchanged.
    (All strides are zero, so the one-element buffers would cover the call even if it were launched.)"""
    L, lib = _lib()
    A = torch.ones(1, device=dev)
    Bm = torch.ones(1, device=dev)
    for (nb1, nb2, K, split) in ((256, 256, 1, 1), (3, 8, 16 * 4096, 4096)):
        Cout = torch.full((1,), 7.0, device=dev)
        d = L.GemmDesc(1, 1, K, 0, 0, 0, 0, 1, nb1, nb2, 0, 0, 0, 0, 0, 0, 1, split, 1.0)
        rc = lib.pca_gemm_f32(C.byref(d), A.data_ptr(), Bm.data_ptr(), None, Cout.data_ptr(), None)
        assert rc != 0, (nb1, nb2, split)
        assert b"grid too large" in lib.pca_last_error()
        torch.cuda.synchronize()
        assert float(Cout[0]) == 7.0


# ----------------------------------------------------------------------------- #
# pca_softmax_rows / pca_softmax_bwd_rows                                        #
# ----------------------------------------------------------------------------- #
# every arm of PCA_DISPATCH_V4 (n / 4 <= 1, 2, 4, ..., 64, 128, 256, 512, 1024; beyond 4096: scalar) and of
# PCA_DISPATCH_G (n <= 8, 16, 32, beyond), and one to either side
SOFTMAX_N = [1, 2, 3, 4, 5, 8, 9, 12, 16, 17, 32, 33, 36, 64, 65, 128, 252, 256, 260, 512, 516, 1024,
             1028, 2048, 2052, 4096, 4097, 4100, 8192]
SOFTMAX_ROWS = (1, 3, 37, 257)
SOFTMAX_FAMILIES = ("randn3", "peaked", "tied_all", "tied_two", "offset")


def _softmax_rows_of(family, rows, n, g):
    if family == "randn3":
        return torch.randn(rows, n, generator=g) * 3
    if family == "peaked":            # one key carries almost all the mass
        return torch.randn(rows, n, generator=g) * 30
    if family == "tied_all":          # every entry equal
        return torch.full((rows, n), 2.5)
    if family == "tied_two":          # two equal maxima among small values
        x = torch.randn(rows, n, generator=g) * 0.1 - 5.0
        x[:, 0] = 3.0
        x[:, n - 1] = 3.0
        return x
    assert family == "offset"         # only the max-subtraction keeps expf finite
    return torch.randn(rows, n, generator=g) + 1000.0


@pytest.mark.parametrize("n", SOFTMAX_N)
def test_softmax_rows_fwd_bwd(dev, n):
    """(Both scales are powers of two, so x * scale is exact in fp32 and the float64 reference sees the very
    scores the kernel exponentiates.)  Rows with n % 4 == 0 run a second time from a base one float past a
    16-byte boundary: the scalar kernels on multiple-of-four rows."""
    L, lib = _lib()
    g = torch.Generator().manual_seed(200 + n)
    offs = (0, 1) if n % 4 == 0 else (0,)
    for rows in SOFTMAX_ROWS:
        dA0 = torch.randn(rows, n, generator=g)
        for family in SOFTMAX_FAMILIES:
            if family == "tied_two" and n < 3:
                continue
            X = _softmax_rows_of(family, rows, n, g)
            for scale in (0.25, 1.0):
                ref = torch.softmax(X.double() * scale, -1)
                for off in offs:
                    what = f"{family} rows={rows} n={n} scale={scale} off={off}"
                    A = dev_at(X, dev, off)
                    L.check(lib.pca_softmax_rows(A.data_ptr(), rows, n, scale, None))
                    close(A, ref, 1e-6, "softmax " + what)
                    a = _d(A)
                    dev_sum = float((a.sum(-1) - 1.0).abs().max())
                    assert dev_sum <= n * 2.0 ** -23, f"softmax {what}: row sums off 1 by {dev_sum:.3e}"
                    dS = dev_at(dA0, dev, off)
                    L.check(lib.pca_softmax_bwd_rows(A.data_ptr(), dS.data_ptr(), rows, n, scale, None))
                    da = dA0.double()
                    close(dS, a * (da - (da * a).sum(-1, keepdim=True)) * scale, 1e-6,
                          "softmax bwd " + what)


# ----------------------------------------------------------------------------- #
# pca_colsum                                                                     #
# ----------------------------------------------------------------------------- #
COLSUM_CASES = [   # arm, rows, cols, floats past a 16-byte boundary
    ("small", 256, 64, 0), ("small", 1, 130, 0), ("small", 17, 4100, 0),
    ("scalar32", 257, 64, 0), ("scalar32", 1000, 130, 0), ("scalar32", 300, 7, 0),
    ("scalar256", 70000, 130, 0),
    ("v4", 4096, 64, 0), ("v4", 4133, 132, 0), ("v4", 5000, 256, 0), ("v4", 8193, 260, 0),
    ("v4_misaligned", 5000, 256, 1),
    ("below_v4", 4095, 64, 0),
]


@pytest.mark.parametrize("case", COLSUM_CASES, ids=[f"{c[0]}-{c[1]}x{c[2]}" for c in COLSUM_CASES])
def test_colsum_arms(dev, case):
    L, lib = _lib()
    arm, rows, cols, off = case
    g = torch.Generator().manual_seed(300 + rows + cols)
    X = torch.randn(rows, cols, generator=g)
    Xd = dev_at(X, dev, off)
    s, sabs = X.double().sum(0), X.double().abs().sum(0)
    for acc in (0, 1):
        out = torch.full((cols,), 2.0, device=dev)
        L.check(lib.pca_colsum(Xd.data_ptr(), rows, cols, out.data_ptr(), acc, None))
        within(out, (s + 2.0 * acc).numpy(), ((rows + 8) * U * (sabs + 2.0 * acc)).numpy(),
               f"colsum {arm} {rows}x{cols} acc={acc}")


def test_colsum_no_rows(dev):
    """rows == 0: zeros, or `out` untouched with accumulate."""
    L, lib = _lib()
    X = torch.ones(64, device=dev)
    for acc in (0, 1):
        out = torch.full((64,), 2.0, device=dev)
        L.check(lib.pca_colsum(X.data_ptr(), 0, 64, out.data_ptr(), acc, None))
        assert torch.equal(out, torch.full((64,), 2.0 * acc, device=dev))


# ----------------------------------------------------------------------------- #
# pca_linear_fwd / pca_linear_bwd                                                #
# ----------------------------------------------------------------------------- #
@pytest.mark.parametrize("M", [1, 3, 257, 5000])
def test_linear_fwd_bwd(dev, M):
    """Y = X W^T + b overwrites; dX = dY W overwrites (and may be NULL); dW += dY^T X and db += colsum(dY)
    add to what the buffers hold.  Bounds: the sum-of-products bound with K = din (Y), dout (dX), M (dW)
    and the column-sum bound with R = M (db)."""
    L, lib = _lib()
    g = torch.Generator().manual_seed(400 + M)
    ws = torch.empty(int(lib.pca_linear_bwd_ws_bytes(M, 130, 65)) + 16, dtype=torch.uint8, device=dev)
    for (din, dout) in [(1, 1), (3, 2), (6, 50), (130, 65), (64, 64)]:
        what = f"linear M={M} {din}->{dout}"
        X = torch.randn(M, din, generator=g).to(dev)
        W = torch.randn(dout, din, generator=g).to(dev)
        b = torch.randn(dout, generator=g).to(dev)
        dY = torch.randn(M, dout, generator=g).to(dev)
        dW0 = torch.randn(dout, din, generator=g).to(dev)
        db0 = torch.randn(dout, generator=g).to(dev)
        x, w, dy = _d(X), _d(W), _d(dY)
        Y = torch.full((M, dout), float("nan"), device=dev)
        L.check(lib.pca_linear_fwd(X.data_ptr(), W.data_ptr(), b.data_ptr(), Y.data_ptr(), M, din, dout,
                                   None))
        within(Y, (x @ w.t() + _d(b)).numpy(),
               ((din + 8) * U * (x.abs() @ w.abs().t() + _d(b).abs())).numpy(), what + " Y")
        ref_dw = _d(dW0) + dy.t() @ x
        bnd_dw = (M + 8) * U * (_d(dW0).abs() + dy.abs().t() @ x.abs())
        ref_db = _d(db0) + dy.sum(0)
        bnd_db = (M + 8) * U * (_d(db0).abs() + dy.abs().sum(0))
        for with_dx in (True, False):
            dX = torch.full((M, din), float("nan"), device=dev)
            dW, db = dW0.clone(), db0.clone()
            L.check(lib.pca_linear_bwd(X.data_ptr(), W.data_ptr(), dY.data_ptr(),
                                       dX.data_ptr() if with_dx else None, dW.data_ptr(), db.data_ptr(),
                                       M, din, dout, ws.data_ptr(), None))
            within(dW, ref_dw.numpy(), bnd_dw.numpy(), what + f" dW (dX {'on' if with_dx else 'NULL'})")
            within(db, ref_db.numpy(), bnd_db.numpy(), what + f" db (dX {'on' if with_dx else 'NULL'})")
            if with_dx:
                within(dX, (dy @ w).numpy(), ((dout + 8) * U * (dy.abs() @ w.abs())).numpy(), what + " dX")


# ----------------------------------------------------------------------------- #
# pca_cross_entropy (hard labels)                                                #
# ----------------------------------------------------------------------------- #
def _ce_ref(x64, y, gs):
    lse = torch.logsumexp(x64, -1)
    li = lse - x64.gather(-1, y.view(-1, 1)).squeeze(-1)
    p = torch.softmax(x64, -1)
    onehot = torch.zeros_like(p).scatter_(1, y.view(-1, 1), 1.0)
    return li, (p - onehot) * gs / x64.shape[0]


@pytest.mark.parametrize("Cn", [1, 2, 63, 64, 65, 128, 129, 1000])
def test_cross_entropy_hard(dev, Cn):
    """Mean loss, dlogits (also NULL), grad_scale and the accumulated statistics.  Every row's maximum is
    raised by 1 so that the argmax is unambiguous; the wrong label is the runner-up, the label an argmax that
    breaks ties badly or reads a neighbouring lane's candidate would pick.  (It also keeps a sample's loss at
    the size of the gap between two logits.  With a random wrong label and logits ~ 30 randn the losses are
    ~100, and the 129 fp32 additions of the mean alone drift by ~1e-5, half the loss bar, which bounds one
    sample's log-sum-exp and not that sum; the kernel adds a workgroup's four samples before its one atomic
    for the same reason.)  stats[0]: each sample's loss is
    within the loss bar, and the 2 B of them are summed in fp32 in any order, so
    |err| <= 2 B bar + (2 B + 8) u sum|loss_b|; stats[1] is exact."""
    L, lib = _lib()
    g = torch.Generator().manual_seed(500 + Cn)
    for B in (1, 3, 4, 5, 129):
        for fam, mul, add in (("randn4", 4.0, 0.0), ("randn30", 30.0, 0.0), ("plus100", 4.0, 100.0)):
            X = torch.randn(B, Cn, generator=g) * mul + add
            am = X.argmax(1)
            X[torch.arange(B), am] += 1.0
            x64 = X.double()
            second = x64.clone()
            second[torch.arange(B), am] = -float("inf")
            y_off = second.argmax(1) if Cn > 1 else am.clone()
            y_mix = torch.where(torch.arange(B) % 2 == 0, am, y_off)
            bar = 2.0 ** -22 * max(1.0, float(X.abs().max())) + 1e-6
            Xd = X.to(dev)
            stats = torch.zeros(2, device=dev)
            tot, tot_abs, hits = 0.0, 0.0, 0
            for y, gs in ((am, 1.0), (y_mix, 0.5)):
                what = f"ce C={Cn} B={B} {fam} gs={gs}"
                li, dref = _ce_ref(x64, y, gs)
                loss = torch.full((1,), float("nan"), device=dev)
                dl = torch.full((B, Cn), float("nan"), device=dev)
                L.check(lib.pca_cross_entropy(Xd.data_ptr(), y.to(dev).data_ptr(), B, Cn, gs,
                                              loss.data_ptr(), dl.data_ptr(), stats.data_ptr(), None))
                err = abs(float(loss) - float(li.mean()))
                assert err <= bar, f"{what}: loss {float(loss)!r} vs {float(li.mean())!r}: {err:.3e} > {bar:.3e}"
                close(dl, dref, 1e-6, what + " dlogits")
                tot += float(li.sum())
                tot_abs += float(li.abs().sum())
                hits += int((y == am).sum())
            st = stats.cpu().double()
            assert float(st[1]) == float(hits), (Cn, B, fam, float(st[1]), hits)
            sbar = 2 * B * bar + (2 * B + 8) * U * tot_abs
            assert abs(float(st[0]) - tot) <= sbar, (Cn, B, fam, float(st[0]), tot, sbar)
            # dlogits = NULL, stats = NULL: the loss alone
            li, _ = _ce_ref(x64, y_mix, 1.0)
            loss = torch.full((1,), float("nan"), device=dev)
            L.check(lib.pca_cross_entropy(Xd.data_ptr(), y_mix.to(dev).data_ptr(), B, Cn, 1.0,
                                          loss.data_ptr(), None, None, None))
            err = abs(float(loss) - float(li.mean()))
            assert err <= bar, f"ce C={Cn} B={B} {fam} dlogits=NULL: {err:.3e} > {bar:.3e}"
