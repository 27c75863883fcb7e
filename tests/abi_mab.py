"""Direct calls of the MAB entry points (include/pca_hip.h: pca_mab_fwd / pca_mab_bwd) with explicit
``MabShape``s, and the judges of their write / accumulate contract.  TEST INFRASTRUCTURE ONLY.

The autograd glue (pca_hip.ops._MabFn) zero-fills the gradients, allocates dQ / dK with torch.empty,
always passes dk_accumulate = 0 and fp32 activations, so a kernel that overwrites where it should add
(or adds where it should write) passes every module test.  Here every output is prefilled with a
chosen value per call, and every block the library is handed (saved, forward and backward scratch,
every output) is filled with 0xFF bytes - NaN in fp32 and in bf16 - and followed directly by a 0xA5 guard
region that ``Arena.check`` verifies after a synchronisation.

The judges are plain tensor arithmetic, checked on the CPU by tests/test_abi_contract_host.py:

* ``written_ok``: a written output does not depend on its prefill (NaN vs zero prefill);
* ``accumulated_ok``: acc = P + fresh for the prefill P;
* ``padding_rows_ok``: the gradient rows of keys past k_lengths[b] are exact zeros (written) or
  exactly P (accumulated);
* ``same_or_bar``: bitwise equality where the kind reproduces itself bit for bit, else a bar.
"""
import ctypes as C

import numpy as np
import torch

import grad_bars as gb

POISON = 0xFF           # NaN in fp32 (0xFFFFFFFF) and in bf16 (0xFFFF)
GUARD_BYTE = 0xA5
GUARD = 1 << 12

NAMES = ("fc_q.weight", "fc_q.bias", "fc_k.weight", "fc_k.bias", "fc_v.weight", "fc_v.bias",
         "fc_o.weight", "fc_o.bias")
LN_NAMES = ("ln0.weight", "ln0.bias", "ln1.weight", "ln1.bias")

# fp32 accumulation: acc and P + fresh differ by the rounding of one more addition per element, plus the
# reassociation of a reduction that adds its partial sums onto P in another order (split-K atomics):
# a few ulps of the larger operand.  1e-5 of max|P| + max|fresh| is ~80 ulps of the larger one.
FP32_ACC_TOL = 1e-5
# bf16 accumulation, element-wise: acc = bf16(P + s) for the kernel's fp32 sum s, fresh = bf16(s).  bf16 has an
# 8-bit significand, so one round-to-nearest moves a value by at most 2^-8 of itself, and
# |acc - (P + fresh)| <= 2^-8 |P + s| + 2^-8 |s| <= 2^-7 (|P| + |s|): the bound is TIGHT, with no slack (it is
# reached when both roundings are maximal and of the same sign).  Every bf16 accumulation the library does is
# of this form (d = 256: k_rowstream<2, 1, true, 2> adds the old bf16 value to its fp32 accumulator and packs
# once, csrc/d256_stream.hip).  Measured: 0.89 of the bound for the d = 256 few-queries dK, 0.50 at d = 128.
BF16_ACC_TOL = 2.0 ** -7
# |s| may differ from |fresh| by the reassociation of a kernel whose sums are not reproducible (kind 2 at
# d = 128 forms dK with float atomics: 5e-10 measured at max|dK| ~ 1); those few fp32 ulps of the partial
# sums are covered by an absolute term of 2^-16 max|fresh|, far below the O(max|fresh|) error of an
# overwrite or a lost prefill.
BF16_ACC_ABS = 2.0 ** -16


def _bits(t):
    t = t.detach().contiguous()
    if t.dtype == torch.bfloat16:
        return t.view(torch.int16)
    if t.dtype == torch.float32:
        return t.view(torch.int32)
    return t.view(torch.int64) if t.dtype == torch.float64 else t


def bit_equal(a, b):
    a, b = a.detach().cpu(), b.detach().cpu()
    return a.shape == b.shape and a.dtype == b.dtype and torch.equal(_bits(a), _bits(b))


def _f64(t):
    return t.detach().to("cpu", torch.float64)


def written_ok(got_nan_prefill, got_zero_prefill, exact=True, bar=gb.PEER, what=""):
    """A written output: both results finite (every element written), and equal - bitwise when
    ``exact``, else within ``bar``.  Returns the list of violations (empty: the contract holds)."""
    bad = []
    for nm, t in (("NaN", got_nan_prefill), ("zero", got_zero_prefill)):
        if not bool(torch.isfinite(_f64(t)).all()):
            n = int((~torch.isfinite(_f64(t))).sum())
            bad.append(f"{what}: {n} non-finite elements after a {nm} prefill (not written, or NaN inputs)")
    if bad:
        return bad
    if exact:
        if not bit_equal(got_nan_prefill, got_zero_prefill):
            d = float((_f64(got_nan_prefill) - _f64(got_zero_prefill)).abs().max())
            bad.append(f"{what}: depends on its prefill (max |diff| {d:.3e}, bitwise equality demanded)")
        return bad
    e = gb.errors(_f64(got_nan_prefill), _f64(got_zero_prefill))
    return [f"{what}: prefill dependence: {v}" for v in gb.verdict(e, bar)]


def accumulated_ok(acc, P, fresh, dtype=torch.float32, what=""):
    """An accumulated output: acc = P + fresh, for the prefill P and the result ``fresh`` of the same
    call with a zero prefill.  fp32: max|acc - (P + fresh)| <= FP32_ACC_TOL (max|P| + max|fresh|);
    bf16: |acc - (P + fresh)| <= BF16_ACC_TOL (|P| + |fresh|) + BF16_ACC_ABS max|fresh| for every element."""
    a, p, f = _f64(acc), _f64(P), _f64(fresh)
    if a.shape != p.shape or a.shape != f.shape:
        return [f"{what}: shapes {tuple(a.shape)} / {tuple(p.shape)} / {tuple(f.shape)}"]
    if not bool(torch.isfinite(a).all()):
        return [f"{what}: {int((~torch.isfinite(a)).sum())} non-finite elements"]
    err = (a - (p + f)).abs()
    if a.numel() == 0:
        return []
    if dtype == torch.bfloat16:
        lim = BF16_ACC_TOL * (p.abs() + f.abs()) + BF16_ACC_ABS * float(f.abs().max())
        over = err > lim
        if bool(over.any()):
            r = float((err / lim.clamp_min(1e-300)).max())
            return [f"{what}: {int(over.sum())} of {a.numel()} elements off P + fresh (worst "
                    f"{r:.2e} x the bf16 bound {BF16_ACC_TOL:g} (|P| + |fresh|))"]
        return []
    lim = FP32_ACC_TOL * (float(p.abs().max()) + float(f.abs().max()))
    worst = float(err.max())
    if not worst <= lim:
        return [f"{what}: max|acc - (P + fresh)| {worst:.3e} > {FP32_ACC_TOL:g} (max|P| + max|fresh|) = {lim:.3e}"]
    return []


def acc_ratio(acc, P, fresh, dtype=torch.float32):
    """The measured fraction of the accumulation bound that ``acc`` uses (for the record)."""
    a, p, f = _f64(acc), _f64(P), _f64(fresh)
    err = (a - (p + f)).abs()
    if a.numel() == 0:
        return 0.0
    if dtype == torch.bfloat16:
        lim = BF16_ACC_TOL * (p.abs() + f.abs()) + BF16_ACC_ABS * float(f.abs().max())
        return float((err / lim.clamp_min(1e-300)).max())
    return float(err.max()) / (FP32_ACC_TOL * (float(p.abs().max()) + float(f.abs().max())))


def padding_rows_ok(got, lengths, expect=None, what=""):
    """Rows of a [B, nk, .] key gradient at and past lengths[b]: exact zeros (``expect`` None, a written
    output) or bitwise the rows of ``expect`` (the prefill of an accumulated one)."""
    bad = []
    got = got.detach().cpu()
    for b, n in enumerate(int(v) for v in lengths):
        g = got[b, n:]
        if expect is None:
            same = g.to(torch.float64) == 0
        else:
            same = _bits(g) == _bits(expect.detach().cpu()[b, n:])
        if not bool(same.all()):
            rows = int((~same).reshape(g.shape[0], -1).any(1).sum())
            bad.append(f"{what}: set {b}: {rows} of the {g.shape[0]} rows past length {n} are not "
                       f"{'exact zeros' if expect is None else 'the untouched prefill'}")
    return bad


def same_or_bar(got, ref, reproducible, bar, what="", scale=None):
    """Results that the contract says must not depend on something (a prefill, a NULL output): bitwise
    equal when the kind reproduces itself bit for bit, else within the kind's ``bar`` (relative to
    ``scale`` instead of max|ref| for a tensor that is zero up to noise, as grad_bars.NOISE judges it)."""
    if reproducible:
        if bit_equal(got, ref):
            return []
        d = float((_f64(got) - _f64(ref)).abs().max()) if got.shape == ref.shape else float("nan")
        return [f"{what}: not bitwise equal (max |diff| {d:.3e}) although the kind is reproducible"]
    e = gb.errors(_f64(got), _f64(ref), scale)
    return [f"{what}: {v}" for v in gb.verdict(e, bar, norm=scale is None)]


# ---- float64 oracle --------------------------------------------------------------------------------
def oracle(Q, K, p, h, dY, q_shared, lengths=None):
    """Y and every gradient of sum(Y * dY) in float64 (autograd of oracle/st_oracle.py:mab_forward, the
    restatement of the reference MAB).  With ``lengths`` each set runs on its first lengths[b] keys, as
    the ABI promises; the gradient rows of the others are zero.  dQ of a shared query is summed over the
    sets.  Returns {"Y", "dQ", "dK", <parameter names>}."""
    from oracle import st_oracle as orc
    B, nk = K.shape[0], K.shape[1]
    Qd = Q.detach().double().requires_grad_(True)
    Kd = K.detach().double().requires_grad_(True)
    leaves = {k: v.detach().double().requires_grad_(True) for k, v in p.items()}
    Qb = Qd.expand(B, -1, -1) if q_shared else Qd
    if lengths is None:
        Y = orc.mab_forward(Qb, Kd, leaves, h)
    else:
        Y = torch.cat([orc.mab_forward(Qb[b:b + 1], Kd[b:b + 1, :int(n)], leaves, h)
                       for b, n in enumerate(lengths)])
    (Y * dY.detach().double()).sum().backward()
    out = {"Y": Y.detach(), "dQ": Qd.grad, "dK": Kd.grad}
    out.update({k: v.grad if v.grad is not None else torch.zeros_like(v) for k, v in leaves.items()})
    return out


# ---- device side -----------------------------------------------------------------------------------
class Arena:
    """Device blocks filled with POISON, each followed by a GUARD-byte region of GUARD_BYTE."""

    def __init__(self, dev):
        self.dev = dev
        self.guards = []

    def block(self, nbytes):
        """nbytes POISON bytes; the guard starts right after the last one, so a write one element past the
        end of a tensor of any size is caught."""
        n = max(int(nbytes), 1)
        full = torch.empty(n + GUARD, dtype=torch.uint8, device=self.dev)
        full[:n] = POISON
        full[n:] = GUARD_BYTE
        self.guards.append(full[n:])
        return full[:n]

    def tensor(self, shape, dtype, fill=None):
        """A tensor followed directly by its guard; ``fill``: None (POISON bytes), a number, or a tensor to copy."""
        shape = tuple(shape)
        n = int(np.prod(shape)) if shape else 1
        es = torch.tensor([], dtype=dtype).element_size()
        t = self.block(n * es)[:n * es].view(dtype).view(shape)
        if isinstance(fill, torch.Tensor):
            t.copy_(fill.to(dtype))
        elif fill is not None:
            t.fill_(fill)
        return t

    def check(self):
        """Violations of the guard regions (after a synchronisation)."""
        if torch.device(self.dev).type == "cuda":
            torch.cuda.synchronize()
        return [f"guard region {i} overwritten" for i, g in enumerate(self.guards)
                if not bool((g == GUARD_BYTE).all())]


def _dt(code):
    from pca_hip import _lib
    return torch.bfloat16 if code == _lib.PCA_BF16 else torch.float32


def mab_params(dq, dk, d, seed, ln=False):
    """nn.Linear-like initialisation (U(-1/sqrt(din), 1/sqrt(din))), fp32 on the CPU."""
    g = torch.Generator().manual_seed(seed)
    p = {}
    for nm, din in (("fc_q", dq), ("fc_k", dk), ("fc_v", dk), ("fc_o", d)):
        bound = 1.0 / np.sqrt(din)
        p[nm + ".weight"] = (torch.rand(d, din, generator=g) * 2 - 1) * bound
        p[nm + ".bias"] = (torch.rand(d, generator=g) * 2 - 1) * bound
    if ln:
        for nm in ("ln0", "ln1"):
            p[nm + ".weight"] = 1 + 0.2 * torch.randn(d, generator=g)
            p[nm + ".bias"] = 0.2 * torch.randn(d, generator=g)
    return p


class Mab:
    """One pca_mab shape with its inputs, parameters and output gradient, on the CPU (the values the
    device holds: bf16 activations are rounded) and on the device."""

    def __init__(self, dev, B, nq, nk, dq, dk, d, h, q_shared, mode, q_dtype=0, k_dtype=0, y_dtype=0,
                 lengths=None, ln=False, seed=0):
        from pca_hip import _lib
        self.dev, self.L = dev, _lib.lib()
        self.B, self.nq, self.nk, self.dq, self.dk, self.d, self.h = B, nq, nk, dq, dk, d, h
        self.q_shared, self.ln = bool(q_shared), bool(ln)
        self.qt, self.kt, self.yt = _dt(q_dtype), _dt(k_dtype), _dt(y_dtype)
        self.lengths = None if lengths is None else [int(v) for v in lengths]
        g = torch.Generator().manual_seed(1000 + seed)
        self.p = mab_params(dq, dk, d, seed, ln)
        Q = torch.randn(nq, dq, generator=g) * 0.5 if q_shared else torch.randn(B, nq, dq, generator=g)
        K = torch.randn(B, nk, dk, generator=g)
        for X, w in ((Q, dq), (K, dk)):
            if w <= 4:
                X[..., -1] = X[..., -1] * 3 - 9          # log-magnitude-like column
        self.Q = Q.to(self.qt).float()
        self.K = K.to(self.kt).float()
        self.dY = torch.randn(B, nq, d, generator=g).to(self.yt).float()
        self.Qd = self.Q.to(dev).to(self.qt).contiguous()
        self.Kd = self.K.to(dev).to(self.kt).contiguous()
        self.dYd = self.dY.to(dev).to(self.yt).contiguous()
        self.names = NAMES + (LN_NAMES if ln else ())
        self.pd = {k: v.to(dev).contiguous() for k, v in self.p.items()}
        self.kl = None if lengths is None else torch.tensor(self.lengths, dtype=torch.int32, device=dev)
        self.s = _lib.MabShape(B, nq, nk, dq, dk, d, h, int(q_shared), mode, q_dtype, k_dtype, y_dtype,
                               None if self.kl is None else self.kl.data_ptr(), int(ln))
        self.pp = _lib.MabParams(*[self.pd[k].data_ptr() for k in NAMES],
                                 *[self.pd[k].data_ptr() if ln else None for k in LN_NAMES])

    # sizes ------------------------------------------------------------------------------------------
    def saved_bytes(self):
        return int(self.L.pca_mab_saved_bytes(C.byref(self.s)))

    def fwd_ws_bytes(self):
        return int(self.L.pca_mab_fwd_ws_bytes(C.byref(self.s)))

    def bwd_ws_bytes(self):
        return int(self.L.pca_mab_bwd_ws_bytes(C.byref(self.s)))

    def error(self):
        m = self.L.pca_last_error()
        return m.decode() if m else ""

    # shapes of the outputs ---------------------------------------------------------------------------
    def dq_shape(self):
        return (self.nq, self.dq) if self.q_shared else (self.B, self.nq, self.dq)

    def dq_dtype(self):
        return torch.float32 if self.q_shared else self.qt

    def dk_shape(self):
        return (self.B, self.nk, self.dk)

    def grad_shapes(self):
        return [(k, tuple(self.p[k].shape)) for k in self.names]

    # calls ------------------------------------------------------------------------------------------
    def fwd(self, ar, y_fill=float("nan"), train=True):
        """(rc, Y, saved): Y prefilled with ``y_fill``; saved (None for inference) and the scratch
        block poisoned."""
        Y = ar.tensor((self.B, self.nq, self.d), self.yt, y_fill)
        saved = ar.block(self.saved_bytes()) if train else None
        ws = ar.block(self.fwd_ws_bytes())
        rc = self.L.pca_mab_fwd(C.byref(self.s), self.Qd.data_ptr(), self.Kd.data_ptr(), C.byref(self.pp),
                                Y.data_ptr(), None if saved is None else saved.data_ptr(), ws.data_ptr(), None)
        return rc, Y, saved

    def bwd(self, ar, saved, dq_fill=None, dk_fill=None, dk_accumulate=0, g_fill=0.0, want_dq=True,
            want_dk=True):
        """One backward with every output prefilled: dQ with ``dq_fill``, dK with ``dk_fill``, each
        gradient with ``g_fill`` (a number, or {name: tensor}); the scratch block poisoned.
        Returns (rc, {"dQ", "dK", <names>}) - dQ / dK None when not requested (NULL)."""
        out = {}
        for k, shp in self.grad_shapes():
            f = g_fill[k] if isinstance(g_fill, dict) else g_fill
            out[k] = ar.tensor(shp, torch.float32, f)
        out["dQ"] = ar.tensor(self.dq_shape(), self.dq_dtype(), dq_fill) if want_dq else None
        out["dK"] = ar.tensor(self.dk_shape(), self.kt, dk_fill) if want_dk else None
        from pca_hip import _lib
        gg = _lib.MabGrads(*[out[k].data_ptr() for k in NAMES],
                           *[out[k].data_ptr() if self.ln else None for k in LN_NAMES])
        ws = ar.block(self.bwd_ws_bytes())
        rc = self.L.pca_mab_bwd(C.byref(self.s), self.Qd.data_ptr(), self.Kd.data_ptr(), C.byref(self.pp),
                                saved.data_ptr(), self.dYd.data_ptr(),
                                None if out["dQ"] is None else out["dQ"].data_ptr(),
                                None if out["dK"] is None else out["dK"].data_ptr(),
                                int(dk_accumulate), C.byref(gg), ws.data_ptr(), None)
        return rc, out

    def oracle(self):
        return oracle(self.Q, self.K, self.p, self.h, self.dY, self.q_shared, self.lengths)

    def emulation(self, kind):
        """Y and every gradient of sum(Y * dY) from the operand-rounding emulation of a fused kind (autograd
        in fp32, as tests/test_gpu_bf16.py uses it): kind 1 oracle/st_oracle.py:mab1_forward_bf16emu, kind 2
        tests/emu.py:mab0_forward_bf16emu (per set on its first k_lengths[b] keys).  The inputs are the
        values the device holds (bf16 activations rounded), so the emulation has the kernels' ReLU masks."""
        from emu import mab0_forward_bf16emu
        from oracle import st_oracle as orc
        Q = self.Q.clone().requires_grad_(True)
        K = self.K.clone().requires_grad_(True)
        leaves = {k: v.clone().requires_grad_(True) for k, v in self.p.items()}
        if kind == 1:
            assert not self.q_shared and self.lengths is None
            Y = orc.mab1_forward_bf16emu(Q, K, leaves, self.h)
        elif kind == 2:
            assert self.q_shared
            lens = [self.nk] * self.B if self.lengths is None else self.lengths
            Y = torch.cat([mab0_forward_bf16emu(Q[None], K[b:b + 1, :n], leaves, self.h)
                           for b, n in enumerate(lens)])
        else:
            raise ValueError(f"no emulation of kind {kind}")
        (Y * self.dY).sum().backward()
        out = {"Y": Y.detach(), "dQ": Q.grad, "dK": K.grad}
        out.update({k: v.grad if v.grad is not None else torch.zeros_like(v) for k, v in leaves.items()})
        return out


def prefill_like(fresh, seed, scale=None, dtype=torch.float32):
    """P = randn x max|fresh| (or ``scale``), in the dtype of the output it is written into."""
    g = torch.Generator().manual_seed(seed)
    f = _f64(fresh)
    S = float(f.abs().max()) if scale is None else float(scale)
    if not S > 0:
        S = 1.0
    return (torch.randn(f.shape, generator=g, dtype=torch.float64) * S).to(dtype)
