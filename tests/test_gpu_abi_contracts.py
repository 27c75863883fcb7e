"""The write / accumulate contract of the MAB entry points (include/pca_hip.h: pca_mab_fwd / pca_mab_bwd),
called directly for every kernel kind, plus the small contracts of pca_linear_* and pca_cross_entropy.

Per shape of ``CASES`` (the kind it resolves to is asserted: tests/dispatch.py's launch counters where a
family identifies the kind, the size queries otherwise), with every block poisoned and guarded
(tests/abi_mab.py):

1. the first backward (written outputs NaN-prefilled, accumulated ones zero) and the forward match the
   float64 oracle, each tensor on its own scale (grad_bars: F32 for the exact kinds, BF16_VS_ORACLE for the
   fused ones; fc_k.bias on the scale of fc_q.bias), and for kinds 1 / 2 the emulation of their operand
   roundings under the tighter measured bar ``EMU``;
2. a second backward with every accumulated output prefilled with P gives P + fresh: the 8 (12 with ln)
   weight and bias gradients, dQ of a shared query, dK with dk_accumulate = 1;
3. written outputs (Y, dQ of per-set queries, dK with dk_accumulate = 0) do not depend on their prefill;
4. gradient rows of keys past k_lengths[b] are exact zeros (written) or exactly P (accumulated);
5. dQ = NULL and / or dK = NULL leave the weight gradients unchanged;
6. an input gradient a fused layer-1 kernel does not build is refused with PCA_EUNSUPPORTED and a message,
   every output untouched;
7. every result is finite with 0xFF-poisoned scratch, and every guard region is intact.

"Unchanged" and "does not depend" are bitwise for the kinds that are bitwise reproducible (``_reproducible``:
declared per kind, and a declared kind that gives two different results for one call fails), within the
kind's bar for the others.
"""
import ctypes as C

import numpy as np
import pytest
import torch

import abi_mab as am
import grad_bars as gb
from dispatch import launches

pytestmark = pytest.mark.gpu

NAN = float("nan")
F32, BF16 = 0, 1                     # PCA_F32 / PCA_BF16
M_F32, M_BF16 = 0, 1                 # PCA_MODE_F32 / PCA_MODE_BF16
EUNSUPPORTED = -2


@pytest.fixture(scope="module")
def dev():
    import pca_hip
    pca_hip.lib()
    yield torch.device("cuda", 0)
    pca_hip.set_mode("f32")


# id: (kind, (B, nq, nk, dq, dk, d, h, q_shared), mode, (q, k, y dtypes), k_lengths, ln, refused gradient)
CASES = {
    "k0": (0, (3, 37, 19, 5, 7, 16, 2, 0), M_F32, (F32, F32, F32), None, 0, None),
    "k0_qshared": (0, (3, 4, 50, 16, 7, 16, 2, 1), M_F32, (F32, F32, F32), None, 0, None),
    "k0_lengths": (0, (3, 37, 19, 5, 7, 16, 2, 0), M_F32, (F32, F32, F32), [19, 1, 7], 0, None),
    "k0_ln": (0, (3, 37, 19, 5, 7, 16, 2, 0), M_F32, (F32, F32, F32), None, 1, None),
    "k1_d128": (1, (3, 200, 16, 128, 128, 128, 4, 0), M_BF16, (F32, F32, F32), None, 0, None),
    "k1_d128_bf16": (1, (3, 200, 16, 128, 128, 128, 4, 0), M_BF16, (BF16, F32, BF16), None, 0, None),
    "k1_d256": (1, (2, 300, 32, 256, 256, 256, 8, 0), M_BF16, (F32, F32, F32), None, 0, None),
    "k1_d256_bf16": (1, (2, 300, 32, 256, 256, 256, 8, 0), M_BF16, (BF16, F32, BF16), None, 0, None),
    "k1_d128_layer1": (1, (2, 77, 16, 2, 128, 128, 4, 0), M_BF16, (F32, F32, F32), None, 0, "dQ"),
    "k1_d256_layer1": (1, (2, 77, 32, 2, 256, 256, 8, 0), M_BF16, (F32, F32, F32), None, 0, "dQ"),
    "k2_d128": (2, (3, 16, 200, 128, 128, 128, 4, 1), M_BF16, (F32, F32, F32), None, 0, None),
    "k2_d128_bf16": (2, (3, 16, 200, 128, 128, 128, 4, 1), M_BF16, (F32, BF16, F32), None, 0, None),
    "k2_d128_lengths": (2, (3, 16, 200, 128, 128, 128, 4, 1), M_BF16, (F32, F32, F32), [200, 1, 77], 0, None),
    "k2_d128_bf16_lengths": (2, (3, 16, 200, 128, 128, 128, 4, 1), M_BF16, (F32, BF16, F32), [130, 200, 3], 0,
                             None),
    "k2_d128_pma": (2, (4, 1, 130, 128, 128, 128, 4, 1), M_BF16, (F32, F32, F32), None, 0, None),
    "k2_d128_layer1": (2, (3, 16, 150, 128, 2, 128, 4, 1), M_BF16, (F32, F32, F32), None, 0, "dK"),
    "k2_d256": (2, (2, 32, 300, 256, 256, 256, 8, 1), M_BF16, (F32, F32, F32), None, 0, None),
    "k2_d256_bf16": (2, (2, 32, 300, 256, 256, 256, 8, 1), M_BF16, (F32, BF16, F32), None, 0, None),
    "k2_d256_pma": (2, (3, 1, 130, 256, 256, 256, 8, 1), M_BF16, (F32, F32, F32), None, 0, None),
    "k2_d256_layer1": (2, (2, 32, 300, 256, 3, 256, 8, 1), M_BF16, (F32, F32, F32), None, 0, "dK"),
    "k4": (4, (2, 150, 150, 128, 128, 128, 4, 0), M_BF16, (F32, F32, F32), None, 0, None),
    "k4_lengths": (4, (2, 150, 150, 128, 128, 128, 4, 0), M_BF16, (F32, F32, F32), [150, 37], 0, None),
    "k4_dh16": (4, (2, 150, 150, 64, 64, 64, 4, 0), M_BF16, (F32, F32, F32), None, 0, None),
}


def _bar(kind):
    return gb.F32 if kind in (0, 3) else gb.BF16_VS_ORACLE


def _peer(kind):
    """Bar of two runs of the same arithmetic that are not bitwise reproducible."""
    return gb.F32 if kind in (0, 3) else gb.PEER


# Fused kinds 1 / 2 against the emulation of their operand roundings (tests/abi_mab.py: Mab.emulation), which
# has the kernels' rounding points.  Measured on an MI355X over the 16 kind-1 / kind-2 cases, outside fc_o.*:
# max 1.2e-1 (dQ), rms 8.2e-3, 2.0e-3 of the elements beyond 4e-2, norm 2.3e-2; a few wrong rows of dQ or dK
# (0.5 % of the elements at nq or nk = 200) exceed both the outlier fraction and the norm ratio.
EMU = gb.Bar(tol=4e-2, tol_n=4e-2, outlier_frac=2.5e-3, cap=4.0)
# fc_o.weight / fc_o.bias: a ReLU of the block's epilogue whose pre-activation the kernel and the emulation
# round to opposite sides of zero moves a whole element of dZ, i.e. a few of the d elements of fc_o.bias.
# Measured: max 1.9e-1, 2.3e-2 of the elements of fc_o.bias beyond 4e-2 (3 of 128, k2_d128_bf16_lengths: 48
# query rows; 4 of 256 for k1_d256_bf16), norm 5.0e-2.  grad_bars.BF16_VS_EMU with room for those few flips.
EMU_FC_O = gb.Bar(tol=4e-2, tol_n=1e-1, outlier_frac=3e-2, cap=10.0)


def _emu_record(cid, got, emu, shapes):
    """Worst own-scale figures of one case against its emulation (fc_k.bias on the scale of fc_q.bias)."""
    w = dict(max=0.0, rms=0.0, norm=0.0, f1=0.0, f15=0.0)
    for k, _ in shapes:
        sc = float(emu["fc_q.bias"].abs().max()) if k == "fc_k.bias" else None
        e = gb.errors(got[k].float(), emu[k], sc)
        w["max"], w["rms"] = max(w["max"], e["max"]), max(w["rms"], e["rms"])
        if sc is None:
            w["norm"] = max(w["norm"], e["norm"])
        w["f1"] = max(w["f1"], float(np.mean(e["d"] > 1e-2)))
        w["f15"] = max(w["f15"], float(np.mean(e["d"] > 1.5e-2)))
    print(f"EMU {cid}: max {w['max']:.2e} rms {w['rms']:.2e} norm {w['norm']:.2e} "
          f"beyond 1e-2 {w['f1']:.2e} beyond 1.5e-2 {w['f15']:.2e}")


def _reproducible(kind, d):
    """Kinds whose backward is bitwise reproducible by construction: kind 4 (csrc/wgrad_rows.hip: per-workgroup
    slabs reduced in a fixed order), and measured so on every call of this file: kind 1, kind 2 at d = 256.
    The exact chain (split-K float atomics) and kind 2 at d = 128 (fc_k.weight and dK) are not; for them a
    pair of equal runs proves nothing, so "unchanged" is judged against the kind's bar."""
    return kind in (1, 4) or (kind == 2 and d == 256)


def _judge(got, ref, bar, shapes, what, bad):
    # a block's own parameter names get a prefix, as in a state_dict (grad_bars.NOISE finds the sibling
    # of fc_k.bias from it)
    nm = lambda k: "blk." + k if k.startswith(("fc_", "ln")) else k
    got, ref = {nm(k): v.float() for k, v in got.items()}, {nm(k): v for k, v in ref.items()}
    shapes = [(nm(k), s) for k, s in shapes]
    try:
        rows = gb.judge(got, ref, bar, shapes, what)
        return max(r["max"] if r["rule"] == "own" else r["max_sib"] for r in rows)
    except AssertionError as e:
        bad.append(str(e))
        return float("nan")


def _witness_kind(m, kind, call):
    """The kind a backward of ``m`` resolves to: launch counters of the fused families and of k_gemm_f32,
    and the size queries (PCA_MODE_BF16 refuses a shape whose kind is the exact chain)."""
    n = launches(call, ("gemm_f32", "mab1_bwd", "mab0_bwd"))
    s = m.s
    if kind == 0:
        assert s.mode == M_F32 and n["gemm_f32"] > 0 and n["mab1_bwd"] == 0 and n["mab0_bwd"] == 0, n
        return n
    assert m.saved_bytes() > 0, m.error()                 # a fused kind: bf16_demand accepted it
    if kind == 1:
        assert n["mab1_bwd"] > 0 and n["mab0_bwd"] == 0, n
    elif kind == 2:
        # (the layer-1 few-queries kernels, dk <= 4, have no launch counter; q_shared leaves no other kind)
        assert s.q_shared == 1 and n["mab1_bwd"] == 0 and (n["mab0_bwd"] > 0 or s.dk <= 4), n
    elif kind == 4:
        assert n["mab1_bwd"] == 0 and n["mab0_bwd"] == 0, n
        f32 = am.Mab(m.dev, s.B, s.nq, s.nk, s.dq, s.dk, s.d, s.h, s.q_shared, M_F32, lengths=m.lengths)
        # the fused attention core never stores the nq x nk scores that the exact chain saves
        assert 0 < m.saved_bytes() < f32.saved_bytes(), (m.saved_bytes(), f32.saved_bytes())
    return n


@pytest.mark.parametrize("cid", list(CASES))
def test_mab_contract(dev, cid):
    kind, shape, mode, dts, lengths, ln, refused = CASES[cid]
    B, nq, nk, dq, dk, d, h, q_shared = shape
    m = am.Mab(dev, *shape, mode, *dts, lengths=lengths, ln=ln, seed=list(CASES).index(cid))
    ar = am.Arena(dev)
    bad = []
    assert m.saved_bytes() > 0 and m.fwd_ws_bytes() > 0 and m.bwd_ws_bytes() > 0, m.error()
    bar, peer = _bar(kind), _peer(kind)
    want_dq, want_dk = refused != "dQ", refused != "dK"
    dq_written = not q_shared

    # forward: Y is written (NaN and zero prefill), reproducibility from a repeat
    rc, Y, saved = m.fwd(ar, NAN)
    assert rc == 0, m.error()
    rc, Y0, _ = m.fwd(ar, 0.0)
    assert rc == 0, m.error()
    rc, Y1, _ = m.fwd(ar, NAN)
    assert rc == 0, m.error()
    torch.cuda.synchronize()
    fwd_repro = am.bit_equal(Y, Y1)
    bad += am.written_ok(Y, Y0, exact=fwd_repro, bar=peer, what="Y")

    def call(dq_fill, dk_fill, acc=0, g_fill=0.0, wq=want_dq, wk=want_dk):
        rc, out = m.bwd(ar, saved, dq_fill=dq_fill, dk_fill=dk_fill, dk_accumulate=acc, g_fill=g_fill,
                        want_dq=wq, want_dk=wk)
        assert rc == 0, f"{cid}: pca_mab_bwd rc={rc}: {m.error()}"
        return out

    fresh_fill = dict(dq_fill=NAN if dq_written else 0.0, dk_fill=NAN)
    fresh = call(**fresh_fill)
    again = call(**fresh_fill)
    torch.cuda.synchronize()
    outs = list(m.names) + [k for k, w in (("dQ", want_dq), ("dK", want_dk)) if w]
    measured = all(am.bit_equal(fresh[k], again[k]) for k in outs)
    repro = _reproducible(kind, d)
    if repro and not measured:
        bad += [f"{k}: two identical calls differ" for k in outs if not am.bit_equal(fresh[k], again[k])]
    # fc_k.bias is zero up to noise (softmax shift invariance): judged on the scale of fc_q.bias
    sc = {k: float(fresh["fc_q.bias"].abs().max()) if k == "fc_k.bias" else None for k in m.names}

    # 1. fresh result vs the float64 oracle
    ref = m.oracle()
    got = {"Y": Y, **{k: fresh[k] for k in outs}}
    shapes = [("Y", (B, nq, d))] + m.grad_shapes()
    shapes += [(k, tuple(fresh[k].shape)) for k in ("dQ", "dK") if k in outs]
    worst = _judge(got, {k: ref[k] for k, _ in shapes}, bar, shapes, f"{cid} vs oracle", bad)
    worst_emu = float("nan")
    if kind in (1, 2):      # and tightly against the emulation of the kind's operand roundings
        emu = m.emulation(kind)
        tight = [(k, sh) for k, sh in shapes if not k.startswith("fc_o.")]
        epi = [(k, sh) for k, sh in shapes if k.startswith("fc_o.")]
        worst_emu = _judge(got, {k: emu[k] for k, _ in tight}, EMU, tight, f"{cid} vs emulation", bad)
        _judge(got, {k: emu[k] for k, _ in epi}, EMU_FC_O, epi, f"{cid} fc_o vs emulation", bad)
        _emu_record(cid, got, emu, shapes)

    # 2. accumulation: every accumulated output prefilled with P
    sk = float(fresh["fc_k.weight"].abs().max())
    P = {k: am.prefill_like(fresh[k].float(), 7 + i, scale=sk if k == "fc_k.bias" else None)
         for i, k in enumerate(m.names)}
    Pq = am.prefill_like(fresh["dQ"].float(), 31, dtype=m.dq_dtype()) if want_dq else None
    Pk = am.prefill_like(fresh["dK"].float(), 37, dtype=m.kt) if want_dk else None
    acc = call(Pq, Pk, acc=1, g_fill={k: v.to(dev) for k, v in P.items()})
    torch.cuda.synchronize()
    ratios = {}
    for k in m.names:
        bad += am.accumulated_ok(acc[k], P[k], fresh[k], torch.float32, f"{k} accumulated")
        ratios[k] = am.acc_ratio(acc[k], P[k], fresh[k])
    if want_dq:
        if dq_written:      # 3. written under a random prefill as well
            bad += am.same_or_bar(acc["dQ"], fresh["dQ"], repro, peer, "dQ (written) after a random prefill")
        else:
            bad += am.accumulated_ok(acc["dQ"], Pq, fresh["dQ"], torch.float32, "dQ (shared) accumulated")
            ratios["dQ"] = am.acc_ratio(acc["dQ"], Pq, fresh["dQ"])
    if want_dk:
        bad += am.accumulated_ok(acc["dK"], Pk, fresh["dK"], m.kt, "dK accumulated (dk_accumulate = 1)")
        ratios["dK"] = am.acc_ratio(acc["dK"], Pk, fresh["dK"], m.kt)

    # 3. written outputs do not depend on their prefill
    zero = call(0.0, 0.0)
    torch.cuda.synchronize()
    if want_dq and dq_written:
        bad += am.written_ok(fresh["dQ"], zero["dQ"], exact=repro, bar=peer, what="dQ (written)")
    if want_dk:
        bad += am.written_ok(fresh["dK"], zero["dK"], exact=repro, bar=peer, what="dK (written)")
    for k in m.names:
        bad += am.same_or_bar(zero[k], fresh[k], repro, peer, f"{k} (second zero-prefilled call)", sc[k])

    # 4. padding rows
    if lengths is not None and want_dk:
        bad += am.padding_rows_ok(fresh["dK"], lengths, None, "dK written")
        bad += am.padding_rows_ok(acc["dK"], lengths, Pk, "dK accumulated")

    # 5. NULL input gradients: the weight gradients (and the other input gradient) are unchanged
    variants = {(False, want_dk), (want_dq, False), (False, False)} - {(want_dq, want_dk)}
    for wq, wk in sorted(variants):
        nul = call(fresh_fill["dq_fill"], NAN, wq=wq, wk=wk)
        torch.cuda.synchronize()
        tag = f"dQ {'NULL' if not wq else 'set'}, dK {'NULL' if not wk else 'set'}"
        for k in list(m.names) + [k for k, w in (("dQ", wq), ("dK", wk)) if w]:
            bad += am.same_or_bar(nul[k], fresh[k], repro, peer, f"{k} with {tag}", sc.get(k))

    # 6. a refused input gradient: PCA_EUNSUPPORTED, a message, every output untouched
    if refused is not None:
        g = torch.Generator().manual_seed(5)
        pre = {k: torch.randn(m.p[k].shape, generator=g) for k in m.names}
        pre["dQ"] = torch.randn(m.dq_shape(), generator=g).to(m.dq_dtype())
        pre["dK"] = torch.randn(m.dk_shape(), generator=g).to(m.kt)
        rc, out = m.bwd(ar, saved, dq_fill=pre["dQ"], dk_fill=pre["dK"], dk_accumulate=0,
                        g_fill={k: pre[k].to(dev) for k in m.names}, want_dq=True, want_dk=True)
        msg = m.error()
        torch.cuda.synchronize()
        assert rc == EUNSUPPORTED, (rc, msg)
        assert refused in msg and "not built" in msg, msg
        for k in list(m.names) + ["dQ", "dK"]:
            if not am.bit_equal(out[k].cpu(), pre[k]):
                bad.append(f"refused call wrote {k}")

    # kind witness (after the checks, on fresh buffers of the same call)
    n = _witness_kind(m, kind, lambda: call(**fresh_fill))
    # 7. guards
    bad += ar.check()
    print(f"{cid}: kind {kind} {n}; reproducible fwd {fwd_repro} bwd {measured} (declared {repro}); worst own-scale {worst:.2e} "
          f"(vs emulation {worst_emu:.2e}); "
          f"accumulation bound used: " + " ".join(f"{k}={v:.1e}" for k, v in ratios.items()))
    assert not bad, f"{cid}: {len(bad)} contract violations:\n  " + "\n  ".join(bad)


def test_sd64_inference_kind(dev):
    """Kind 3, the shipped d = 64 / 8-head shape: the inference forward (saved = NULL) runs the fused fp32
    kernel - held to the fp32 bar against the oracle with a poisoned scratch block - while a training call
    of the same shape takes a training kind (the self-attention core, kind 4) instead of refusing."""
    ar = am.Arena(dev)
    m = am.Mab(dev, 2, 64, 64, 64, 64, 64, 8, 0, M_BF16, seed=64)
    assert m.fwd_ws_bytes() > 0 and m.saved_bytes() > 0, m.error()
    ref = m.oracle()
    n = launches(lambda: m.fwd(ar, NAN, train=False), ("gemm_f32", "mab1_fwd", "mab0_fwd"))
    assert all(v == 0 for v in n.values()), n
    rc, Y, _ = m.fwd(ar, NAN, train=False)
    assert rc == 0, m.error()
    rc, Y0, _ = m.fwd(ar, 0.0, train=False)
    assert rc == 0, m.error()
    torch.cuda.synchronize()
    assert am.written_ok(Y, Y0) == []
    gb.own_close(Y, ref["Y"], gb.F32, "kind 3 inference Y vs oracle")
    rc, Yt, saved = m.fwd(ar, NAN, train=True)
    assert rc == 0, m.error()
    rc, out = m.bwd(ar, saved, dq_fill=NAN, dk_fill=NAN)
    assert rc == 0, m.error()
    torch.cuda.synchronize()
    shapes = [("Y", tuple(Yt.shape))] + m.grad_shapes() + [("dQ", m.dq_shape()), ("dK", m.dk_shape())]
    bad = []
    _judge({"Y": Yt, **{k: out[k] for k, _ in shapes[1:]}}, ref, gb.BF16_VS_ORACLE, shapes,
           "sd64 shape, training call", bad)
    assert not bad, bad
    assert ar.check() == []


# ---- the d -> d ISAB as scripts/isab256_fwdbwd_bench.py runs it ------------------------------------------
def _isab_run(dev, d, h, m, X, I, dY, p0, p1, io_bf16):
    """mab0 (s0: the shared query I over the keys X) then mab1 (s1: X over H), forward with saved blocks,
    then mab1's backward (dX written, dH written) and mab0's (dI accumulated, dX accumulated with
    dk_accumulate = 1).  io_bf16: X, Y and dY cross the ABI in bf16 (s0 k_dtype, s1 q_dtype / y_dtype)."""
    from pca_hip import _lib
    L = _lib.lib()
    ar = am.Arena(dev)
    B, N = X.shape[:2]
    at = BF16 if io_bf16 else F32
    tt = torch.bfloat16 if io_bf16 else torch.float32
    s0 = _lib.MabShape(B, m, N, d, d, d, h, 1, M_BF16, F32, at, F32, None, 0)
    s1 = _lib.MabShape(B, N, m, d, d, d, h, 0, M_BF16, at, F32, at, None, 0)
    Xd, Id, dYd = X.to(dev).to(tt), I.to(dev), dY.to(dev).to(tt)
    pd0 = [p0[k].to(dev) for k in am.NAMES]
    pd1 = [p1[k].to(dev) for k in am.NAMES]
    pp0 = _lib.MabParams(*[t.data_ptr() for t in pd0], None, None, None, None)
    pp1 = _lib.MabParams(*[t.data_ptr() for t in pd1], None, None, None, None)
    g0 = [ar.tensor(tuple(t.shape), torch.float32, 0.0) for t in pd0]
    g1 = [ar.tensor(tuple(t.shape), torch.float32, 0.0) for t in pd1]
    gg0 = _lib.MabGrads(*[t.data_ptr() for t in g0], None, None, None, None)
    gg1 = _lib.MabGrads(*[t.data_ptr() for t in g1], None, None, None, None)
    sizes = []
    for s in (s0, s1):
        sizes.append([int(f(C.byref(s))) for f in (L.pca_mab_saved_bytes, L.pca_mab_fwd_ws_bytes,
                                                    L.pca_mab_bwd_ws_bytes)])
        assert all(v > 0 for v in sizes[-1]), L.pca_last_error()
    sv0, sv1 = ar.block(sizes[0][0]), ar.block(sizes[1][0])
    H = ar.tensor((B, m, d), torch.float32, NAN)
    Y = ar.tensor((B, N, d), tt, NAN)
    dX = ar.tensor((B, N, d), tt, NAN)
    dH = ar.tensor((B, m, d), torch.float32, NAN)
    dI = ar.tensor((m, d), torch.float32, 0.0)
    _lib.check(L.pca_mab_fwd(C.byref(s0), Id.data_ptr(), Xd.data_ptr(), C.byref(pp0), H.data_ptr(),
                             sv0.data_ptr(), ar.block(sizes[0][1]).data_ptr(), None), "s0 fwd")
    _lib.check(L.pca_mab_fwd(C.byref(s1), Xd.data_ptr(), H.data_ptr(), C.byref(pp1), Y.data_ptr(),
                             sv1.data_ptr(), ar.block(sizes[1][1]).data_ptr(), None), "s1 fwd")
    _lib.check(L.pca_mab_bwd(C.byref(s1), Xd.data_ptr(), H.data_ptr(), C.byref(pp1), sv1.data_ptr(),
                             dYd.data_ptr(), dX.data_ptr(), dH.data_ptr(), 0, C.byref(gg1),
                             ar.block(sizes[1][2]).data_ptr(), None), "s1 bwd")
    _lib.check(L.pca_mab_bwd(C.byref(s0), Id.data_ptr(), Xd.data_ptr(), C.byref(pp0), sv0.data_ptr(),
                             dH.data_ptr(), dI.data_ptr(), dX.data_ptr(), 1, C.byref(gg0),
                             ar.block(sizes[0][2]).data_ptr(), None), "s0 bwd")
    torch.cuda.synchronize()
    assert ar.check() == []
    out = {"Y": Y.float().cpu(), "dX": dX.float().cpu(), "enc.0.I": dI.cpu()}
    for pre, gs in (("enc.0.mab0.", g0), ("enc.0.mab1.", g1)):
        out.update({pre + k: t.cpu() for k, t in zip(am.NAMES, gs)})
    return out


@pytest.mark.parametrize("d,h,m", [(256, 8, 32), (128, 4, 16)], ids=["d256", "d128"])
@pytest.mark.parametrize("N", [256, 300])
def test_isab_fwd_bwd_bf16_io(dev, d, h, m, N):
    """The north-star ISAB unit with bf16 activations at the ABI: Y, dX, dI and the 16 weight and bias
    gradients against a float64 ISAB fed the bf16-rounded X and dY (BF16_VS_ORACLE), and against the same
    chain with fp32 I/O (PEER)."""
    from oracle import st_oracle as orc
    B = 2
    g = torch.Generator().manual_seed(N + d)
    p0, p1 = am.mab_params(d, d, d, seed=N + 1), am.mab_params(d, d, d, seed=N + 2)
    I = torch.randn(m, d, generator=g) * 0.5
    X = torch.randn(B, N, d, generator=g).to(torch.bfloat16).float()
    dY = torch.randn(B, N, d, generator=g).to(torch.bfloat16).float()
    got = _isab_run(dev, d, h, m, X, I, dY, p0, p1, io_bf16=True)
    f32 = _isab_run(dev, d, h, m, X, I, dY, p0, p1, io_bf16=False)
    # float64 oracle
    Xl, Il = X.double().requires_grad_(True), I.double().requires_grad_(True)
    l0 = {k: v.double().requires_grad_(True) for k, v in p0.items()}
    l1 = {k: v.double().requires_grad_(True) for k, v in p1.items()}
    Hr = orc.mab_forward(Il.expand(B, -1, -1), Xl, l0, h)
    Yr = orc.mab_forward(Xl, Hr, l1, h)
    (Yr * dY.double()).sum().backward()
    ref = {"Y": Yr.detach(), "dX": Xl.grad, "enc.0.I": Il.grad}
    for pre, lv in (("enc.0.mab0.", l0), ("enc.0.mab1.", l1)):
        ref.update({pre + k: v.grad for k, v in lv.items()})
    shapes = [(k, tuple(v.shape)) for k, v in got.items()]
    assert len(shapes) == 19          # Y, dX and the 17 parameter gradients (16 weights / biases, I)
    bad = []
    w_or = _judge(got, ref, gb.BF16_VS_ORACLE, shapes, f"ISAB d={d} N={N} bf16 I/O vs oracle", bad)
    w_32 = _judge(f32, ref, gb.BF16_VS_ORACLE, shapes, f"ISAB d={d} N={N} fp32 I/O vs oracle", bad)
    w_pe = _judge(got, f32, gb.PEER, shapes, f"ISAB d={d} N={N} bf16 I/O vs fp32 I/O", bad)
    print(f"ISAB d={d} N={N}: worst own-scale vs oracle {w_or:.2e} (fp32 I/O {w_32:.2e}), vs fp32 I/O {w_pe:.2e}")
    assert not bad, "\n".join(bad)


# ---- layer-1 input gradients through the autograd glue ------------------------------------------------
def _st_case(dev, din, d, h, m):
    import models
    import inputs as gi
    B, N, Cc = 4, 200, 10
    torch.manual_seed(900 + din + d)
    net = models.ST(dim_input=din, num_outputs=1, dim_output=Cc, num_inds=m, dim_hidden=d,
                    num_heads=h).to(dev)
    Xn = torch.from_numpy(gi.pc_input(9000 + din, B, N, din))
    yn = torch.from_numpy(gi.labels(9001 + din, B, Cc))
    return net, Xn, yn


def _st_step(net, Xn, yn, dev, xgrad):
    import pca_hip
    net.zero_grad(set_to_none=True)
    X = Xn.to(dev).requires_grad_(xgrad)
    loss = pca_hip.cross_entropy(net(X), yn.to(dev))
    loss.backward()
    torch.cuda.synchronize()
    out = {k: p.grad.detach().cpu().clone() for k, p in net.named_parameters()}
    if xgrad:
        out["X"] = X.grad.detach().cpu().clone()
    return out


@pytest.mark.parametrize("din,d,h,m", [(2, 128, 4, 16), (3, 256, 8, 32)], ids=["d128", "d256"])
def test_layer1_input_grad_modes(dev, din, d, h, m):
    """models.ST with X.requires_grad: 'auto' runs the layer-1 blocks on the exact chain (the fused ones
    build no dX) and matches the oracle, X.grad included; 'bf16' refuses at the forward naming the shape
    and the gradient; 'f32' is unchanged.  Without X.requires_grad 'auto' still launches the fused layer-1
    kernels."""
    import pca_hip
    from oracle import st_oracle as orc
    net, Xn, yn = _st_case(dev, din, d, h, m)
    leaves = {k: v.detach().cpu().double().requires_grad_(True) for k, v in net.state_dict().items()}
    Xl = Xn.double().requires_grad_(True)
    orc.cross_entropy(orc.st_forward(Xl, leaves, h).reshape(Xn.shape[0], -1), yn).backward()
    ref = {k: v.grad for k, v in leaves.items()}
    ref["X"] = Xl.grad
    shapes = gb.shapes_of(net) + [("X", tuple(Xn.shape))]
    fams = ("gemm_f32", "mab1_fwd", "mab1_bwd", "mab0_bwd")
    try:
        pca_hip.set_mode("auto")
        got = _st_step(net, Xn, yn, dev, True)
        gb.judge(got, ref, gb.BF16_VS_ORACLE, shapes, f"auto, X.requires_grad, d={d}")
        n_x = launches(lambda: _st_step(net, Xn, yn, dev, True), fams)
        n_0 = launches(lambda: _st_step(net, Xn, yn, dev, False), fams)
        # layer 1 leaves the fused kernels only when dX is asked for; layer 2 and the PMA stay fused
        assert n_x["mab1_bwd"] > 0 and n_0["mab1_bwd"] > n_x["mab1_bwd"], (n_x, n_0)
        assert n_0["mab1_fwd"] > n_x["mab1_fwd"] > 0, (n_x, n_0)
        assert n_x["gemm_f32"] > n_0["gemm_f32"], (n_x, n_0)
        pca_hip.set_mode("bf16")
        with pytest.raises(pca_hip.PcaHipError, match=rf"returns dK .*dk={din} d={d}"):
            net(Xn.to(dev).requires_grad_(True))
        _st_step(net, Xn, yn, dev, False)             # without dX the explicit mode trains as before
        pca_hip.set_mode("f32")
        got = _st_step(net, Xn, yn, dev, True)
        gb.judge(got, ref, gb.F32, shapes, f"f32, X.requires_grad, d={d}")
    finally:
        pca_hip.set_mode("f32")
    print(f"layer-1 input grads d={d}: auto with dX {n_x}, without {n_0}")


# ---- pca_linear_fwd / pca_linear_bwd ------------------------------------------------------------------
def _linear(dev, ar, X, W, b, dY, dX_fill, dW_fill, db_fill, want=(True, True, True)):
    from pca_hip import _lib
    L = _lib.lib()
    M, din = X.shape
    dout = W.shape[0]
    dX = ar.tensor((M, din), torch.float32, dX_fill) if want[0] else None
    dW = ar.tensor((dout, din), torch.float32, dW_fill) if want[1] else None
    db = ar.tensor((dout,), torch.float32, db_fill) if want[2] else None
    ptr = lambda t: None if t is None else t.data_ptr()
    rc = L.pca_linear_bwd(X.data_ptr(), W.data_ptr(), dY.data_ptr(), ptr(dX), ptr(dW), ptr(db), M, din, dout,
                          ar.block(L.pca_linear_bwd_ws_bytes(M, din, dout)).data_ptr(), None)
    assert rc == 0, L.pca_last_error()
    torch.cuda.synchronize()
    return {"dX": dX, "dW": dW, "db": db}


@pytest.mark.parametrize("M,din,dout", [(1, 1, 1), (37, 128, 50), (4099, 256, 10), (128, 64, 64)], ids=str)
def test_linear_contract(dev, M, din, dout):
    """Y = X W^T + b against float64 (F32 bar); dW and db accumulate; dX is written; dX, dW and db may each
    be NULL (linear_bwd_f32: the fused dW + db job, or linear_dw / colsum alone)."""
    from pca_hip import _lib
    L = _lib.lib()
    g = torch.Generator().manual_seed(M + din + dout)
    X, W, b = torch.randn(M, din, generator=g), torch.randn(dout, din, generator=g), torch.randn(dout, generator=g)
    dY = torch.randn(M, dout, generator=g)
    ref = {"Y": X.double() @ W.double().t() + b.double(), "dX": dY.double() @ W.double(),
           "dW": dY.double().t() @ X.double(), "db": dY.double().sum(0)}
    ar = am.Arena(dev)
    Xd, Wd, bd, dYd = (t.to(dev) for t in (X, W, b, dY))
    Y = ar.tensor((M, dout), torch.float32, NAN)
    assert L.pca_linear_fwd(Xd.data_ptr(), Wd.data_ptr(), bd.data_ptr(), Y.data_ptr(), M, din, dout, None) == 0
    torch.cuda.synchronize()
    bad = []
    gb.own_close(Y, ref["Y"], gb.F32, "Y")
    fresh = _linear(dev, ar, Xd, Wd, bd, dYd, NAN, 0.0, 0.0)
    again = _linear(dev, ar, Xd, Wd, bd, dYd, NAN, 0.0, 0.0)
    repro = all(am.bit_equal(fresh[k], again[k]) for k in fresh)
    for k in ("dX", "dW", "db"):
        gb.own_close(fresh[k], ref[k], gb.F32, k)
    P = {k: am.prefill_like(fresh[k].cpu(), i + 3) for i, k in enumerate(("dW", "db"))}
    acc = _linear(dev, ar, Xd, Wd, bd, dYd, 0.0, P["dW"].to(dev), P["db"].to(dev))
    for k in ("dW", "db"):
        bad += am.accumulated_ok(acc[k], P[k], fresh[k], torch.float32, f"{k} accumulated")
    bad += am.written_ok(fresh["dX"], acc["dX"], exact=repro, bar=gb.F32, what="dX")
    for want in ((False, True, True), (True, False, True), (True, True, False)):
        out = _linear(dev, ar, Xd, Wd, bd, dYd, NAN, 0.0, 0.0, want)
        for k, w in zip(("dX", "dW", "db"), want):
            if w:
                bad += am.same_or_bar(out[k], fresh[k], repro, gb.F32, f"{k} with {want}")
    bad += ar.check()
    assert not bad, "\n".join(bad)


def test_linear_fp32_after_bf16_block(dev):
    """pca_linear_fwd after d = 256 bf16 block calls on the same thread (a trained one, and one the library
    refuses) still runs fp32 operands: a Bf16OperandScope left armed would round them to bf16 silently."""
    from pca_hip import _lib
    L = _lib.lib()
    ar = am.Arena(dev)
    for shape in ((2, 130, 32, 256, 256, 256, 8, 0), (2, 77, 32, 2, 256, 256, 8, 0),
                  (2, 32, 130, 256, 256, 256, 8, 1)):
        m = am.Mab(dev, *shape, M_BF16, seed=3)
        rc, _, saved = m.fwd(ar, NAN)
        assert rc == 0, m.error()
        rc, _ = m.bwd(ar, saved, dq_fill=NAN if not shape[-1] else 0.0, dk_fill=NAN)
        assert rc == (EUNSUPPORTED if shape[3] <= 4 else 0), m.error()
    g = torch.Generator().manual_seed(11)
    M, din, dout = 37, 128, 50
    X, W, b = torch.randn(M, din, generator=g), torch.randn(dout, din, generator=g), torch.randn(dout, generator=g)
    Y = ar.tensor((M, dout), torch.float32, NAN)
    Xd, Wd, bd = X.to(dev), W.to(dev), b.to(dev)
    assert L.pca_linear_fwd(Xd.data_ptr(), Wd.data_ptr(), bd.data_ptr(), Y.data_ptr(), M, din, dout, None) == 0
    torch.cuda.synchronize()
    gb.own_close(Y, X.double() @ W.double().t() + b.double(), gb.F32, "linear after bf16 blocks")
    assert ar.check() == []


# ---- pca_cross_entropy --------------------------------------------------------------------------------
@pytest.mark.parametrize("B,Cc,big", [(1, 5, False), (7, 50, False), (5, 10, True)], ids=["B1", "B7", "pm3e4"])
def test_cross_entropy_contract(dev, B, Cc, big):
    """loss = mean(logsumexp - picked) against float64; dlogits = (softmax - onehot) grad_scale / B;
    stats_out accumulates {sum of per-sample loss, #correct}; labels at 0 and C - 1; logits of +-3e4."""
    from pca_hip import _lib
    L = _lib.lib()
    g = torch.Generator().manual_seed(B * Cc)
    logits = torch.randn(B, Cc, generator=g) * 3
    if big:
        logits = torch.where(torch.rand(B, Cc, generator=g) < 0.5, -3e4, 3e4) + torch.randn(B, Cc, generator=g)
    labels = torch.randint(0, Cc, (B,), generator=g)
    labels[0] = Cc - 1
    if B > 1:
        labels[1] = 0
    lg = logits.double()
    per = torch.logsumexp(lg, 1) - lg.gather(1, labels.view(-1, 1)).squeeze(1)
    correct = float((lg.argmax(1) == labels).sum())
    ar = am.Arena(dev)
    bad = []
    for gs in (1.0, 0.37):
        loss = ar.tensor((1,), torch.float32, NAN)
        dlog = ar.tensor((B, Cc), torch.float32, NAN)
        P = torch.tensor([3.25, 2.0])
        stats = ar.tensor((2,), torch.float32, P)
        ld, yd = logits.to(dev), labels.to(dev)
        rc = L.pca_cross_entropy(ld.data_ptr(), yd.data_ptr(), B, Cc, gs, loss.data_ptr(), dlog.data_ptr(),
                                 stats.data_ptr(), None)
        assert rc == 0, L.pca_last_error()
        torch.cuda.synchronize()
        lv = float(loss.cpu())
        assert np.isfinite(lv) and abs(lv - float(per.mean())) <= 1e-6 * max(1.0, float(per.abs().max())), \
            (lv, float(per.mean()))
        ref_d = (torch.softmax(lg, 1) - torch.nn.functional.one_hot(labels, Cc).double()) * gs / B
        gb.own_close(dlog, ref_d, gb.F32, f"dlogits (grad_scale {gs})")
        st = stats.cpu().double()
        assert abs(float(st[0]) - (3.25 + float(per.sum()))) <= 1e-6 * (3.25 + float(per.abs().sum())), (st, per)
        assert float(st[1]) == 2.0 + correct, (st, correct)
    assert ar.check() == []
