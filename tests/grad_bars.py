"""One judge for whole-step gradients, each tensor on its OWN scale.

tests/util.py's ``close`` / ``close_robust`` measure an error relative to max(1, max|ref|).  The gradients
of a mean cross-entropy over a few sets are 1e-2 .. 1e-11, so there that floor of 1 turns the relative
bar into an absolute one far above the value checked: at the set-resident train step (B = 6, N = 256,
din = 2) ``close_robust(., 5e-2)`` accepts an all-zero result for 28 of the 45 tensors
(tests/test_grad_bars_host.py).  Here:

* ``own_close``: the error of every element relative to S = max|ref| (no floor), the semantics of
  ``close_robust`` (rms <= tol / 2, at most ``outlier_frac`` of the elements beyond tol, none beyond
  cap * tol) plus a norm criterion ||got - ref||_2 <= tol_n ||ref||_2 that catches a uniform mis-scaling
  of a heavy-tailed tensor.  S = 0 fails unless the caller supplies another scale.
* ``NOISE``: the tensors whose exact gradient is (nearly) zero for an analytic reason; they are judged
  on the scale of a named sibling of the same block, never on 1.
* ``judge``: walks the named parameters of a flat gradient vector (``STEngine.grads``, state_dict
  order) or a dict, judges every tensor, prints one table row per tensor and raises on the failures.
* the bars of each comparison kind, calibrated on an MI355X (worst per-tensor own-scale value measured
  next to each constant).  Setting ``GRAD_BARS_CALIBRATE=<file>`` makes ``judge`` append its
  measurements to that file as JSON lines instead of asserting (the assertions of tests/util.py that
  the call sites keep are not affected).
"""
import json
import os
import re
from typing import NamedTuple

import numpy as np
import torch


class Bar(NamedTuple):
    tol: float            # per element, relative to the tensor's own max|ref|
    tol_n: float          # ||got - ref||_2 <= tol_n ||ref||_2
    outlier_frac: float   # fraction of the elements allowed beyond tol
    cap: float            # no element beyond cap * tol


# Calibrated on an MI355X over every call site of the kind (tests/test_gpu_*.py); "measured" is the worst
# per-tensor own-scale value outside NOISE: max element error, rms, fraction beyond tol, norm ratio.
# fp32 paths against the oracle, the golden vectors or another fp32 path (reduction order only).
# Measured: max 7.2e-5, rms 6.3e-6, norm 2.2e-5 (enc.1.mab1.fc_o.bias, configs[2] full size).
F32 = Bar(tol=2e-4, tol_n=6e-5, outlier_frac=0.0, cap=1.0)
# bf16 / fp8 engine against the emulation of its operand roundings (tests/emu.py).  Measured: max 2.8e-1,
# rms 1.8e-2, 8e-3 beyond 3e-2, norm 5.7e-2 (bf16) / 7.0e-2 (fp8) (dec.0.mab.fc_o.bias / .fc_k.weight,
# configs[4] varlen train step: 5 sets, a ReLU flip of the PMA's fc_o moves a fifth of an element).
BF16_VS_EMU = Bar(tol=4e-2, tol_n=1e-1, outlier_frac=1e-2, cap=10.0)
FP8_VS_EMU = BF16_VS_EMU
# bf16-operand paths against the exact oracle, the golden vectors or the library's fp32 mode.  Measured:
# max 5.0e-1, rms 3.9e-2, 1.6e-2 beyond 6e-2, norm 1.28e-1 - all dec.0.mab.fc_o.* at 2 or 3 sets (the
# PMA's ReLU flips, see above); elsewhere norm <= 7.2e-2.  CPU emulation vs exact: max 1.9e-2, norm 8.8e-3.
BF16_VS_ORACLE = Bar(tol=8e-2, tol_n=1.5e-1, outlier_frac=2e-2, cap=8.0)
# fp8 mode against the exact oracle.  Measured: max 5.3e-1, rms 4.4e-2, 1.6e-2 beyond 1e-1, norm 1.56e-1
# (configs[4] varlen, enc.1.mab0.fc_k.weight); CPU emulation vs exact: 2.3e-2 beyond 1e-1, norm 1.52e-1.
FP8_VS_ORACLE = Bar(tol=1e-1, tol_n=2e-1, outlier_frac=3e-2, cap=8.0)
# peers, the same arithmetic by two implementations (set-resident vs per-block launches, the A/B switches;
# a merged fp32 statistic in another order flips the rounding of a few bf16 activations).  Measured: max
# 6.2e-2 (dec.0.mab.fc_o.bias), rms 6.4e-3, 2.2e-2 beyond 2e-2 and norm 2.0e-2 (enc.1.I, din = 1).
PEER = Bar(tol=5e-2, tol_n=5e-2, outlier_frac=2.5e-2, cap=4.0)


# name pattern, class, sibling (same block) whose scale judges it, reason.  Both classes are judged on the
# sibling's scale under every bar: on their own scale the measured errors are noise-sized (the "cancel"
# class: 0.7 of its own scale between peers, 0.96 against the emulation, 1.6e-2 in fp32 against the oracle).
NOISE = [
    (r"(^|\.)fc_k\.bias$", "zero", "fc_q.bias",
     "identically zero: softmax is shift-invariant, so a bias added to every key of a head moves no score; "
     "judged on the query bias, the same [d] row reduction of an uncancelled gradient"),
    (r"^enc\.\d+\.mab1\.fc_k\.weight$", "cancel", "fc_q.weight",
     "cancellation-dominated: the keys are the m nearly equal rows of H, so near shift-invariance cancels "
     "it to ~1e-5 of its block's fc_q.weight"),
]

# Extra analytically-zero tensors of one set size, for ``judge(..., zero=)``: with a single key per set the
# softmax is 1 whatever the key projection, so no gradient reaches the few-queries blocks' fc_k.weight.
SINGLE_KEY = [
    (r"(\.mab0|^dec\.0\.mab)\.fc_k\.weight$", "zero", "fc_v.weight",
     "one key per set: a softmax over one score is 1, so the key projection gets no gradient"),
]


def noise_class(name, extra=()):
    """(class, sibling name) of a NOISE (or ``extra``) tensor, or None."""
    for pat, cls, sib, _ in list(extra) + NOISE:
        if re.search(pat, name):
            return cls, name[:name.rindex(".fc_k.")] + "." + sib
    return None


def _np(a):
    if isinstance(a, torch.Tensor):
        a = a.detach().cpu().numpy()
    return np.asarray(a, dtype=np.float64)


def errors(got, ref, scale=None):
    """Own-scale error figures of one tensor: max, rms and the element errors relative to S (max|ref| or
    the given scale), and ||got - ref|| / ||ref||."""
    a, b = _np(got), _np(ref)
    assert a.shape == b.shape, (a.shape, b.shape)
    S = float(np.max(np.abs(b))) if scale is None else float(scale)
    d = np.abs(a - b) / S if S > 0 else np.full(a.shape, np.inf)
    nb = float(np.linalg.norm(b))
    return dict(S=S, max=float(d.max()) if d.size else 0.0,
                rms=float(np.sqrt(np.mean(d ** 2))) if d.size else 0.0,
                norm=float(np.linalg.norm(a - b)) / nb if nb > 0 else np.inf,
                finite=bool(np.all(np.isfinite(a))), d=d)


def verdict(e, bar, outlier_frac=None, norm=True):
    """The list of the bar's criteria that the errors ``e`` (from ``errors``) violate."""
    frac = bar.outlier_frac if outlier_frac is None else outlier_frac
    bad = []
    if not e["finite"]:
        bad.append("non-finite values")
    if not e["S"] > 0:
        bad.append("reference is all zero (declare the tensor in NOISE or pass a scale)")
        return bad
    out = float(np.mean(e["d"] > bar.tol)) if e["d"].size else 0.0
    if e["rms"] > bar.tol / 2:
        bad.append(f"rms {e['rms']:.2e} > {bar.tol / 2:.1e}")
    if out > frac:
        bad.append(f"{out:.2e} of elements beyond {bar.tol:.1e} (max {e['max']:.2e})")
    if e["max"] > bar.cap * bar.tol:
        bad.append(f"max {e['max']:.2e} > {bar.cap:g} * {bar.tol:.1e}")
    if norm and e["norm"] > bar.tol_n:
        bad.append(f"norm ratio {e['norm']:.2e} > {bar.tol_n:.1e}")
    return bad


def own_close(got, ref, bar, what="", scale=None, outlier_frac=None):
    """Assert one tensor against ``bar`` on its own scale (or ``scale``); returns its max error."""
    e = errors(got, ref, scale)
    bad = verdict(e, bar, outlier_frac, norm=scale is None)
    assert not bad, f"{what}: " + "; ".join(bad)
    return e["max"]


def split(got, shapes):
    """A flat gradient vector -> {name: tensor} in ``shapes`` order (every element accounted for)."""
    out, off = {}, 0
    flat = got.detach().reshape(-1) if isinstance(got, torch.Tensor) else np.asarray(got).reshape(-1)
    for k, shp in shapes:
        n = int(np.prod(shp))
        out[k] = flat[off:off + n].reshape(shp)
        off += n
    assert off == flat.shape[0], f"flat gradient has {flat.shape[0]} elements, the parameters {off}"
    return out


def shapes_of(net):
    """(name, shape) of every parameter of a module, in the order of its flat gradient vector."""
    return [(k, tuple(p.shape)) for k, p in net.named_parameters()]


def judge(got, ref, bar, shapes, what="", outlier_frac=None, zero=(), quiet=False):
    """Judge every named gradient of ``got`` against ``ref`` (each a flat vector in ``shapes`` order or a
    dict) under ``bar``; NOISE tensors, and those ``zero`` declares (entries like NOISE's), on their
    sibling's scale.  Prints the per-tensor table, raises listing every failing tensor; returns the table."""
    if not isinstance(got, dict):
        got = split(got, shapes)
    if not isinstance(ref, dict):
        ref = split(ref, shapes)
    g = {k: _np(got[k]).reshape(shp) for k, shp in shapes}
    r = {k: _np(ref[k]).reshape(shp) for k, shp in shapes}
    rows, fails = [], []
    for k, _ in shapes:
        nc = noise_class(k, zero)
        scale, rule = None, "own"
        if nc is not None:
            scale, rule = float(np.max(np.abs(r[nc[1]]))), "sib"
        e = errors(g[k], r[k], scale)
        out = float(np.mean(e["d"] > bar.tol)) if e["d"].size else 0.0
        bad = verdict(e, bar, outlier_frac, norm=scale is None)
        row = dict(name=k, rule=rule, S=e["S"], max=e["max"], rms=e["rms"], out=out, norm=e["norm"])
        if nc is not None:       # both scales of a noise tensor, for calibration
            s2 = float(np.max(np.abs(r[nc[1]])))
            row["max_sib"] = float(np.max(np.abs(g[k] - r[k]))) / s2 if s2 > 0 else np.inf
            s1 = float(np.max(np.abs(r[k])))
            row["max_own"] = float(np.max(np.abs(g[k] - r[k]))) / s1 if s1 > 0 else np.inf
        rows.append(row)
        if bad:
            fails.append(f"{k} [{rule}]: " + "; ".join(bad))
    if not quiet:
        print(f"-- {what}: per-tensor own-scale errors (bar tol {bar.tol:.1e}, tol_n {bar.tol_n:.1e})")
        for row in rows:
            print(f"   {row['name']:<28} {row['rule']} S={row['S']:.2e} max={row['max']:.2e} "
                  f"rms={row['rms']:.2e} out={row['out']:.1e} norm={row['norm']:.2e}")
    cal = os.environ.get("GRAD_BARS_CALIBRATE")
    if cal:
        with open(cal, "a") as f:
            test = os.environ.get("PYTEST_CURRENT_TEST", "").split(" ")[0]
            f.write(json.dumps(dict(test=test, what=what, bar=bar._asdict(), rows=rows,
                                    fails=fails)) + "\n")
        return rows
    assert not fails, f"{what}: {len(fails)} tensors off their own scale:\n  " + "\n  ".join(fails)
    return rows
