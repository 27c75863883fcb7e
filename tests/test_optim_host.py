"""The guarded optimiser step without a GPU: the C ABI of csrc/optim.hip (symbols, the arguments refused
before any launch, the partial-count query), the host schedule helper, the Trainer's signature, and the
CPU restatement tests/optim_ref.py against stock torch (clip_grad_norm_ + torch.optim.Adam)."""
import ctypes as C
import inspect
import math

import numpy as np
import pytest
import torch

import pca_hip
from pca_hip import _lib

import optim_ref
from test_abi_host import header_symbols
from util import close

NEW = ("pca_grad_sumsq_partials", "pca_grad_sumsq", "pca_adam_step_ex")


def test_new_symbols_declared_exported_bound():
    syms = header_symbols()
    handle = C.CDLL(_lib.LIB_PATH)
    for s in NEW:
        assert s in syms, f"{s} not declared in pca_hip.h"
        assert hasattr(handle, s), f"{s} not exported"
        assert s in _lib.SIGNATURES, f"{s} not bound"
    assert pca_hip.lib().pca_abi_version() == 2
    # the structs as the header lays them out
    assert C.sizeof(_lib.OptimCfg) == 32 and C.sizeof(_lib.OptimState) == 32
    assert _lib.OptimState.norm_sum.offset == 16 and _lib.OptimState.norm_count.offset == 24


def test_partials_query_is_a_function_of_n_within_bounds():
    L = pca_hip.lib()
    seen = []
    for n in (0, 1, 3, 4, 255, 2048, 2049, 4096, 4097, 292_530, 1_151_026, 10 ** 8, 2 ** 33 + 5):
        a, b = L.pca_grad_sumsq_partials(n), L.pca_grad_sumsq_partials(n)
        assert a == b and 1 <= a <= 1024, (n, a, b)
        seen.append(a)
    assert seen == sorted(seen) and seen[0] == 1 and seen[-1] > 1      # grows with n, then saturates
    assert L.pca_grad_sumsq_partials(10 ** 8) == L.pca_grad_sumsq_partials(2 ** 33 + 5)
    assert L.pca_grad_sumsq_partials(-1) == 0


def _host_buffers(n=16):
    """Host memory standing in for device pointers: every call below must be refused before a launch
    could touch it (a launch on a machine without a GPU would return PCA_ELAUNCH, not PCA_EINVAL)."""
    f = [(C.c_float * n)() for _ in range(4)]
    step = (C.c_int32 * 2)()
    state = _lib.OptimState()
    part = (C.c_double * 1024)()
    table = (C.c_float * 4)()
    return f, step, state, part, table


def _addr(x):
    return C.addressof(x)


def _refused(rc, *words):
    assert rc == -1, rc                                                # PCA_EINVAL
    msg = pca_hip.lib().pca_last_error().decode()
    assert msg and all(w in msg for w in words), msg


def test_grad_sumsq_refuses_bad_arguments_before_any_launch():
    L = pca_hip.lib()
    f, _, _, part, _ = _host_buffers()
    np_ = L.pca_grad_sumsq_partials(16)
    _refused(L.pca_grad_sumsq(None, 16, _addr(part), np_, None), "grad_sumsq", "null")
    _refused(L.pca_grad_sumsq(_addr(f[0]), 16, None, np_, None), "grad_sumsq", "null")
    _refused(L.pca_grad_sumsq(_addr(f[0]), -1, _addr(part), 1, None), "grad_sumsq", "n=-1")
    _refused(L.pca_grad_sumsq(_addr(f[0]), 16, _addr(part), np_ + 1, None), "grad_sumsq", "n_partials")
    _refused(L.pca_grad_sumsq(_addr(f[0]), 16, _addr(part), 0, None), "grad_sumsq", "n_partials")
    assert all(v == 0.0 for v in part)


def test_adam_step_ex_refuses_bad_arguments_before_any_launch():
    L = pca_hip.lib()
    f, step, state, part, table = _host_buffers()
    n = 16
    np_ = L.pca_grad_sumsq_partials(n)

    def call(p=f[0], g=f[1], m=f[2], v=f[3], n=n, o="cfg", partials=part, n_partials=np_, lr_table=table,
             lr_table_len=4, step=step, state=state, max_norm=1.0, skip=1):
        cfg = _lib.OptimCfg(1e-3, 0.9, 0.999, 1e-8, 1e-3, 1.0, max_norm, skip)
        a = lambda x: None if x is None else _addr(x)
        return L.pca_adam_step_ex(a(p), a(g), a(m), a(v), n, None if o is None else C.byref(cfg),
                                  a(partials), n_partials, a(lr_table), lr_table_len, a(step), a(state), 1,
                                  None)

    for name in ("p", "g", "m", "v", "o", "step", "state"):
        _refused(call(**{name: None}), "adam_step_ex", "null")
    _refused(call(n=-5), "adam_step_ex", "n=-5")
    _refused(call(lr_table_len=0), "adam_step_ex", "lr_table_len=0")
    _refused(call(lr_table_len=-2), "adam_step_ex", "lr_table_len=-2")
    _refused(call(max_norm=float("nan")), "adam_step_ex", "max_norm", "NaN")
    _refused(call(n_partials=np_ + 1), "adam_step_ex", "n_partials")
    # no partials: legal only when nothing needs the norm
    _refused(call(partials=None, n_partials=0), "adam_step_ex", "partials is NULL")
    _refused(call(partials=None, n_partials=0, max_norm=0.0, skip=1), "adam_step_ex", "partials is NULL")
    _refused(call(partials=None, n_partials=0, max_norm=2.0, skip=0), "adam_step_ex", "partials is NULL")
    # nothing ran: the buffers are as they were
    assert list(step) == [0, 0] and state.skipped == 0 and state.norm_count == 0
    assert all(v == 0.0 for b in f for v in b)


def test_warmup_cosine_matches_its_closed_form():
    from pca_hip import trainer
    base, W, Tn, lo = 3e-3, 5, 20, 1e-5
    tab = trainer.warmup_cosine(base, W, Tn, lr_min=lo)
    assert isinstance(tab, list) and len(tab) == Tn and all(isinstance(x, float) for x in tab)
    for t in range(1, Tn + 1):
        want = base * t / W if t <= W else \
            lo + 0.5 * (base - lo) * (1 + math.cos(math.pi * (t - W) / (Tn - W)))
        assert tab[t - 1] == pytest.approx(want, rel=1e-15, abs=0.0), t
    assert tab[0] == base / W and tab[W - 1] == base                   # ramp from base / W up to base
    assert tab[-1] == pytest.approx(lo, rel=1e-12)                     # half a cosine: ends at lr_min
    assert all(a < b for a, b in zip(tab[:W], tab[1:W])) and all(a > b for a, b in zip(tab[W - 1:], tab[W:]))
    assert trainer.warmup_cosine(1.0, 0, 3)[0] == pytest.approx(0.5 * (1 + math.cos(math.pi / 3)))
    assert trainer.warmup_cosine(2.0, 4, 4) == [0.5, 1.0, 1.5, 2.0]    # lr_min defaults to 0; all ramp
    with pytest.raises(ValueError):
        trainer.warmup_cosine(1.0, 5, 4)


def test_trainer_signature_carries_the_options_with_their_defaults():
    from pca_hip import trainer
    sig = inspect.signature(trainer.Trainer).parameters
    assert sig["max_grad_norm"].default is None
    assert sig["skip_nonfinite"].default is False
    assert sig["lr_schedule"].default is None
    assert sig["schedule_steps"].default is None
    assert callable(trainer.Trainer.read_optim_stats)
    # the table the options are materialised into
    tab = trainer._lr_table(lambda t: 0.1 * t, 3)
    assert tab.dtype == torch.float32 and tab.tolist() == [np.float32(0.1), np.float32(0.2), np.float32(0.3)]
    assert trainer._lr_table([1e-3, 2e-3], None).numel() == 2 and trainer._lr_table(None, None) is None
    for bad in (dict(lr_schedule=lambda t: 1.0, schedule_steps=None), dict(lr_schedule=[], schedule_steps=None),
                dict(lr_schedule=[1.0, float("nan")], schedule_steps=None)):
        with pytest.raises(ValueError):
            trainer._lr_table(**bad)


def test_restatement_equals_stock_torch_clip_schedule_skip():
    """tests/optim_ref.py against torch.nn.utils.clip_grad_norm_ + torch.optim.Adam over 6 steps: a
    4-entry table, a max_norm that clips some steps and not others, and a NaN gradient at step 3 that
    stock Adam simply is not stepped for."""
    g = torch.Generator().manual_seed(4)
    n = 3001
    p0 = {"a": torch.randn(n, generator=g), "b": torch.randn(7, 5, generator=g)}
    table = [2e-4, 6e-4, 1e-3, 5e-4]
    scales = [1.0, 0.3, 1.0, 1.0, 0.2, 1.0]
    max_norm = 0.5 * math.sqrt(n + 35)
    P = {k: v.clone() for k, v in p0.items()}
    ref = optim_ref.OptimRef(P, max_norm=max_norm, skip_nonfinite=True, table=table)
    truth = optim_ref.TorchTruth(p0, max_norm=max_norm, skip_nonfinite=True, table=table)
    for it, sc in enumerate(scales):
        grads = {k: torch.randn(v.shape, generator=g) * sc for k, v in p0.items()}
        if it == 2:
            grads["a"][17] = float("nan")
        ref.step(P, grads)
        truth.step(grads)
        if it != 2:
            assert ref.last_norm == pytest.approx(truth.norms[-1], rel=1e-6)
        assert ref.last_lr == np.float32(table[min(it + 1, 4) - 1])
    assert ref.skipped == 1 and ref.clipped == 3 and ref.adam.t == 5
    for k in p0:
        m, v = truth.moments(k)
        close(P[k], truth.p[k], 1e-6, k)
        close(ref.m[k], m, 1e-6, "m " + k)
        close(ref.v[k], v, 1e-6, "v " + k)
