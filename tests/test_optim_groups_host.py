"""pca_adam_step_groups without a GPU: the CPU restatement tests/optim_groups_ref.py against stock torch
(torch.optim.AdamW / Adam in param groups, clip_grad_norm_, AveragedModel), the header and the binding,
the arguments refused before any launch, and how the Trainer resolves ``param_groups``."""
import ctypes as C
import inspect
import os
import re

import pytest
import torch

import pca_hip
from pca_hip import _lib

import optim_groups_ref as ogr
from conftest import ROOT
from test_abi_host import header_symbols
from util import close

ADAM_TOL = 1e-6          # the project's bar for one fused Adam pass (tests/test_gpu_optim.py)


# ---- the restatement against stock torch ---------------------------------------------------------------
@pytest.fixture(scope="module")
def inputs():
    return ogr.adam_inputs()


def _run_both(name, inputs, **over):
    n, p, grads = inputs
    kw = dict(ogr.CASES[name], **over)
    ref, truth = ogr.GroupsRef(p, **kw), ogr.StockTruth(p, **kw)
    for g in ogr.case_grads(name, grads):
        ref.step(g)
        truth.step(g)
    return ref, truth


@pytest.mark.parametrize("name", sorted(ogr.CASES))
def test_restatement_equals_stock_torch(inputs, name):
    ref, truth = _run_both(name, inputs)
    for what in ("p", "m", "v"):
        err = close(getattr(ref, what), getattr(truth, what), ADAM_TOL, f"{name} {what}")
        print(f"{name} {what}: max|d| {err:.2e}")
    if ref.avg is not None:
        close(ref.avg, truth.avg, ADAM_TOL, f"{name} avg")
    if name == "skip":
        assert ref.skipped == 1 and truth.applied == 4 and truth.averaged == 4   # four times, not five
    if "clipped" in name:
        assert ref.clipped == 4


def test_the_switches_show_at_these_hyper_parameters(inputs):
    """What the issue measured with stock torch at lr = 1e-2, wd = 0.1: every switch moves the result
    orders of magnitude above ADAM_TOL, so a kernel that ignored one would fail the GPU comparison."""
    n, p, grads = inputs
    gs = ogr.case_grads("x", grads)
    common = dict(max_norm=50.0, avg_decay=0.9, avg_start=2)

    def run(**kw):
        t = ogr.StockTruth(p, **dict(common, **kw))
        for g in gs:
            t.step(g)
        return t

    dec, cpl, grp = run(decoupled=True), run(decoupled=False), run(decoupled=True, **ogr.GROUPS)
    d = lambda a, b: float((a - b).abs().max())
    assert d(dec.p, cpl.p) > 1e-2 and d(dec.avg, dec.p) > 1e-2
    diffs = [d(grp.p[lo:hi], dec.p[lo:hi]) for lo, hi in grp.segs]
    print("coupled vs decoupled", d(dec.p, cpl.p), "ema vs p", d(dec.avg, dec.p), "segments", diffs,
          "max|p|", float(dec.p.abs().max()))
    # segment 1 has both scales 1: the ungrouped run, up to the rounding of a norm summed in other pieces
    assert diffs[0] <= ADAM_TOL * float(dec.p.abs().max()) and all(x > 1e-3 for x in diffs[1:])
    assert torch.equal(grp.p[4099:4101], p[4099:4101])                     # lr_scale 0: does not move
    assert float(grp.m[4099:4101].abs().min()) > 0.0


def test_tiny_vector_with_a_one_element_segment():
    g = torch.Generator().manual_seed(3)
    p = torch.randn(3, generator=g)
    kw = dict(seg_end=(1, 3), lr_scale=(0.5, 1.0), wd_scale=(0.0, 1.0), decoupled=True, avg_decay=0.9)
    ref, truth = ogr.GroupsRef(p, **kw), ogr.StockTruth(p, **kw)
    for _ in range(3):
        gr = torch.randn(3, generator=g)
        ref.step(gr)
        truth.step(gr)
    for what in ("p", "m", "v", "avg"):
        close(getattr(ref, what), getattr(truth, what), ADAM_TOL, what)


# ---- header and binding ------------------------------------------------------------------------------------
def test_symbol_declared_exported_bound_and_the_struct_laid_out_as_declared():
    assert "pca_adam_step_groups" in header_symbols()
    assert hasattr(C.CDLL(_lib.LIB_PATH), "pca_adam_step_groups")
    assert "pca_adam_step_groups" in _lib.SIGNATURES
    assert pca_hip.lib().pca_abi_version() == 2
    text = open(os.path.join(ROOT, "include", "pca_hip.h")).read()
    body = re.search(r"typedef struct pca_optim_groups \{(.*?)\} pca_optim_groups;", text, re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    decl = [(" ".join(d.split()[:-1]).replace(" *", "*"), d.split()[-1].lstrip("*"))
            for d in (x.strip() for x in body.split(";")) if d]
    ctype = {"int32_t": C.c_int32, "float": C.c_float, "const int64_t*": C.c_void_p,
             "const float*": C.c_void_p, "float*": C.c_void_p}
    assert [(name, ctype[t]) for t, name in decl] == list(_lib.OptimGroups._fields_)
    assert C.sizeof(_lib.OptimGroups) == 48 and _lib.OptimGroups.avg_weight.offset == 40
    # the arguments of pca_adam_step_ex, then the struct, the host mirror and the stream
    ex, gr = _lib.SIGNATURES["pca_adam_step_ex"][1], _lib.SIGNATURES["pca_adam_step_groups"][1]
    assert gr[:len(ex) - 1] == ex[:-1] and len(gr) == len(ex) + 2
    assert gr[len(ex) - 1] == C.POINTER(_lib.OptimGroups)


def _refused(rc, *words):
    assert rc == -1, rc                                                # PCA_EINVAL
    msg = pca_hip.lib().pca_last_error().decode()
    assert msg and all(w in msg for w in words), msg


def test_refuses_bad_arguments_before_any_launch():
    """Host memory stands in for the device pointers: a launch on a machine without a GPU would return
    PCA_ELAUNCH, not PCA_EINVAL, and one with a GPU would fault on them."""
    L = pca_hip.lib()
    n = 16
    f = [(C.c_float * n)() for _ in range(5)]
    step, state = (C.c_int32 * 2)(), _lib.OptimState()
    part = (C.c_double * 1024)()
    scales = (C.c_float * 256)(*([1.0] * 256))
    np_ = L.pca_grad_sumsq_partials(n)
    a = lambda x: None if x is None else C.addressof(x)

    def call(ends=(4, 9, 16), n_seg=None, avg_weight=0.1, avg_start=1, gr=True, mirror=True, null=None,
             partials=part, max_norm=1.0, skip=1):
        table = (C.c_int64 * max(len(ends), 1))(*ends)
        cfg = _lib.OptimCfg(1e-3, 0.9, 0.999, 1e-8, 1e-3, 1.0, max_norm, skip)
        g = _lib.OptimGroups(1, len(ends) if n_seg is None else n_seg, a(table), a(scales), a(scales),
                             a(f[4]), avg_weight, avg_start)
        ptrs = {k: a(v) for k, v in dict(p=f[0], g=f[1], m=f[2], v=f[3], step=step, state=state).items()}
        if null:
            ptrs[null] = None
        return L.pca_adam_step_groups(ptrs["p"], ptrs["g"], ptrs["m"], ptrs["v"], n, C.byref(cfg),
                                      a(partials), np_ if partials is not None else 0, None, 0,
                                      ptrs["step"], ptrs["state"], 1, C.byref(g) if gr else None,
                                      a(table) if mirror else None, None)

    _refused(call(gr=False), "adam_step_groups", "gr is NULL")
    for name in ("p", "g", "m", "v", "step", "state"):                   # state_dev is required
        _refused(call(null=name), "adam_step_groups", "null")
    _refused(call(n_seg=-1), "adam_step_groups", "n_seg=-1")
    _refused(call(ends=tuple(range(1, 258)), n_seg=257), "adam_step_groups", "n_seg=257")
    _refused(call(ends=(4, 4, 16)), "adam_step_groups", "ascending")
    _refused(call(ends=(9, 4, 16)), "adam_step_groups", "ascending")
    _refused(call(ends=(0, 16)), "adam_step_groups", "ascending")
    _refused(call(ends=(4, 9, 15)), "adam_step_groups", "ends at 15", "n=16")
    _refused(call(ends=(4, 9, 17)), "adam_step_groups", "ends at 17")
    _refused(call(mirror=False), "adam_step_groups", "seg_end_host")
    for w in (0.0, -0.1, 1.5, float("nan")):
        _refused(call(avg_weight=w), "adam_step_groups", "avg_weight")
    _refused(call(avg_start=0), "adam_step_groups", "avg_start=0")
    _refused(call(avg_start=-3), "adam_step_groups", "avg_start=-3")
    _refused(call(partials=None), "adam_step_groups", "partials is NULL")
    _refused(call(partials=None, max_norm=0.0, skip=1), "adam_step_groups", "partials is NULL")
    # nothing ran: the buffers are as they were
    assert list(step) == [0, 0] and state.skipped == 0 and state.norm_count == 0
    assert all(v == 0.0 for b in f for v in b)


# ---- group resolution ----------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def net():
    import models
    return models.ST(2, 1, 10, 16, 128, 4)


def test_no_decay_groups_marks_biases_inducing_points_and_seed(net):
    """Exactly the bias tensors, enc.0.I, enc.1.I and dec.0.S lose their decay.  (ST has 21 bias tensors:
    four per MAB, five MABs, and dec.1's.)"""
    from pca_hip import trainer
    res = trainer.resolve_param_groups(net, trainer.no_decay_groups())
    keys = list(net.state_dict().keys())
    marked = [k for k in keys if res["tensors"][k] == (1.0, 0.0)]
    biases = [k for k in keys if k.endswith(".bias")]
    assert len(keys) == 45 and len(biases) == 21
    assert sorted(marked) == sorted(biases + ["enc.0.I", "enc.1.I", "dec.0.S"])
    assert all(res["tensors"][k] == (1.0, 1.0) for k in keys if k not in marked)
    # the merged table: strictly ascending, ends at the parameter count, no two neighbours alike
    n = sum(p.numel() for p in net.parameters())
    ends = res["seg_end"]
    assert ends[-1] == n and all(b > a for a, b in zip([0] + ends[:-1], ends))
    pairs = list(zip(res["lr_scale"], res["wd_scale"]))
    assert len(pairs) == len(ends) <= 256 and all(a != b for a, b in zip(pairs, pairs[1:]))
    # enc.0.I is the first tensor and a segment of its own; dec.1.bias (10 elements) the last
    assert ends[0] == net.enc[0].I.numel() and pairs[0] == (1.0, 0.0)
    assert ends[-1] - ends[-2] == 10 and pairs[-1] == (1.0, 0.0)
    # every element's scales, read back through the table, are its tensor's
    off, seg = 0, 0
    for k, p in net.state_dict().items():
        for pos in (off, off + p.numel() - 1):
            while ends[seg] <= pos:
                seg += 1
            assert pairs[seg] == res["tensors"][k], k
        off += p.numel()


def test_first_match_wins_adjacent_equals_merge_and_an_unmatched_pattern_raises(net):
    from pca_hip import trainer
    n = sum(p.numel() for p in net.parameters())
    res = trainer.resolve_param_groups(net, [(r"^dec\.1\.", 1.0, 1.0), (r"", 0.0, 1.0)])
    head = net.dec[1].weight.numel() + net.dec[1].bias.numel()
    assert res["seg_end"] == [n - head, n] and res["lr_scale"] == [0.0, 1.0]     # only dec.1 moves
    assert res["tensors"]["dec.1.bias"] == (1.0, 1.0) and res["tensors"]["enc.0.I"] == (0.0, 1.0)
    assert trainer.resolve_param_groups(net, [])["seg_end"] == [n]
    with pytest.raises(ValueError, match="fc_z"):
        trainer.resolve_param_groups(net, trainer.no_decay_groups() + [(r"fc_z", 1.0, 0.0)])
    with pytest.raises(ValueError, match="lr_scale"):
        trainer.resolve_param_groups(net, [(r"bias", -1.0, 0.0)])


def test_trainer_and_fit_signatures_carry_the_options_with_their_defaults():
    from pca_hip import trainer
    import runfiles
    sig = inspect.signature(trainer.Trainer).parameters
    assert sig["decoupled_weight_decay"].default is False and sig["param_groups"].default is None
    assert sig["average_decay"].default is None and sig["average_start"].default == 1
    assert sig["eval_weights"].default == "model"
    assert callable(trainer.Evaluator.use_params)
    assert inspect.signature(trainer.STEngine.forward).parameters["params"].default is None
    assert inspect.signature(trainer.STEngine.attention).parameters["params"].default is None
    assert inspect.signature(runfiles.save_run).parameters["state_dict"].default is None


def test_save_run_writes_a_given_state_dict_in_the_reference_layout(net, tmp_path):
    import runfiles
    sd = {k: torch.full_like(v, 0.25) for k, v in net.state_dict().items()}
    cfg = dict(architecture=runfiles.ARCHITECTURES["FST"])
    pth, _ = runfiles.save_run(net, cfg, str(tmp_path), state_dict=sd)
    back = torch.load(pth, weights_only=True)
    assert list(back) == ["module." + k for k in net.state_dict()]
    assert all(bool((v == 0.25).all()) for v in back.values())
    # without it the model's own weights are written, as before
    pth, _ = runfiles.save_run(net, cfg, str(tmp_path / "own"))
    back = torch.load(pth, weights_only=True)
    assert all(torch.equal(back["module." + k], v) for k, v in net.state_dict().items())
