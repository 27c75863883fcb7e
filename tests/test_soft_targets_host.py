"""Soft targets without a GPU: the float64 restatement (tests/soft_ce_ref.py) against
torch.nn.functional.cross_entropy with probability targets, the three new symbols of the C ABI, what the
entry points refuse before any launch, and the datasets' ``mix_targets`` option."""
import ctypes
import os

import numpy as np
import pytest
import torch

import pca_hip
from pca_hip import _lib

import soft_ce_ref as ref
from test_abi_host import header_symbols

NEW = ("pca_cross_entropy_soft", "pca_st_train_fwd_bwd_soft", "pca_frame_points_ex_targets")
P = 0x1000                       # a stand-in device address: a refused call never reads it
NAN = float("nan")


# ---- the restatement -----------------------------------------------------------------------------------
def _case(C, B, wkind, seed):
    rng = np.random.Generator(np.random.PCG64(seed))
    x = rng.normal(0, 3, size=(B, C))
    y1 = rng.integers(0, C, size=B)
    y2 = rng.integers(0, C, size=B)
    y2[0] = y1[0]                                          # y1 == y2 is allowed
    y1[1], y2[1] = 0, C - 1
    w = rng.uniform(0, 1, size=B) if wkind == "random" else np.full(B, float(wkind))
    return x, y1, y2, w


@pytest.mark.parametrize("eps", [0.0, 0.1])
@pytest.mark.parametrize("wkind", [0.0, 0.5, 1.0, "random"])
@pytest.mark.parametrize("C", [3, 50, 70])
def test_restatement_against_torch_probability_targets(C, wkind, eps):
    B = 6
    x, y1, y2, w = _case(C, B, wkind, 17 * C + B)
    for gs in (1.0, 0.37):
        got = ref.soft_ce(x, y1, y2, w, eps, gs)
        t = torch.from_numpy(got["t"])
        assert torch.allclose(t.sum(1), torch.ones(B, dtype=torch.float64), atol=1e-15)
        xt = torch.from_numpy(x).requires_grad_(True)
        loss = torch.nn.functional.cross_entropy(xt, t)
        (loss * gs).backward()
        assert abs(got["loss"] - float(loss.detach())) <= 1e-12, (got["loss"], float(loss.detach()))
        assert float(np.abs(got["dlogits"] - xt.grad.numpy()).max()) <= 1e-12
        per = torch.nn.functional.cross_entropy(xt.detach(), t, reduction="none").numpy()
        assert float(np.abs(got["per"] - per).max()) <= 1e-12


@pytest.mark.parametrize("eps", [0.0, 0.1])
@pytest.mark.parametrize("C", [3, 50, 70])
def test_restatement_at_w1_is_label_smoothing(C, eps):
    B = 5
    x, y1, y2, _ = _case(C, B, 1.0, 5 * C)
    for kw in (dict(labels2=y2, weight=np.ones(B)), dict(labels2=None, weight=None), dict(labels2=y2)):
        got = ref.soft_ce(x, y1, eps=eps, **kw)
        xt = torch.from_numpy(x).requires_grad_(True)
        loss = torch.nn.functional.cross_entropy(xt, torch.from_numpy(y1), label_smoothing=eps)
        loss.backward()
        assert abs(got["loss"] - float(loss.detach())) <= 1e-12
        assert float(np.abs(got["dlogits"] - xt.grad.numpy()).max()) <= 1e-12


def test_restatement_dominant_label_rule():
    y1, y2 = np.array([1, 1, 1, 1, 2]), np.array([2, 2, 2, 2, 2])
    w = np.array([1.0, 0.5, 0.49999, 0.0, 0.3])
    assert ref.dominant(y1, y2, w).tolist() == [1, 1, 2, 2, 2]          # a tie goes to y1
    assert ref.dominant(y1).tolist() == y1.tolist() and ref.dominant(y1, y2).tolist() == y1.tolist()
    x = np.zeros((5, 3))
    x[:, 1] = 1.0                                                        # argmax is class 1 everywhere
    assert ref.soft_ce(x, y1, y2, w)["correct"] == 2
    x[:, 2] = 1.0                                                        # two maxima: the first one wins
    assert ref.soft_ce(x, y1, y2, w)["correct"] == 2
    x[:, 1] = 0.0
    assert ref.soft_ce(x, y1, y2, w)["correct"] == 3
    # the hard label is the value w = 1, eps = 0 of the target
    t = ref.targets(y1, y2, np.ones(5), 0.0, 4)
    assert np.array_equal(t, np.eye(4)[y1])


# ---- the C ABI -----------------------------------------------------------------------------------------
def test_new_symbols_are_declared_exported_and_bound():
    syms = header_symbols()
    handle = ctypes.CDLL(_lib.LIB_PATH)
    for name in NEW:
        assert name in syms, f"{name} not declared in pca_hip.h"
        assert hasattr(handle, name), f"{name} not exported"
        assert name in _lib.SIGNATURES
        assert getattr(pca_hip.lib(), name).argtypes == _lib.SIGNATURES[name][1]
    # the soft entries take their hard twin's arguments plus the targets
    hard, soft = _lib.SIGNATURES["pca_cross_entropy"][1], _lib.SIGNATURES["pca_cross_entropy_soft"][1]
    assert len(soft) == len(hard) + 1 and soft[:2] == hard[:2] and soft[3:] == hard[2:]
    hard, soft = _lib.SIGNATURES["pca_st_train_fwd_bwd"][1], _lib.SIGNATURES["pca_st_train_fwd_bwd_soft"][1]
    assert len(soft) == len(hard) + 1 and soft[:5] == hard[:5] and soft[6:] == hard[5:]
    hard, soft = _lib.SIGNATURES["pca_frame_points_ex"][1], _lib.SIGNATURES["pca_frame_points_ex_targets"][1]
    assert len(soft) == len(hard) + 3 and soft[:-4] == hard[:-1] and soft[-1] == hard[-1]
    txt = open(os.path.join(os.path.dirname(_lib.LIB_PATH), "..", "..", "include", "pca_hip.h")).read()
    assert "typedef struct PcaSoftTargets {" in txt
    assert ctypes.sizeof(_lib.PcaSoftTargets) == 24
    assert (_lib.PcaSoftTargets.labels2.offset, _lib.PcaSoftTargets.weight.offset,
            _lib.PcaSoftTargets.smoothing.offset) == (0, 8, 16)


def test_abi_version_and_existing_layouts_unchanged():
    assert pca_hip.lib().pca_abi_version() == 2
    assert ctypes.sizeof(_lib.PcaFrameAugEx) == ctypes.sizeof(_lib.PcaFrameAug) + 16 + 64 + 5 * 8 + 8 + 24
    assert ctypes.sizeof(_lib.PcaFrameAugEx) == 200
    assert ctypes.sizeof(_lib.StConfig) == 36


# ---- refusals before any launch ------------------------------------------------------------------------
@pytest.mark.parametrize("eps", [-0.1, 1.0, NAN], ids=["neg", "one", "nan"])
def test_smoothing_out_of_range_is_refused(eps):
    L = pca_hip.lib()
    soft = _lib.PcaSoftTargets(P, P, eps)
    assert L.pca_cross_entropy_soft(P, P, ctypes.byref(soft), 4, 10, 1.0, P, P, None, None) == -1
    msg = L.pca_last_error()
    assert msg.startswith(b"cross_entropy:") and b"smoothing" in msg, msg
    cfg = _lib.StConfig(4, 256, 2, 128, 4, 16, 1, 10, _lib.MODE_BF16)
    for phase in (-1, 0, 1):
        assert L.pca_st_train_fwd_bwd_soft(ctypes.byref(cfg), P, P, None, P, ctypes.byref(soft), P, P, P, P,
                                           1.0, phase, P, None) == -1
        msg = L.pca_last_error()
        assert msg.startswith(b"st_train_fwd_bwd:") and b"smoothing" in msg, msg


AUG = dict(jitter=0, gain_db=0.0, win_lengths=P, n_win=1, norm_mode=0, seed=0, draw=0, draw_dev=None,
           n_speed=1, nwin=0, num_table=0, n_bg=3, ratios=(1.0,), tables=None, bg_waves=P, bg_off=P,
           bg_rms=P, clip_rms=P, bg_max_len=5000, mix_prob=0.5, snr_lo_db=-20.0, snr_hi_db=20.0)


def _frame_call(L, **over):
    """pca_frame_points_ex_targets with valid host arguments and stand-in device addresses, ``over``
    replacing some (as tests/test_frame_aug_host.py calls pca_frame_points_ex)."""
    a = dict(clip_labels=P, labels_out=P, bg_labels=P, labels2_out=P, weight_out=P)
    a.update(over)
    g = AUG
    r = tuple(g["ratios"]) + (1.0,) * (8 - len(g["ratios"]))
    s = _lib.PcaFrameAugEx(g["jitter"], g["gain_db"], g["win_lengths"], g["n_win"], g["norm_mode"], g["seed"],
                           g["draw"], g["draw_dev"], g["n_speed"], g["nwin"], g["num_table"], g["n_bg"],
                           (ctypes.c_double * 8)(*r), g["tables"], g["bg_waves"], g["bg_off"], g["bg_rms"],
                           g["clip_rms"], g["bg_max_len"], g["mix_prob"], g["snr_lo_db"], g["snr_hi_db"])
    return L.pca_frame_points_ex_targets(P, P, P, 2, 9000, 3000, a["clip_labels"], P, 4, 256, 128, 129, 1, P,
                                         None, ctypes.byref(s), P, a["labels_out"], None, None,
                                         a["bg_labels"], a["labels2_out"], a["weight_out"], None)


@pytest.mark.parametrize("over,word", [
    (dict(labels2_out=None), b"go together"),                            # bg_labels without labels2_out
    (dict(weight_out=None), b"go together"),
    (dict(bg_labels=None), b"go together"),
    (dict(bg_labels=None, labels2_out=None), b"go together"),
    (dict(clip_labels=None, labels_out=None), b"need clip_labels"),       # targets without clip_labels
    (dict(clip_labels=None), b"go together"),
], ids=lambda v: None if isinstance(v, bytes) else "-".join(v))
def test_frame_targets_refused_without_gpu(over, word):
    L = pca_hip.lib()
    assert _frame_call(L, **over) == -1
    msg = L.pca_last_error()
    assert msg.startswith(b"frame_points_ex:") and word in msg, msg


# ---- the datasets --------------------------------------------------------------------------------------
def test_dataset_mix_targets_on_the_host():
    import dataset
    clips = [np.zeros(n, dtype=np.float32) for n in (2205, 4851, 16170)]
    y = [3, 1, 4]
    bg = [np.ones(10, np.float32), np.ones(20, np.float32)]
    for mk in (lambda **kw: dataset.ESC_wave_pc(clips, y, 44100, 64, **kw),
               lambda **kw: dataset.ESC_wave_pc_temp(clips, y, 44100, 64, 4, **kw)):
        assert not mk().soft_targets and not mk(mix_clips="self", mix_prob=0.5).soft_targets
        d = mk(mix_clips="self", mix_prob=0.5, mix_targets=True)
        assert d.soft_targets and d.stochastic
        v = d.plain()
        assert not v.soft_targets and not v.stochastic and v.mix_prob == 0.0 and d.soft_targets
        d = mk(mix_clips=bg, mix_prob=0.5, mix_targets=True, mix_labels=[7, 2])
        assert d.soft_targets and d.mix_labels.tolist() == [7, 2] and d.mix_labels.dtype == np.int64
        assert mk(mix_clips="self", mix_targets=True).soft_targets        # mix_prob 0: every weight is 1
        for kw in (dict(mix_targets=True),                                # without mix_clips
                   dict(mix_targets=True, mix_prob=0.0, mix_labels=[1]),
                   dict(mix_clips=bg, mix_prob=0.5, mix_targets=True, mix_labels=[7, 2, 1]),  # wrong length
                   dict(mix_clips=bg, mix_prob=0.5, mix_targets=True, mix_labels=[7]),
                   dict(mix_clips=bg, mix_prob=0.5, mix_targets=True)):   # mix_labels missing for a list
            with pytest.raises(ValueError):
                mk(**kw)
