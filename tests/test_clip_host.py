"""Clip-level aggregation without a GPU: the C ABI of pca_clip_aggregate (declared, exported, arguments
refused before anything is launched), the float64 restatement tests/clip_ref.py against a hand-worked
example, and the conditions on the inputs of tests/test_gpu_clip.py that let it compare predictions."""
import ctypes
import math
import os
import re

import numpy as np
import pytest
import torch

import clip_ref as cr
import pca_hip
from pca_hip import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ---- the C ABI ---------------------------------------------------------------------------------------
def test_header_declares_and_library_exports_clip_aggregate():
    txt = open(os.path.join(ROOT, "include", "pca_hip.h")).read()
    comment = re.search(r"/\*((?:(?!\*/).)*?)\*/\s*int pca_clip_aggregate\s*\(", txt, flags=re.S)
    assert comment, "pca_clip_aggregate not declared (with its comment) in pca_hip.h"
    assert "Code/pceval.py:95" in comment.group(1) and "replaces: nothing" in comment.group(1)
    handle = ctypes.CDLL(_lib.LIB_PATH)
    assert hasattr(handle, "pca_clip_aggregate"), "pca_clip_aggregate not exported"
    assert "pca_clip_aggregate" in _lib.SIGNATURES
    assert callable(pca_hip.clip_aggregate)
    assert pca_hip.lib().pca_abi_version() == 2


def test_clip_aggregate_refuses_bad_arguments_without_a_gpu():
    L = pca_hip.lib()
    p = 4096          # a non-null value that is never dereferenced: the checks come before any launch

    def call(logits=p, n_sets=100, C=10, off=p, n_clips=4, labels=None, mean=p, votes=p, pred=p,
             counts=None, slot=0):
        rc = L.pca_clip_aggregate(logits, n_sets, C, off, n_clips, labels, mean, votes, pred, counts,
                                  slot, None)
        return rc, L.pca_last_error()

    for kw in (dict(logits=None), dict(off=None)):
        rc, msg = call(**kw)
        assert rc == -1 and b"null pointer" in msg, (kw, msg)
    for kw, word in ((dict(n_clips=-1), b"n_clips=-1"), (dict(C=0), b"C=0"), (dict(C=-3), b"C=-3"),
                     (dict(n_sets=-1), b"n_sets=-1"), (dict(labels=p, counts=p, slot=-1), b"slot=-1")):
        rc, msg = call(**kw)
        assert rc == -1 and word in msg, (kw, msg)
    for kw in (dict(labels=p), dict(counts=p)):
        rc, msg = call(**kw)
        assert rc == -1 and b"labels and counts go together" in msg, (kw, msg)
    # nothing to do is not an error, and still launches nothing
    assert call(n_clips=0) [0] == 0


def test_clip_aggregate_on_cpu_tensors_raises():
    lg = torch.zeros(4, 3)
    off = torch.tensor([0, 4])
    with pytest.raises(pca_hip.PcaHipError):
        pca_hip.clip_aggregate(lg, off)


def test_clip_accuracy_is_exported_with_the_documented_arguments():
    import inspect

    import evalsweep
    assert "clip_accuracy" in evalsweep.__all__
    p = inspect.signature(evalsweep.clip_accuracy).parameters
    assert list(p)[:5] == ["model", "clips", "labels", "fs", "N"]
    for name in ("Ntemp", "n_fft", "trim_dB", "batch_size", "json_file"):
        assert p[name].default is None, name
    assert "mode" in p


# ---- the restatement against a hand-worked example ----------------------------------------------------
def test_clip_ref_hand_worked():
    """Three classes; rows given as log-probabilities (ln p with sum p = 1), so that log_softmax of a
    row is the row itself and the means below follow by hand."""
    ln = math.log
    nan, ninf = float("nan"), float("-inf")
    rows = [
        # clip 0: votes 1 : 1 between classes 0 and 1.  mean[0] = ln(.5 * .125) / 2 = ln .25,
        # mean[1] = ln(.25 * .75) / 2 = ln(.1875) / 2 > mean[0], mean[2] = ln(.25 * .125) / 2:
        # the vote tie goes to class 1 (by index it would be class 0)
        [ln(.5), ln(.25), ln(.25)],
        [ln(.125), ln(.75), ln(.125)],
        # clip 1: rows (1, 0, -inf) and (0, 1, -inf): one vote each for classes 0 and 1, both means
        # -(1 + 2 ln(1 + 1/e)) / 2, class 2 at -inf: a full tie, class 0
        [1.0, 0.0, ninf],
        [0.0, 1.0, ninf],
        # clip 2: no rows
        # clip 3: one row, p = (.25, .25, .5)
        [ln(.25), ln(.25), ln(.5)],
        # clip 4: a NaN frame votes for the NaN's class (1) and makes every mean NaN; the other frame
        # votes for class 2: tie 1 : 1 between classes 1 and 2 with equal (NaN) means -> class 1;
        # the mean rule takes the first NaN, class 0
        [0.0, nan, 0.0],
        [0.0, 0.0, 2.0],
    ]
    off = [0, 2, 4, 4, 5, 7]
    labels = [1, 0, 0, 2, 0]
    r = cr.clip_ref(np.array(rows, dtype=np.float64), off, labels)
    assert r["frame_argmax"].tolist() == [0, 1, 0, 1, 2, 1, 2]
    assert r["votes"].tolist() == [[1, 1, 0], [1, 1, 0], [0, 0, 0], [0, 0, 1], [0, 1, 1]]
    assert r["pred"].tolist() == [[1, 1], [0, 0], [-1, -1], [2, 2], [1, 0]]
    m = r["mean"]
    np.testing.assert_allclose(m[0], [ln(.25), ln(.1875) / 2, ln(.03125) / 2], rtol=1e-14)
    t = -(1 + 2 * ln(1 + math.exp(-1))) / 2
    assert m[1, 0] == m[1, 1] and abs(m[1, 0] - t) < 1e-15 and m[1, 2] == ninf
    assert m[2].tolist() == [0, 0, 0]
    np.testing.assert_allclose(m[3], [ln(.25), ln(.25), ln(.5)], rtol=1e-14)
    assert np.isnan(m[4]).all()
    # clip 0 vote + mean, clip 1 both, clip 3 both; clip 2 (no rows) is not tallied; clip 4: mean rule only
    assert r["counts"] == [3, 4]


def test_clip_ref_agrees_with_torch_on_random_rows():
    g = torch.Generator().manual_seed(1)
    x = torch.randn(40, 7, generator=g, dtype=torch.float64)
    x[3, 2] = float("nan")
    x[9, :] = 1.5
    np.testing.assert_allclose(cr.log_softmax(x.numpy())[4:], torch.log_softmax(x, 1).numpy()[4:],
                               rtol=1e-13, atol=1e-13)
    assert np.isnan(cr.log_softmax(x.numpy())[3]).all()
    assert cr.row_argmax(x.numpy()).tolist() == x.argmax(1).tolist()


# ---- the GPU test's inputs: conditions on the inputs, not tolerances on the kernel --------------------
@pytest.mark.parametrize("C", cr.CLASSES)
def test_gpu_cases_leave_no_clip_out(C):
    logits, off, labels = cr.gpu_case(C)
    lens = np.diff(off)
    assert set(lens.tolist()) == set(cr.LENGTHS) and logits.dtype == np.float32
    assert logits.shape == (off[-1], C) and labels.shape == (lens.size,)
    ref = cr.clip_ref(logits, off, labels)
    assert not cr.left_out(ref).any()
    n = int((lens > 0).sum())
    if C > 1:
        assert 0 < ref["counts"][0] < n and 0 < ref["counts"][1] < n      # a tally that can be wrong


def test_crafted_case_is_what_its_comments_say():
    logits, off, pred, votes = cr.crafted_case()
    ref = cr.clip_ref(logits, off)
    assert ref["pred"].tolist() == pred.tolist()
    for c, v in enumerate(votes):
        want = np.zeros(logits.shape[1], dtype=np.int64)
        for k, n in v.items():
            want[k] = n
        assert ref["votes"][c].tolist() == want.tolist(), c
    m = ref["mean"]
    assert m[0, 3] == m[0, 7] and m[1, 4] == m[1, 7]                      # the exact ties
    assert m[2, 8] - m[2, 1] > 1 and np.isneginf(m[3]).all() and np.isnan(m[4]).all()
