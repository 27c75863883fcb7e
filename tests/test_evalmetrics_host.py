"""pca_eval_metrics and the exact-resume index logic without a GPU: the C ABI (declared with its comment,
exported, arguments refused before anything is launched), the float64 restatement
tests/evalmetrics_ref.py against torch on the CPU and against hand-worked rows, and
ShardedIndexStream restored from (seed, epoch, cursor)."""
import ctypes
import inspect
import os
import re

import numpy as np
import pytest
import torch

import evalmetrics_ref as er
import pca_hip
from pca_hip import _lib, trainer

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ---- the C ABI ---------------------------------------------------------------------------------------
def test_header_declares_and_library_exports_eval_metrics():
    txt = open(os.path.join(ROOT, "include", "pca_hip.h")).read()
    comment = re.search(r"/\*((?:(?!\*/).)*?)\*/\s*int pca_eval_metrics\s*\(", txt, flags=re.S)
    assert comment, "pca_eval_metrics not declared (with its comment) in pca_hip.h"
    assert "replaces: Code/settransformer.py:121-130" in comment.group(1)
    assert re.search(r"size_t pca_eval_metrics_ws_bytes\s*\(", txt)
    handle = ctypes.CDLL(_lib.LIB_PATH)
    for name in ("pca_eval_metrics", "pca_eval_metrics_ws_bytes"):
        assert hasattr(handle, name), f"{name} not exported"
        assert name in _lib.SIGNATURES
    assert callable(pca_hip.eval_metrics)
    p = inspect.signature(pca_hip.eval_metrics).parameters
    assert list(p) == ["logits", "labels", "topk", "counts", "slot", "confusion", "loss_sum", "rows"]
    assert p["topk"].default == 5 and p["rows"].default is False
    assert pca_hip.lib().pca_abi_version() == 2
    src = open(os.path.join(ROOT, "point-cloud-audio_amd", "csrc", "evalmetrics.hip")).read()
    assert "replaces: Code/settransformer.py:121-130" in src


def test_eval_metrics_refuses_bad_arguments_without_a_gpu():
    L = pca_hip.lib()
    p = 4096          # a non-null value that is never dereferenced: the checks come before any launch

    def call(logits=p, labels=p, n_rows=100, C=10, topk=5, counts=None, slot=0, loss_sum=None, ws=None):
        rc = L.pca_eval_metrics(logits, labels, n_rows, C, topk, p, p, p, counts, slot, None, loss_sum,
                                ws, None)
        return rc, L.pca_last_error()

    for kw in (dict(logits=None), dict(labels=None)):
        rc, msg = call(**kw)
        assert rc == -1 and b"null pointer" in msg, (kw, msg)
    for kw, word in ((dict(n_rows=-1), b"n_rows=-1"), (dict(C=0), b"C=0"), (dict(C=-3), b"C=-3"),
                     (dict(topk=0), b"topk=0"), (dict(slot=-1), b"slot=-1")):
        rc, msg = call(**kw)
        assert rc == -1 and word in msg, (kw, msg)
    for kw in (dict(counts=p), dict(loss_sum=p)):
        rc, msg = call(**kw)
        assert rc == -1 and b"need the workspace" in msg, (kw, msg)
    # nothing to do is not an error, and still launches nothing
    assert call(n_rows=0)[0] == 0
    assert call(n_rows=0, logits=None, labels=None, counts=p)[0] == 0
    assert L.pca_eval_metrics_ws_bytes(0) == 0
    assert 0 < L.pca_eval_metrics_ws_bytes(1) <= L.pca_eval_metrics_ws_bytes(10 ** 7) <= 1 << 16


def test_eval_metrics_on_cpu_tensors_raises():
    with pytest.raises(pca_hip.PcaHipError):
        pca_hip.eval_metrics(torch.zeros(4, 3), torch.zeros(4, dtype=torch.int64))


# ---- the restatement ---------------------------------------------------------------------------------
@pytest.mark.parametrize("C", er.CLASSES)
def test_ref_agrees_with_torch_in_float64(C):
    logits, labels = er.random_case(C)
    ref = er.eval_metrics_ref(logits, labels, er.TOPK)
    ok = (labels >= 0) & (labels < C)
    assert 0 < (~ok).sum() < 30 and ref["counts"][3] == int((~ok).sum())
    x = torch.from_numpy(logits).double()
    ce = torch.nn.functional.cross_entropy(x[ok], torch.from_numpy(labels[ok]), reduction="none")
    np.testing.assert_allclose(ref["loss"][ok], ce.numpy(), rtol=1e-12, atol=1e-12)
    assert (ref["loss"][~ok] == 0).all() and (ref["rank"][~ok] == -1).all()
    assert abs(ref["loss_sum"] - float(ce.sum())) <= 1e-9 * max(1.0, abs(float(ce.sum())))
    assert ref["pred"].tolist() == x.argmax(1).tolist()
    # rank against a sort: the label's position in the stable descending order (no NaN here)
    order = np.argsort(-logits.astype(np.float64), axis=1, kind="stable")
    pos = np.argmax(order == np.where(ok, labels, 0)[:, None], axis=1)
    assert np.array_equal(ref["rank"][ok], pos[ok])
    assert np.array_equal(ref["rank"][ok] == 0, ref["pred"][ok] == labels[ok])
    # confusion against a histogram
    want = np.histogram2d(labels[ok], ref["pred"][ok], bins=(np.arange(C + 1), np.arange(C + 1)))[0]
    assert np.array_equal(ref["confusion"], want.astype(np.int64))
    n = int(ok.sum())
    assert ref["counts"][0] == n == int(ref["confusion"].sum())
    assert ref["counts"][1] == int(np.trace(ref["confusion"]))
    assert ref["counts"][2] == int((pos[ok] < er.TOPK).sum())
    if C > er.TOPK:
        assert 0 < ref["counts"][1] < ref["counts"][2] < n          # figures that can be wrong
    else:
        assert ref["counts"][2] == n                                  # topk >= C: every scored row


@pytest.mark.parametrize("C", [10, 64, 70])
def test_crafted_case_is_what_its_comments_say(C):
    logits, labels, pred, rank = er.crafted_case(C)
    ref = er.eval_metrics_ref(logits, labels, 3)
    assert ref["pred"].tolist() == pred.tolist()
    assert ref["rank"].tolist() == rank.tolist()
    loss = ref["loss"]
    assert np.isnan(loss[[6, 7, 8, 9, 10, 11]]).all() and loss[12] == 0 and np.isposinf(loss[13])
    assert loss[14] == 0 and loss[15] == 0 and ref["counts"][3] == 2
    np.testing.assert_allclose(loss[2], np.log(C), rtol=1e-14)
    np.testing.assert_allclose(loss[0], np.log(2 + (C - 2) * np.exp(-2.0)), rtol=1e-14)


def test_cases_cover_what_the_issue_lists():
    cs = er.cases()
    Cs = {v[0].shape[1] for v in cs.values()}
    assert set(er.CLASSES) <= Cs
    assert any(v[0].shape[0] == 1 for v in cs.values())
    assert all(v[0].dtype == np.float32 and v[1].dtype == np.int64 for v in cs.values())
    assert any(v[2] > v[0].shape[1] for v in cs.values()) and any(v[2] == v[0].shape[1] for v in cs.values())
    for n in (v[0].shape[0] for k, v in cs.items() if k.startswith("random")):
        assert n % 128 and n % 64 and n % 4


# ---- the index stream restored from (seed, epoch, cursor) --------------------------------------------
@pytest.mark.parametrize("world", [1, 2])
@pytest.mark.parametrize("shuffle", [True, False])
@pytest.mark.parametrize("taken", [0, 3, 7, 14, 17])      # 7 batches per epoch: mid-epoch and boundaries
def test_index_stream_restored_hands_out_the_remaining_batches(world, shuffle, taken):
    n, B = 59 * world + 1, 8                                # 59 per rank: 7 batches, 3 indices dropped
    for rank in range(world):
        a = trainer.ShardedIndexStream(n, B, rank, world, seed=5, shuffle=shuffle)
        assert a.steps_per_epoch() == 7
        for _ in range(taken):
            a.next()
        st = a.state()
        assert set(st) == {"seed", "epoch", "cursor"} and all(type(v) is int for v in st.values())
        b = trainer.ShardedIndexStream(n, B, rank, world, seed=999, shuffle=shuffle)
        b.load_state(st)
        for _ in range(16):
            assert torch.equal(a.next(), b.next())
        assert a.state() == b.state()


def test_index_stream_restored_after_next_epoch():
    """The Trainer's cursor mode takes whole epochs (next_epoch): restored, the stream re-derives the
    epoch's permutation, and the next call starts the following epoch."""
    a = trainer.ShardedIndexStream(100, 8, 1, 2, seed=3)
    a.next_epoch()
    ep = a.next_epoch()
    b = trainer.ShardedIndexStream(100, 8, 1, 2, seed=0)
    b.load_state(a.state())
    assert torch.equal(b._perm[:ep.numel()], ep)
    assert torch.equal(a.next_epoch(), b.next_epoch())


def test_checkpoint_entry_points_exist():
    import runfiles
    assert {"save_checkpoint", "load_checkpoint"} <= set(runfiles.__all__)
    for name in ("state_dict", "load_state_dict", "fit"):
        assert callable(getattr(trainer.Trainer, name))
    p = inspect.signature(trainer.Trainer.fit).parameters
    assert list(p)[1:] == ["epochs", "test_dataset", "eval_every", "checkpoint_path", "checkpoint_every", "log"]
    assert p["eval_every"].default == 10
    p = inspect.signature(trainer.Evaluator.__init__).parameters
    assert list(p)[1:] == ["model", "dataset", "batch_size", "mode", "topk", "process_group"]
