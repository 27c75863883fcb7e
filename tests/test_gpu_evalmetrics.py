"""pca_eval_metrics on the device against the float64 restatement tests/evalmetrics_ref.py.

row_pred, row_rank, the counters and the confusion matrix are compared exactly for every case (both sides
compare the same fp32 values: no row is excused); row_loss to the fp32 forward bar of
tests/test_gpu_clip.py, 1e-4 of max(1, max|ref|) over the finite entries with NaN and inf in the same
places; loss_sum / n to the same bar."""
import numpy as np
import pytest
import torch

import evalmetrics_ref as er
from util import T

pytestmark = pytest.mark.gpu

TOL = 1e-4
CASES = er.cases()


@pytest.fixture(scope="module")
def dev():
    return torch.device("cuda", 0)


def _bufs(C, dev, slots=1):
    return (torch.zeros(4 * slots, dtype=torch.int64, device=dev),
            torch.zeros((C, C), dtype=torch.int64, device=dev),
            torch.zeros(1, dtype=torch.float64, device=dev))


def _check_loss(got, ref, what):
    """1e-4 of max(1, max|ref|) over the finite entries; NaN, +inf and -inf where the reference's are."""
    got = np.asarray(got, dtype=np.float64)
    fin = np.isfinite(ref)
    assert np.array_equal(np.isnan(got), np.isnan(ref)), what
    assert np.array_equal(np.isposinf(got), np.isposinf(ref)), what
    assert np.array_equal(np.isneginf(got), np.isneginf(ref)), what
    if not fin.any():
        return
    scale = max(1.0, float(np.abs(ref[fin]).max()))
    err = float(np.abs(got[fin] - ref[fin]).max())
    print(f"{what}: max|loss - ref| = {err:.3e} (bar {TOL * scale:.3e})")
    assert err <= TOL * scale, (what, err, scale)


@pytest.mark.parametrize("name", list(CASES))
def test_eval_metrics_matches_float64_reference(name, dev):
    import pca_hip
    logits, labels, topk = CASES[name]
    n, C = logits.shape
    ref = er.eval_metrics_ref(logits, labels, topk)
    counts, conf, lsum = _bufs(C, dev, 2)
    loss, pred, rank = pca_hip.eval_metrics(T(logits, dev), T(labels, dev), topk, counts, 1, conf, lsum,
                                            rows=True)
    assert loss.dtype == torch.float32 and pred.dtype == torch.int64 and rank.dtype == torch.int32
    assert np.array_equal(pred.cpu().numpy(), ref["pred"])
    assert np.array_equal(rank.cpu().numpy(), ref["rank"])
    assert counts.tolist() == [0, 0, 0, 0] + ref["counts"]
    assert np.array_equal(conf.cpu().numpy(), ref["confusion"])
    _check_loss(loss.cpu().numpy(), ref["loss"], name)
    scored = max(ref["counts"][0], 1)
    _check_loss(np.array([float(lsum) / scored]), np.array([ref["loss_sum"] / scored]), name + " loss_sum / n")


def test_crafted_rows_by_hand(dev):
    """The expected predictions and ranks written next to the rows (not computed by the restatement), on
    both kernels: C = 10 and 64 a lane per row, C = 70 a wave per row."""
    import pca_hip
    for C in (10, 64, 70):
        logits, labels, want_pred, want_rank = er.crafted_case(C)
        _, pred, rank = pca_hip.eval_metrics(T(logits, dev), T(labels, dev), 3, rows=True)
        assert pred.tolist() == want_pred.tolist(), C
        assert rank.tolist() == want_rank.tolist(), C


def test_outputs_are_optional_and_unaligned_logits_work(dev):
    """Each accumulator alone gives what all together give; a logit buffer that is not 16-byte aligned
    (a row slice of odd C) takes the scalar staging path."""
    import pca_hip
    logits, labels, topk = CASES["random_C50"]
    ref = er.eval_metrics_ref(logits, labels, topk)
    lg, lab = T(logits, dev), T(labels, dev)
    counts, conf, lsum = _bufs(50, dev)
    assert pca_hip.eval_metrics(lg, lab, topk, counts=counts) is None
    pca_hip.eval_metrics(lg, lab, topk, confusion=conf)
    pca_hip.eval_metrics(lg, lab, topk, loss_sum=lsum)
    both = _bufs(50, dev)
    pca_hip.eval_metrics(lg, lab, topk, both[0], 0, both[1], both[2])
    assert counts.tolist() == both[0].tolist() == ref["counts"]
    assert torch.equal(conf, both[1]) and torch.equal(lsum.view(torch.int64), both[2].view(torch.int64))
    lg7 = np.ascontiguousarray(CASES["random_C65"][0][:, :63])
    lab7 = CASES["random_C65"][1] % 63
    big = T(lg7, dev)
    off = big[1:]                                              # 63 floats in: 4-byte aligned only
    assert off.data_ptr() % 16 != 0 and off.is_contiguous()
    ref7 = er.eval_metrics_ref(lg7[1:], lab7[1:], 5)
    c7, f7, s7 = _bufs(63, dev)
    loss, pred, rank = pca_hip.eval_metrics(off, T(lab7[1:], dev), 5, c7, 0, f7, s7, rows=True)
    assert np.array_equal(pred.cpu().numpy(), ref7["pred"]) and np.array_equal(rank.cpu().numpy(), ref7["rank"])
    assert c7.tolist() == ref7["counts"] and np.array_equal(f7.cpu().numpy(), ref7["confusion"])
    _check_loss(loss.cpu().numpy(), ref7["loss"], "unaligned C=63")


@pytest.mark.parametrize("C", [50, 300])
def test_reproducible_captured_and_accumulating(C, dev):
    import pca_hip
    logits, labels, topk = CASES[f"random_C{C}"]
    ref = er.eval_metrics_ref(logits, labels, topk)
    lg, lab = T(logits, dev), T(labels, dev)

    def once():
        counts, conf, lsum = _bufs(C, dev)
        rows = pca_hip.eval_metrics(lg, lab, topk, counts, 0, conf, lsum, rows=True)
        return rows[0].view(torch.int32).clone(), lsum.view(torch.int64).clone()

    a, b = once(), once()
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])        # the same bits
    # counts and confusion accumulate over calls and slots; the other slots are not touched
    counts, conf, lsum = _bufs(C, dev, 3)
    for _ in range(3):
        pca_hip.eval_metrics(lg, lab, topk, counts, 0, conf, lsum)
    pca_hip.eval_metrics(lg, lab, topk, counts, 2, conf, lsum)
    pca_hip.eval_metrics(lg, lab, topk)
    assert counts.tolist() == [3 * v for v in ref["counts"]] + [0] * 4 + ref["counts"]
    assert np.array_equal(conf.cpu().numpy(), 4 * ref["confusion"])
    one = a[1].view(torch.float64)
    assert float(lsum) == float(((one + one) + one) + one)            # four adds of the same fp64 sum
    # captured into a graph: every replay gives the eager call's bits and adds the same counts
    cg, fg, sg = _bufs(C, dev)
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        pca_hip.eval_metrics(lg, lab, topk, cg, 0, fg, sg, rows=True)   # warm-up outside the capture
    torch.cuda.current_stream().wait_stream(s)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        got = pca_hip.eval_metrics(lg, lab, topk, cg, 0, fg, sg, rows=True)
    seen = []
    for _ in range(2):
        cg.zero_(); fg.zero_(); sg.zero_()
        for t in got:
            t.zero_()
        graph.replay()
        torch.cuda.synchronize()
        seen.append((got[0].view(torch.int32).clone(), sg.view(torch.int64).clone()))
        assert cg.tolist() == ref["counts"] and np.array_equal(fg.cpu().numpy(), ref["confusion"])
    for r in seen:
        assert torch.equal(r[0], a[0]) and torch.equal(r[1], a[1])
