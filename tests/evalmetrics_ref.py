"""float64 numpy restatement of pca_eval_metrics (include/pca_hip.h), and the seeded inputs of
tests/test_gpu_evalmetrics.py.

Per row: loss = logsumexp(row) - row[label]; pred = the row's argmax as torch.argmax (first maximum, NaN
is the maximum); rank = number of classes that come before the label's class in that order (NaN first,
then the larger value, then the lower index).  A row whose label is outside [0, C) is skipped: loss 0,
rank -1, counted as skipped only.  counts = [scored, top-1 correct, top-k correct, skipped];
confusion[label, pred]; loss_sum = float64 sum of the scored rows' losses.

The logits are float32 values widened to float64, so every comparison (argmax, rank) sees exactly the
values the kernel compares: pred, rank, counts and confusion are exact, no row excused."""
import numpy as np

CLASSES = (1, 2, 10, 50, 64, 65, 300)
N_ROWS = 1037                  # odd: no multiple of the kernels' 128-row blocks, 4-row groups or float4
TOPK = 5


def row_argmax(x):
    """torch.argmax of every row of x [n, C]."""
    nan = np.isnan(x)
    return np.where(nan.any(1), np.argmax(nan, 1), np.argmax(np.where(nan, -np.inf, x), 1))


def eval_metrics_ref(logits, labels, topk):
    x = np.asarray(logits, dtype=np.float64)
    lab = np.asarray(labels, dtype=np.int64)
    n, C = x.shape
    ok = (lab >= 0) & (lab < C)
    safe = np.where(ok, lab, 0)
    rows = np.arange(n)
    with np.errstate(invalid="ignore", divide="ignore", over="ignore"):
        m = np.max(x, axis=1, keepdims=True)                      # np.max propagates NaN
        lse = m[:, 0] + np.log(np.sum(np.exp(x - m), axis=1))
        lv = x[rows, safe]
        loss = np.where(ok, lse - lv, 0.0)
    pred = row_argmax(x).astype(np.int64)
    nan, lnan = np.isnan(x), np.isnan(lv)[:, None]
    j = np.arange(C)[None, :]
    with np.errstate(invalid="ignore"):
        before = np.where(nan != lnan, nan,
                          np.where(~nan & (x != lv[:, None]), x > lv[:, None], j < safe[:, None]))
    before &= j != safe[:, None]
    rank = np.where(ok, before.sum(1), -1).astype(np.int32)
    confusion = np.zeros((C, C), dtype=np.int64)
    np.add.at(confusion, (lab[ok], pred[ok]), 1)
    counts = [int(ok.sum()), int((ok & (rank == 0)).sum()), int((ok & (rank >= 0) & (rank < topk)).sum()),
              int((~ok).sum())]
    return dict(loss=loss, pred=pred, rank=rank, counts=counts, confusion=confusion,
                loss_sum=float(np.sum(loss[ok])) if ok.any() else 0.0)


def random_case(C, n=N_ROWS, seed=None, bad_labels=True):
    """(logits float32 [n, C], labels int64 [n]): N(0, 2) plus 3 on the row's own class; the label is
    that class for most rows, another class for some, and (bad_labels) outside [0, C) for a few."""
    rng = np.random.Generator(np.random.PCG64(1000 + C if seed is None else seed))
    own = rng.integers(0, C, size=n)
    logits = rng.normal(0.0, 2.0, size=(n, C)).astype(np.float32)
    logits[np.arange(n), own] += np.float32(3.0)
    labels = np.where(rng.random(n) < 0.7, own, rng.integers(0, C, size=n)).astype(np.int64)
    if bad_labels and n >= 8:
        where = rng.choice(n, size=max(3, n // 100), replace=False)
        labels[where] = np.resize(np.array([-1, C, C + 7, -2 ** 40, 2 ** 40], dtype=np.int64), where.size)
    return logits, labels


def crafted_case(C):
    """Rows with exactly representable values, C >= 10: ties on the maximum, ties on the label's value on
    both sides of the label, NaN, +inf, -inf.  Returns (logits, labels, expected pred, expected rank)."""
    nan, inf = np.float32("nan"), np.float32("inf")
    rows, labels, pred, rank = [], [], [], []

    def add(lab, p, r, fill=0.0, **kw):
        v = np.full(C, fill, dtype=np.float32)
        for k, val in kw.items():
            v[int(k[1:])] = val
        rows.append(v); labels.append(lab); pred.append(p); rank.append(r)

    add(3, 3, 0, c3=2, c9=2)                       # two equal maxima, the label is the first
    add(9, 3, 1, c3=2, c9=2)                       # ... the label is the second: one class before it
    add(0, 0, 0)                                   # all equal: class 0, and it is the label
    add(5, 0, 5)                                   # all equal, label 5: the five lower classes come first
    add(C - 1, 0, C - 1)                           # all equal, the last class
    add(4, 7, 3, c7=5, c2=1, c4=1, c6=1, c1=3)     # tie on the label's value: 7 and 1 above, 2 ties before, 6 after
    add(6, 2, 0, c2=nan, c6=1)                     # NaN is the maximum; the label is not it: rank counts...
    rank[-1] = 1                                   # ... the NaN only (1 > 0 everywhere else)
    add(2, 2, 0, c2=nan, c8=nan)                   # two NaNs: the first wins, and it is the label
    add(8, 2, 1, c2=nan, c8=nan)                   # the label is the second NaN
    add(1, 5, 1, c5=inf, c1=3)                     # +inf: loss is NaN (inf - inf), the order is still defined
    add(5, 5, 0, c5=inf)
    add(3, 0, 3, fill=-inf)                        # every logit -inf: loss NaN, order by index
    add(3, 3, 0, fill=-inf, c3=0)                  # one finite logit: loss 0
    add(4, 3, C - 1, c4=-inf, c3=1)                # the label at -inf: loss +inf, everything comes first
    add(-1, 3, -1, c3=1)                           # skipped
    add(C, 0, -1)                                  # skipped
    return (np.stack(rows), np.asarray(labels, dtype=np.int64), np.asarray(pred, dtype=np.int64),
            np.asarray(rank, dtype=np.int32))


def cases():
    """name -> (logits, labels, topk): the cases of the GPU test."""
    out = {}
    for C in CLASSES:
        out[f"random_C{C}"] = random_case(C) + (TOPK,)           # topk >= C for C = 1, 2
    for C in (1, 10, 65):
        out[f"one_row_C{C}"] = random_case(C, n=1, seed=77 + C, bad_labels=False) + (TOPK,)
    out["topk_eq_C"] = random_case(10, n=300, seed=5) + (10,)
    out["topk_gt_C"] = random_case(50, n=300, seed=6) + (64,)
    out["top1"] = random_case(64, n=129, seed=7) + (1,)
    for C in (10, 64, 70):
        lg, lab, _, _ = crafted_case(C)
        out[f"crafted_C{C}"] = (lg, lab, 3)
    # the crafted rows in the middle of ordinary ones (block edges on both sides)
    lg, lab = random_case(50, n=400, seed=8)
    cl, clab, _, _ = crafted_case(50)
    out["mixed_C50"] = (np.concatenate([lg[:130], cl, lg[130:]]), np.concatenate([lab[:130], clab, lab[130:]]), TOPK)
    return out
