"""float64 numpy restatement of pca_clip_aggregate (include/pca_hip.h), and the seeded inputs of
tests/test_gpu_clip.py.

Per row: log_softmax = (x - max) - log(sum(exp(x - max))); the row's argmax as torch.argmax (first
maximum, NaN is the maximum).  Per clip: mean of the log_softmax rows, votes = histogram of the row
argmaxes, pred[0] by votes (ties: the higher mean log-prob in argmax order, then the lower class),
pred[1] = argmax of the mean.  A clip without rows: zeros and pred -1."""
import numpy as np

LENGTHS = (0, 1, 3, 4, 5, 216, 431, 5000)       # segment lengths of the GPU test
CLASSES = (1, 10, 50, 257)
SEEDS = {1: 11, 10: 12, 50: 13, 257: 14}        # chosen so that no clip is left out (see left_out)
MARGIN = 1e-3                                   # float64 top-2 margin in mean log-prob


def argmax_torch(v):
    """torch.argmax of a 1-D array: the first NaN if there is one, else the first maximum."""
    v = np.asarray(v)
    nan = np.isnan(v)
    return int(np.argmax(nan)) if nan.any() else int(np.argmax(v))


def row_argmax(x):
    """argmax_torch of every row of x [n, C]."""
    nan = np.isnan(x)
    return np.where(nan.any(1), np.argmax(nan, 1), np.argmax(np.where(nan, -np.inf, x), 1))


def log_softmax(x):
    """Rows of x [n, C] in float64; a NaN (or +inf) in a row makes the row NaN, as in torch."""
    x = np.asarray(x, dtype=np.float64)
    with np.errstate(invalid="ignore", divide="ignore", over="ignore"):
        z = x - np.max(x, axis=1, keepdims=True)            # np.max propagates NaN
        return z - np.log(np.sum(np.exp(z), axis=1, keepdims=True))


def clip_ref(logits, offsets, labels=None):
    """logits [n_sets, C], offsets [n_clips + 1] -> dict(mean [n_clips, C] float64, votes
    [n_clips, C] int64, pred [n_clips, 2] int64, counts [2] (with labels: clips each rule gets right),
    frame_argmax [n_sets])."""
    logits = np.asarray(logits)
    offsets = np.asarray(offsets, dtype=np.int64)
    n_clips, C = offsets.size - 1, logits.shape[1]
    mean = np.zeros((n_clips, C))
    votes = np.zeros((n_clips, C), dtype=np.int64)
    pred = np.full((n_clips, 2), -1, dtype=np.int64)
    am = row_argmax(logits) if logits.shape[0] else np.zeros(0, dtype=np.int64)
    for c in range(n_clips):
        a, b = int(offsets[c]), int(offsets[c + 1])
        if b <= a:
            continue
        with np.errstate(invalid="ignore"):
            mean[c] = log_softmax(logits[a:b]).sum(0) / (b - a)
        votes[c] = np.bincount(am[a:b], minlength=C)
        top = np.flatnonzero(votes[c] == votes[c].max())
        pred[c, 0] = top[argmax_torch(mean[c, top])]
        pred[c, 1] = argmax_torch(mean[c])
    out = dict(mean=mean, votes=votes, pred=pred, frame_argmax=am)
    if labels is not None:
        lab = np.asarray(labels, dtype=np.int64)
        out["counts"] = [int(((pred[:, r] == lab) & (pred[:, r] >= 0)).sum()) for r in (0, 1)]
    return out


def left_out(ref):
    """Clips whose predictions a float32 implementation may legitimately give differently: a vote tie
    (broken by the mean's last bits) or a float64 top-2 margin of the mean log-prob below MARGIN.
    Boolean [n_clips]; clips without rows and C = 1 are never left out."""
    mean, votes, pred = ref["mean"], ref["votes"], ref["pred"]
    out = np.zeros(mean.shape[0], dtype=bool)
    if mean.shape[1] < 2:
        return out
    for c in range(mean.shape[0]):
        if pred[c, 0] < 0:
            continue
        v = np.sort(votes[c])
        m = np.sort(mean[c])
        out[c] = v[-1] == v[-2] or not (m[-1] - m[-2] >= MARGIN)
    return out


def gpu_case(C):
    """(logits float32 [n_sets, C], offsets int64, labels int64) of the GPU test for C classes: 16
    clips, every length of LENGTHS once and eight more drawn from it, in a seeded order.  A clip's
    rows are N(0, 1) plus 4 on the clip's own class, so that frames mostly agree and the seeds of
    SEEDS leave no vote tied and no mean within MARGIN; the label is that class for most clips."""
    rng = np.random.Generator(np.random.PCG64(SEEDS[C]))
    lens = np.concatenate([np.asarray(LENGTHS), rng.choice(LENGTHS, size=8)])
    lens = lens[rng.permutation(lens.size)]
    offsets = np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)
    own = rng.integers(0, C, size=lens.size)
    logits = rng.normal(0.0, 1.0, size=(int(offsets[-1]), C)).astype(np.float32)
    for c, k in enumerate(own):
        logits[offsets[c]:offsets[c + 1], k] += np.float32(4.0)
    labels = np.where(rng.random(lens.size) < 0.7, own, rng.integers(0, C, size=lens.size))
    return logits, offsets, labels.astype(np.int64)


def crafted_case():
    """Ties with exactly representable logits, C = 10.  A row whose classes other than two are -inf
    has exp terms {1, e^-1, 0, ...}: its sum is the same in any order, so two such rows that mirror
    each other give bit-equal log-probs to the two classes in float32 and float64 alike.
    Returns (logits float32, offsets, expected pred [n_clips, 2], expected votes rows as dicts)."""
    ninf = -np.inf
    C = 10

    def two(a, va, b, vb):
        r = np.full(C, ninf, dtype=np.float32)
        r[a], r[b] = va, vb
        return r

    def flat(**kw):
        r = np.zeros(C, dtype=np.float32)
        for k, v in kw.items():
            r[int(k[1:])] = v
        return r

    clips = [
        # full tie, two mirrored rows: votes 3 and 7 once each, equal means -> the lower class
        [two(3, 1, 7, 0), two(3, 0, 7, 1)],
        # the same tie over eight rows, ordered so that every partial sum meets a mirrored twin
        [two(7, 2, 4, 0), two(7, 0, 4, 2)] * 2 + [two(7, 0, 4, 2), two(7, 2, 4, 0)] * 2,
        # vote tie 2 : 2 between classes 8 and 1; class 8 is far ahead in mean log-prob
        [flat(c8=8), flat(c8=8), flat(c1=0.25), flat(c1=0.25)],
        # every log-prob -inf: votes tied between 5 and 2, means tied at -inf -> class 2
        [two(5, 0, 5, 0), two(2, 0, 2, 0)],
        # a NaN frame: its argmax is the NaN's class; the clip's mean is NaN everywhere, so the vote
        # tie 4 : 6 goes to class 4 and the mean rule to class 0
        [flat(c6=float("nan")), flat(c4=3)],
        # no rows
        [],
        # one frame, two equal maxima: the first wins
        [flat(c3=2, c9=2)],
        # all rows equal everywhere: class 0
        [flat()] * 5,
    ]
    pred = np.array([[3, 3], [4, 4], [8, 8], [2, 0], [4, 0], [-1, -1], [3, 3], [0, 0]], dtype=np.int64)
    votes = [{3: 1, 7: 1}, {7: 4, 4: 4}, {8: 2, 1: 2}, {5: 1, 2: 1}, {6: 1, 4: 1}, {}, {3: 1}, {0: 5}]
    lens = [len(c) for c in clips]
    offsets = np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)
    logits = np.stack([r for c in clips for r in c]).astype(np.float32)
    return logits, offsets, pred, votes
