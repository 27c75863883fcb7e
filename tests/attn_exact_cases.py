"""Exact-operand inputs for the fused attention blocks: softmax rows that are one-hot or exact 2- / 4-way
ties, built so that no operand rounding of any kernel family changes a number.  numpy / torch on the CPU
only; test_attn_exact_host.py checks the conditions below with the references, test_gpu_attn_exact.py runs
the kernels on the same inputs.

The code design (every d -> d block).  A head slice of dh columns is a *code* half (c = dh / 2 columns)
and a *payload* half; the payload's first column is the offset column, the others hold integers in
[-8, 8].  fc_q = I, fc_k = I on the code columns and the offset column, fc_v = I on the other payload
columns, fc_o = a signed permutation, fc_o.bias = 1/8, every other bias 0.  Codes are rows of the c x c
Hadamard matrix times a gain (g_k = 8, d = 64: 16, on the keys; g_q of query_gain() on the queries), so
<Q_h, K_h> / sqrt(d) is g_q g_k c / sqrt(d) (>= 64 nats, asserted) where the codes match and exactly 0 where
they do not.  Code 0 is the decoy code:
most keys carry it, no query asks for it.  The P codes 1 .. P are asked for; each is planted on 1, 2 or 4
live keys (never 3).  The last code of the book is owned by no key and asked for by no query (a shared
query meets sets of every length, and a row of L equal scores is exact only for L in {1, 2, 4}).  Every
softmax row is then 1, 1/2 or 1/4 on its planted keys and below exp(-64) elsewhere, tied keys have
identical code columns (bit-identical scores in any arithmetic, the reassociated G' = sl2e Qp_h Wk_h of
the few-queries kernels included: its bf16 rounding is one common factor on entries of equal mantissa),
and O = Qp + A Vp has at most two fractional bits below 64: exact in bf16.

The backward kernels feed dS = A (dA - sum A dA) / sqrt(d) to the MFMA in bf16 as well, and on a key column
that is the same in every key (the offset column, column 0 of the Hadamard codes) the exact dQ is the total
cancellation sum_n dS_n = 0, which a rounding of dS breaks in proportion to that column's size.  So tie
partners share their payload but for its first column, where partner i holds base + i: dS is then
dO_c (2 i - 1) / 4 or dO_c (4 i - 6) / 16 over sqrt(d), values that come in exact +- pairs, whose roundings
cancel as the values do.  (With independent payloads of the partners dS reaches the hundreds and dQ of the
many-queries blocks was off by up to 9.4e-2 of its maximum under the offset: a property of bf16 operands on
this input, not a fault of a kernel.)

Planted positions, L the live length of a set: the pool starts with 0, L - 1, 15, 16, 127, 128 and the
first index of the last 128-tile, then a seeded permutation of the rest.  The codes take the pool in
passes (every code once, then the codes of multiplicity >= 2, then the 4-fold ones twice), so tie partners
land in different 128-tiles and split ranges, and the multiplicities rotate with head and set so that
sole winners sit at index 0 (every later exponential underflows) and in the last tile (the accumulated
decoy sum is rescaled to nothing) - has_structure() says which of these a case really has.  Behind a
set's length every key carries an asked code: the keys at index L and N - 1 the first two, so a mask that
lets one of them through halves a weight.

The offset variant (offset_values()) writes a = 4 g_q (d = 64: 2 g_q) into the offset column of every query
and +-b into the offset column of every key, b the smallest multiple of 4 with a b / sqrt(d) >= 96: all scores
of a row move by the same +-96 (d = 64), +-98.2 (d = 256) or +-98.6 nats (d = 128).  The query's column always holds a; the key's column is 0 in the other
runs.  fc_k.bias is not used: the reassociated
kernels drop it, as they may.

Self-attention (Q = K = X): the slice is [query code cc | key code cc | payload], fc_q and fc_k select
their block into the same cc code dims (dh = 32: cc = 8, dh = 16: cc = 4, dh = 8: cc = 2 with the four
sign vectors as the book: a mismatch is 0 or negative there).

Layer-1 blocks (dq or dk <= 4) cannot carry codes on the narrow side.  Few queries (keys are the points
(f, [t,] v)): the argmax design - f on the integer grid 1 .. 6 (0 and 7 behind the length), fc_k maps f to
the first column of every head slice, + for even heads and - for odd ones, gain 32 on both sides (one
grid step is 1024 / sqrt(d) >= 64 nats); the query's entry there is +-32, so a row is won by the live keys
of largest or smallest f, 1, 2 or 4 of them with different v.  Scores reach +-540 nats, so these cases
carry their own offset, of both signs.  Many queries (queries are the points): fc_q maps f to code a_j and
v to code b_j of equal multiplicity, the points are (1, 0), (0, 1), (1, 1): a row asks for a, b or both.

tiled_forward() is a plain online-softmax reference in float32 (128-key tiles, S split ranges merged by
(m, l, T), per-set length) with injectable faults; the host test shows that every fault is visible on
these inputs at 100 x the GPU bar."""
import math
import zlib
from dataclasses import dataclass, replace
from typing import Optional, Tuple

import numpy as np
import torch

FWD_BAR = 2.0 ** -16          # forward against the fp64 oracle, of max(1, max|ref|)
BWD_BAR = 1.5e-2              # gradients, of max(1, max|ref tensor|), plain max error
HOST_BAR = 2.0 ** -20         # emulation / fp32 oracle / tiled reference against the fp64 oracle


@dataclass(frozen=True)
class Case:
    family: str                   # BlockPath the GPU call must take
    kind: str                     # "mq" many queries, "fq" few shared queries, "sab" self-attention
    B: int
    N: int                        # points per set
    m: int                        # inducing points / seeds (sab: unused)
    d: int
    h: int
    din: int = 0                  # layer-1 width of the narrow side (0: d)
    lengths: Optional[Tuple[int, ...]] = None
    off: int = 0                  # sign of the offset variant
    S: int = 2                    # split ranges of the tiled reference
    train: bool = True

    @property
    def key(self):
        s = f"{self.family}-{self.kind}-B{self.B}-N{self.N}-m{self.m}-d{self.d}-h{self.h}"
        if self.din:
            s += f"-din{self.din}"
        if self.lengths is not None:
            s += "-len" + ".".join(str(x) for x in self.lengths)
        if self.off:
            s += "-off" + ("+" if self.off > 0 else "-")
        return s

    @property
    def layer1(self):
        return 0 < self.din <= 4

    @property
    def nkeys(self):
        return self.m if self.kind == "mq" else self.N


def _mq(fam, B, N, m, d, h, din=0, **kw):
    return Case(fam, "mq", B, N, m, d, h, din, **kw)


def _fq(fam, B, N, m, d, h, din=0, **kw):
    return Case(fam, "fq", B, N, m, d, h, din, **kw)


MQ_BASE = [
    _mq("Mab1_128", 2, 200, 16, 128, 4),
    _mq("Mab1_128", 2, 129, 16, 128, 4),
    _mq("Mab1_128", 1, 1, 16, 128, 4),
    _mq("Mab1_256", 2, 300, 32, 256, 8),
    _mq("Mab1_256", 1, 1, 32, 256, 8),
    _mq("Mab1_128", 2, 77, 16, 128, 4, din=2),
    _mq("Mab1_256", 2, 77, 32, 256, 8, din=3),
]
# (base case, lengths of its masked run)
FQ_BASE = [
    (_fq("Mab0_128", 3, 333, 16, 128, 4, S=2), (333, 129, 17)),
    (_fq("Mab0_128", 2, 517, 16, 128, 4, S=4), (517, 100)),
    (_fq("Mab0_128", 3, 333, 1, 128, 4), (129, 333, 17)),
    (_fq("Mab0_128", 2, 150, 2, 128, 4), (150, 129)),
    (_fq("Mab0_256", 3, 333, 32, 256, 8), (333, 129, 17)),
    (_fq("Mab0_256", 2, 517, 16, 256, 8, S=4), (100, 517)),
    (_fq("Mab0_256", 3, 333, 1, 256, 8), (17, 333, 129)),
    (_fq("Mab0_256", 2, 515, 2, 256, 8, S=4), (515, 129)),
    (_fq("Mab0_256", 2, 333, 8, 256, 8, din=2), (333, 17)),
    (_fq("Mab0_256", 3, 261, 16, 256, 8, din=3), (261, 129, 17)),
    (_fq("Mab0_128", 3, 77, 16, 128, 4, din=2), (77, 17, 1)),
]
SAB_CASES = [
    Case("ExactCore", "sab", 3, 150, 0, 128, 4, lengths=(150, 129, 17)),
    Case("ExactCore", "sab", 3, 130, 0, 64, 8, lengths=(130, 129, 17)),
    Case("ExactCore", "sab", 3, 130, 0, 64, 4, lengths=(17, 130, 129)),
]
SD64_CASES = [
    _fq("Sd64", 3, 300, 64, 64, 8, train=False),
    _fq("Sd64", 3, 300, 64, 64, 8, lengths=(300, 129, 17), train=False),
    _fq("Sd64", 3, 300, 64, 64, 8, off=1, train=False),
    _fq("Sd64", 3, 300, 64, 64, 8, lengths=(300, 129, 17), off=-1, train=False),
    _mq("Sd64", 2, 300, 64, 64, 8, train=False),
    _mq("Sd64", 2, 300, 64, 64, 8, off=1, train=False),
    _mq("Sd64", 2, 300, 64, 64, 8, off=-1, train=False),
]


def _variants():
    out = []
    for c in MQ_BASE:
        out.append(c)
        if not c.layer1:                  # (layer 1 carries no offset column: the module docstring)
            out += [replace(c, off=1), replace(c, off=-1)]
    for c, lens in FQ_BASE:
        out += [c, replace(c, lengths=lens)]
        if not c.layer1:
            out += [replace(c, off=1), replace(c, off=-1, lengths=lens)]
    return out + SAB_CASES + SD64_CASES


CASES = _variants()


# --------------------------------------------------------------------------------------------------------- #
def hadamard(n):
    H = np.array([[1.0]])
    while H.shape[0] < n:
        H = np.block([[H, H], [H, -H]])
    assert H.shape[0] == n, n
    return H


def codebook(cc):
    if cc == 2:
        return np.array([[1.0, 1.0], [1.0, -1.0], [-1.0, 1.0], [-1.0, -1.0]])
    return hadamard(cc)


def _rng(case, salt=0):
    return np.random.Generator(np.random.PCG64(zlib.crc32(case.key.encode()) + salt))


def pool_of(L, rng):
    """Planting order of the live indices: the edges first, then a seeded permutation of the rest."""
    first = [0, L - 1, 15, 16, 127, 128, (L - 1) // 128 * 128]
    first = [i for i in dict.fromkeys(first) if 0 <= i < L]
    rest = [int(i) for i in rng.permutation(L) if int(i) not in first]
    return first + rest


def mults_of(P, rot):
    return [(1, 2, 4)[(k + rot) % 3] for k in range(1, P + 1)]


def plant(L, N, P, rot, rng):
    """Key codes [N] of one (set, head): 0 = decoy, k = 1 .. P on mults_of(P, rot)[k - 1] live keys, every
    key behind L an asked code (index L: code 1, index N - 1: code 2 or, P = 1, code 1)."""
    mult = mults_of(P, rot)
    assert sum(mult) <= L, (L, mult)
    z = np.zeros(N, dtype=np.int64)
    pool = pool_of(L, rng)
    order = []
    for rnd in range(4):
        order += [k for k in range(1, P + 1) if mult[k - 1] > rnd]
    for k, i in zip(order, pool):
        z[i] = k
    for n in range(L, N):
        z[n] = 1 + (n - L) % P
    if L < N:
        z[N - 1] = min(2, P) if N - 1 > L else 1
    return z


def _geometry(case):
    """(code dims cc, book, gain, payload columns of a head slice as offsets, offset column or None, key-code
    column offset, P)."""
    dh = case.d // case.h
    if case.kind == "sab":
        cc = {32: 8, 16: 4, 8: 2}[dh]
        g, kcol, pay, offc = 16.0, cc, list(range(2 * cc, dh)), None
    else:
        cc = dh // 2
        g, kcol, pay, offc = {64: 16.0, 128: 8.0, 256: 8.0}[case.d], 0, list(range(cc + 1, dh)), cc
    book = codebook(cc)
    P = min(6, len(book) - 2)
    gram = book @ book.T
    gap = min(gram[k, k] - max(gram[k, j] for j in range(len(book)) if j != k) for k in range(1, P + 1))
    gq = query_gain(case)
    assert gq * g * gap / math.sqrt(case.d) >= 64.0, (case.key, gq * g * gap / math.sqrt(case.d))
    return cc, book, g, gq, pay, offc, kcol, P


def query_gain(case):
    """g_q.  A power of two where the scores are products of the bf16 operands Qp and Kp; in the
    few-queries d >= 128 kernels the operand is sl2e g_q itself, rounded to bf16: a common factor in the
    forward, but the backward's dK = dS G' carries its error (3.2e-3 at g_q = 8, d = 128) against the
    oracle.  7.75 (d = 128) and 8.1875 (d = 256) are the bf16 values near 8 whose sl2e multiple rounds by
    less than 4e-5; every entry of a query's code and offset columns is a power of two times g_q, so the
    factor stays common."""
    if case.kind == "sab" or case.d == 64:
        return 16.0
    return {128: 7.75, 256: 8.1875}[case.d]


def offset_values(case):
    """(a, b): the offset column of every query and (times case.off) of every key; a b / sqrt(d) >= 96."""
    a = (4.0 if case.d >= 128 else 2.0) * query_gain(case)
    return a, 4.0 * math.ceil(96.0 * math.sqrt(case.d) / a / 4.0)


def offset_nats(case):
    a, b = offset_values(case)
    return case.off * a * b / math.sqrt(case.d)


def _fc_o(d):
    P = np.roll(np.eye(d), 3, axis=0) * np.where(np.arange(d) % 2, 1.0, -1.0)[None, :]
    return torch.tensor(P), torch.full((d,), 0.125, dtype=torch.float64)


def _lens(case):
    return list(case.lengths) if case.lengths is not None else [case.nkeys] * case.B


def _build_code(case):
    d, h, B = case.d, case.h, case.B
    dh = d // h
    cc, book, g, gq, pay, offc, kcol, P = _geometry(case)
    rng = _rng(case)
    nk = case.nkeys
    lens = _lens(case)
    zs = np.zeros((B, h, nk), dtype=np.int64)
    K = np.zeros((B, nk, d))
    for b in range(B):
        for j in range(h):
            rot = j if (case.kind == "mq" and case.layer1) else j + b
            zs[b, j] = plant(lens[b], nk, P, rot, rng)
            K[b, :, j * dh + kcol:j * dh + kcol + cc] = g * book[zs[b, j]]
            for c in pay:
                K[b, :, j * dh + c] = rng.integers(-8, 9, size=nk)
            for k in range(1, P + 1):                  # tie partners: one payload, but for its first column
                at = np.nonzero(zs[b, j, :lens[b]] == k)[0]
                K[b, at, j * dh + pay[0]:j * dh + pay[-1] + 1] = K[b, at[0], j * dh + pay[0]:j * dh + pay[-1] + 1]
                K[b, at, j * dh + pay[0]] = rng.integers(-8, 6) + np.arange(len(at))
            if offc is not None:
                K[b, :, j * dh + offc] = case.off * offset_values(case)[1]
    eye = np.eye(d)
    code_rows, pay_rows = np.zeros(d), np.zeros(d)
    for j in range(h):
        code_rows[j * dh:j * dh + cc] = 1
        if offc is not None:
            code_rows[j * dh + offc] = 1
        pay_rows[[j * dh + c for c in pay]] = 1
    p = {k + ".bias": torch.zeros(d, dtype=torch.float64) for k in ("fc_q", "fc_k", "fc_v")}
    p["fc_o.weight"], p["fc_o.bias"] = _fc_o(d)
    p["fc_v.weight"] = torch.tensor(eye * pay_rows[:, None])
    ws = np.zeros((B, h, 0), dtype=np.int64)
    if case.kind == "sab":
        # X slice: [query code | key code | payload]; fc_q / fc_k move their block into the first cc dims
        Wq, Wk = np.zeros((d, d)), np.zeros((d, d))
        for j in range(h):
            for c in range(cc):
                Wq[j * dh + c, j * dh + c] = 1
                Wk[j * dh + c, j * dh + cc + c] = 1
            for c in pay:
                Wq[j * dh + c, j * dh + c] = 1
        ws = rng.integers(1, P + 1, size=(B, h, nk))
        for b in range(B):
            for j in range(h):
                K[b, :, j * dh:j * dh + cc] = gq * book[ws[b, j]]
        p["fc_q.weight"], p["fc_k.weight"] = torch.tensor(Wq), torch.tensor(Wk)
        X = torch.tensor(K)
        return dict(Q=X, K=X, p=p, zs=zs, ws=ws)
    p["fc_k.weight"] = torch.tensor(eye * code_rows[:, None])
    if case.kind == "mq" and case.layer1:
        dq = case.din
        Wq = np.zeros((d, dq))
        for j in range(h):
            # codes a and a + 3 have equal multiplicities (mults_of repeats with 3): 1 on even heads, 2 on
            # odd ones, so the point (1, 1) meets a 2- or 4-way tie
            a = 1 + (j % 2 - j - 1) % 3
            assert mults_of(P, j)[a - 1] == mults_of(P, j)[a + 2] == 1 + j % 2
            Wq[j * dh:j * dh + cc, 0] = gq * book[a]
            Wq[j * dh:j * dh + cc, 1] = gq * book[a + 3]
            for c in pay:
                Wq[j * dh + c] = rng.integers(-2, 3, size=dq)
        pts = np.array([(1, 0), (0, 1), (1, 1)], dtype=np.float64)[np.arange(case.N) % 3]
        Q = np.zeros((B, case.N, dq))
        Q[:, :, :2] = pts
        if dq == 3:
            Q[:, :, 2] = rng.integers(-2, 3, size=(B, case.N))
        p["fc_q.weight"] = torch.tensor(Wq)
        return dict(Q=torch.tensor(Q), K=torch.tensor(K), p=p, zs=zs, ws=ws)
    p["fc_q.weight"] = torch.tensor(eye)
    nq, Bq = (case.m, 1) if case.kind == "fq" else (case.N, B)
    ws = rng.integers(1, P + 1, size=(Bq, h, nq))
    Q = np.zeros((Bq, nq, d))
    for b in range(Bq):
        for j in range(h):
            Q[b, :, j * dh:j * dh + cc] = gq * book[ws[b, j]]
            for c in pay:
                Q[b, :, j * dh + c] = rng.integers(-8, 9, size=nq)
            Q[b, :, j * dh + offc] = offset_values(case)[0]
    return dict(Q=torch.tensor(Q), K=torch.tensor(K), p=p, zs=zs, ws=ws)


def _build_argmax(case):
    """Few shared queries against layer-1 points (f, [t,] v): see the module docstring."""
    d, h, B, N, dk = case.d, case.h, case.B, case.N, case.din
    dh = d // h
    cc = dh // 2
    rng = _rng(case)
    lens = _lens(case)
    X = np.zeros((B, N, dk))
    for b in range(B):
        L = lens[b]
        f = rng.integers(2, 6, size=N).astype(np.float64)
        pool = pool_of(L, rng)
        if L >= 8:
            nmax, nmin = (1, 2, 4)[b % 3], (1, 2, 4)[(b + 1) % 3]
            sel = pool[:nmax + nmin] if b % 2 == 0 else pool[:nmax + nmin][::-1]
            f[sel[:nmax]] = 6
            f[sel[nmax:]] = 1
        elif L >= 2:
            f[pool[0]], f[pool[1]] = 6, 1
        f[L:] = np.where(np.arange(N - L) % 2 == 0, 7.0, 0.0)
        if L < N - 1:
            f[N - 1] = 0.0
        X[b, :, 0] = f
        X[b, :, -1] = rng.integers(-8, 9, size=N)
        if dk == 3:
            X[b, :, 1] = rng.integers(-2, 3, size=N)
    Wk, Wv = np.zeros((d, dk)), np.zeros((d, dk))
    for j in range(h):
        Wk[j * dh, 0] = 32.0 if j % 2 == 0 else -32.0
        for c in range(cc, dh):
            Wv[j * dh + c, -1] = rng.integers(-2, 3)
            if dk == 3:
                Wv[j * dh + c, 1] = rng.integers(-1, 2)
    Q = np.zeros((1, case.m, d))
    for j in range(h):
        Q[0, :, j * dh] = 32.0 * rng.choice([-1.0, 1.0], size=case.m)
        for c in range(cc, dh):
            Q[0, :, j * dh + c] = rng.integers(-8, 9, size=case.m)
    p = {k + ".bias": torch.zeros(d, dtype=torch.float64) for k in ("fc_q", "fc_k", "fc_v")}
    p["fc_o.weight"], p["fc_o.bias"] = _fc_o(d)
    p["fc_q.weight"] = torch.tensor(np.eye(d))
    p["fc_k.weight"], p["fc_v.weight"] = torch.tensor(Wk), torch.tensor(Wv)
    return dict(Q=torch.tensor(Q), K=torch.tensor(X), p=p, zs=None, ws=None)


_built = {}


def build(case):
    """{"Q", "K", "p" (float64; sab: Q is K), "G" (the cotangent of Y, integers in [-4, 4], zero on rows
    behind a set's length), "lengths" (list or None), "zs" / "ws" (key / query codes or None)}.  Cached:
    callers must not write into it."""
    if case.key not in _built:
        c = _build_argmax(case) if (case.kind == "fq" and case.layer1) else _build_code(case)
        nq = case.m if case.kind == "fq" else case.N
        G = torch.tensor(_rng(case, 1).integers(-4, 5, size=(case.B, nq, case.d)).astype(np.float64))
        if case.kind == "sab" and case.lengths is not None:
            for b, L in enumerate(case.lengths):
                G[b, L:] = 0
        c["G"] = G
        c["lengths"] = None if case.lengths is None else list(case.lengths)
        _built[case.key] = c
    return _built[case.key]


def f32(p):
    return {k: v.float() for k, v in p.items()}


# --------------------------------------------------------------------------------------------------------- #
# the fp64 oracle on the truncated sets, forward and gradients                                               #
# --------------------------------------------------------------------------------------------------------- #
def per_set_forward(fn, case, Q, K, p, lengths=None):
    """fn(Q_b, K_b, p) on every set cut to its length, padded back with zeros (sab: the padded rows of Y)."""
    lens = lengths if lengths is not None else [K.shape[1]] * case.B
    outs = []
    for b, L in enumerate(lens):
        Kb = K[b:b + 1, :L]
        if case.kind == "sab":
            y = fn(Kb, Kb, p)
            y = torch.cat([y, y.new_zeros(1, K.shape[1] - L, y.shape[-1])], 1)
        else:
            y = fn(Q if Q.shape[0] == 1 else Q[b:b + 1], Kb, p)
        outs.append(y)
    return torch.cat(outs, 0)


def oracle_forward(case, dtype=torch.float64, saved=False):
    from oracle import st_oracle as orc
    c = build(case)
    p = {k: v.to(dtype) for k, v in c["p"].items()}
    if saved:
        lens = _lens(case)
        out = []
        for b, L in enumerate(lens):
            Kb = c["K"][b:b + 1, :L].to(dtype)
            Qb = Kb if case.kind == "sab" else (c["Q"] if c["Q"].shape[0] == 1 else c["Q"][b:b + 1]).to(dtype)
            out.append(orc.mab_forward(Qb, Kb, p, case.h, return_saved=True))
        return out
    return per_set_forward(lambda q, k, pp: orc.mab_forward(q, k, pp, case.h), case, c["Q"].to(dtype),
                           c["K"].to(dtype), p, c["lengths"])


def grads_of(fn, case, dtype=torch.float64):
    """Gradients of sum(Y * G) through per_set_forward(fn): {"Y", parameters, "dQ", "dK"} (sab: "dX")."""
    c = build(case)
    leaves = {k: v.to(dtype).clone().requires_grad_(True) for k, v in c["p"].items()}
    K = c["K"].to(dtype).clone().requires_grad_(True)
    Q = K if case.kind == "sab" else c["Q"].to(dtype).clone().requires_grad_(True)
    Y = per_set_forward(fn, case, Q, K, leaves, c["lengths"])
    (Y * c["G"].to(dtype)).sum().backward()
    g = {k: (v.grad if v.grad is not None else torch.zeros_like(v)).detach() for k, v in leaves.items()}
    g["Y"] = Y.detach()
    if case.kind == "sab":
        g["dX"] = K.grad
    else:
        g["dQ"], g["dK"] = Q.grad, K.grad
    return g


_oracle_grads = {}


def oracle_grads(case):
    from oracle import st_oracle as orc
    if case.key not in _oracle_grads:
        _oracle_grads[case.key] = grads_of(lambda q, k, p: orc.mab_forward(q, k, p, case.h), case)
    return _oracle_grads[case.key]


def has_structure(case):
    """What the planting of a code-design case really contains: {"tie_across_tiles", "tie_across_ranges",
    "sole_at_0", "sole_in_last_tile", "masked_winner_at_L", "masked_winner_at_end"}."""
    c = build(case)
    zs, lens = c["zs"], _lens(case)
    nk = case.nkeys
    ntile = -(-nk // 128)
    per = -(-ntile // case.S) * 128                        # keys per split range of the tiled reference
    out = dict.fromkeys(("tie_across_tiles", "tie_across_ranges", "sole_at_0", "sole_in_last_tile",
                         "masked_winner_at_L", "masked_winner_at_end"), False)
    for b in range(case.B):
        L = lens[b]
        for j in range(case.h):
            z = zs[b, j]
            for k in range(1, int(z.max()) + 1):
                at = np.nonzero(z[:L] == k)[0]
                if len(at) >= 2:
                    out["tie_across_tiles"] |= len(set(at // 128)) > 1
                    out["tie_across_ranges"] |= len(set(at // per)) > 1
                if len(at) == 1:
                    out["sole_at_0"] |= at[0] == 0
                    out["sole_in_last_tile"] |= L > 128 and at[0] // 128 == (L - 1) // 128
            if L < nk:
                out["masked_winner_at_L"] |= z[L] > 0
                out["masked_winner_at_end"] |= z[nk - 1] > 0
    return {k: bool(v) for k, v in out.items()}


# --------------------------------------------------------------------------------------------------------- #
# the tiled online-softmax reference with injectable faults                                                  #
# --------------------------------------------------------------------------------------------------------- #
FAULTS = ("no_max", "no_rescale", "merge_last_max", "empty_not_skipped", "mask_L_plus_1", "mask_per_tile",
          "heads_swapped")


def tiled_forward(case, fault=None, tile=None, S=None):
    """The block on build(case) as a fused kernel runs its attention, in float32: per (set, head) the keys
    in tiles of `tile`, cut into S ranges of whole tiles; inside a range the running (m, l, T) with the
    rescale alpha = exp2(m_old - m_new), the ranges merged by their maxima; keys at and behind the set's
    length masked to -inf, ranges that start behind the length skipped (their partial is (-inf, 0, 0)).
    `fault` breaks one of these on purpose.  Many-queries cases have 16 / 32 / 64 keys: they take tiles of
    4 so that there is something to rescale and to merge.  Returns Y float32 [B, nq, d] (sab: rows behind
    the length zero)."""
    assert fault is None or fault in FAULTS, fault
    c = build(case)
    d, h = case.d, case.h
    dh = d // h
    f = np.float32
    tile = tile or (4 if case.kind == "mq" else 128)
    S = S or case.S
    p = {k: v.numpy().astype(f) for k, v in c["p"].items()}
    K = c["K"].numpy().astype(f)
    Q = c["Q"].numpy().astype(f)
    lens = _lens(case)
    sl2e = f(math.log2(math.e) / math.sqrt(d))
    nk = K.shape[1]
    ntile = -(-nk // tile)
    per = -(-ntile // S) * tile
    Y = []
    with np.errstate(all="ignore"):
        for b in range(case.B):
            L = lens[b]
            Qb = K[b] if case.kind == "sab" else Q[0 if Q.shape[0] == 1 else b]
            Qp = Qb @ p["fc_q.weight"].T + p["fc_q.bias"]
            Kp = K[b] @ p["fc_k.weight"].T + p["fc_k.bias"]
            Vp = K[b] @ p["fc_v.weight"].T + p["fc_v.bias"]
            O = np.zeros_like(Qp)
            for j in range(h):
                jk = {0: 1, 1: 0}.get(j, j) if fault == "heads_swapped" else j
                s = (Qp[:, j * dh:(j + 1) * dh] @ Kp[:, jk * dh:(jk + 1) * dh].T) * sl2e
                V = Vp[:, j * dh:(j + 1) * dh]
                parts = []
                for lo in range(0, nk, per):
                    hi = min(nk, lo + per)
                    m = np.full(s.shape[0], -np.inf, dtype=f)
                    l = np.zeros(s.shape[0], dtype=f)
                    T = np.zeros((s.shape[0], dh), dtype=f)
                    if lo >= L and fault != "empty_not_skipped":
                        parts.append((m, l, T))
                        continue
                    for t0 in range(lo, hi, tile):
                        cols = np.arange(t0, min(t0 + tile, hi))
                        if fault == "mask_L_plus_1":
                            live = cols < L + 1
                        elif fault == "mask_per_tile":
                            live = np.full(len(cols), t0 < L)
                        else:
                            live = cols < L
                        st = np.where(live[None, :], s[:, cols], f(-np.inf))
                        mnew = np.zeros_like(m) if fault == "no_max" else np.maximum(m, st.max(1))
                        alpha = np.ones_like(m) if fault == "no_rescale" else np.exp2(m - mnew)
                        pt = np.exp2(st - mnew[:, None])
                        l = l * alpha + pt.sum(1, dtype=f)
                        T = T * alpha[:, None] + pt @ V[cols]
                        m = mnew
                    parts.append((m, l, T))
                M = parts[-1][0] if fault == "merge_last_max" else np.max([q[0] for q in parts], 0)
                lsum = np.zeros_like(M)
                Tsum = np.zeros((s.shape[0], dh), dtype=f)
                for m, l, T in parts:
                    skip = np.isneginf(m) & (l == 0) if fault != "empty_not_skipped" else np.zeros_like(l, bool)
                    w = np.where(skip, f(0), np.exp2(m - M))
                    lsum = lsum + w * l
                    Tsum = Tsum + w[:, None] * T
                O[:, j * dh:(j + 1) * dh] = Qp[:, j * dh:(j + 1) * dh] + Tsum / lsum[:, None]
            Z = O @ p["fc_o.weight"].T + p["fc_o.bias"]
            y = O + np.maximum(Z, 0)
            if case.kind == "sab":
                y[L:] = 0
            Y.append(y)
    return np.stack(Y)
