"""The d = 128 backward tail's plan, seen from the host (csrc/tail_plan.hip: tail_form_from_env, plan_tail;
pca_debug_tail_plan builds a BwdDefer of made-up addresses and returns the plan as integers - no device).

The job tables are the ones a training step queues (B sets of N points, m = 16 inducing points, 2 or 3 input
columns): bf16 list = layer 2's fc_o and fc_q jobs and layer 1's fc_o job, B N rows each; fp32 list = the PMA's
jobs (B rows) and the two layers' [B 16]-row jobs; the layer-1 fc_v job, B 16 rows; three post jobs; the three
dG sums due before them; layer 1's two fc_q sums pending."""
import ctypes
import itertools

import pytest

import pca_hip
from pca_hip import _lib

SLABS, FOLD, RIDE, POST_FUSE, MID_WIDE, MID_SMALL, DZ_MASK = (1 << i for i in range(7))
NOWHERE, WGRAD_ROWS, TERMINAL_ROWS, TERMINAL_ROWS_POST2_SUMS = range(4)
STEP, WG_BF16, WG_F32, WG256, SUMS_DUE, TERMINAL1, POST1, POST2, SUMS_LATE2 = range(9)
CAP = 80 << 20                      # the room the engine lends (st_engine.hip: carve)
FULL = (128 * 128 + 128) * 4        # bytes of a [128 x 128] slab with its bias row
CASES = [(3, 256, 2), (5, 512, 3), (3, 300, 2), (1, 1024, 3), (9, 128, 2), (13, 2048, 3), (128, 512, 3)]


def consistent_forms():
    """Every TailForm tail_form_from_env can return: the ride only with slabs, the fold and the small mid chain."""
    for bits in range(128):
        if bits & RIDE and not (bits & SLABS and bits & FOLD and bits & MID_SMALL):
            continue
        yield bits


def heads(M):
    return [(M, 1 if j == 0 else 0, 32 * j, 32 * j + 32) for j in range(4)]


def step_tables(B, N, dq, phase=-1):
    """(bf16 jobs, fp32 jobs, fc_v job, post jobs, due sums, pending late sums, classes) of a step, or of one
    phase of a split step (0: head, PMA and layer 2; 1: layer 1)."""
    bf16, f32, fcv, posts, sums, late, C = [], [], None, [], [], [], 0
    if phase != 1:
        f32 += [(B, 1, 0, 128)] + heads(B)                                   # PMA
        posts.append((1, 128, 128, 1))
        sums.append(4 * 1 * 128)
        bf16 += [(B * N, 1, 0, 128), (B * N, 1, 0, 128)]                      # layer 2: fc_o, fc_q
        f32 += [(B * 16, 1, 0, 128)] * 3 + heads(B * 16)
        posts.append((16, 128, 128, 1))
        sums.append(64 * 128)
        C = 35
    if phase != 0:
        bf16.append((B * N, 1, 0, 128))                                       # layer 1: fc_o
        late += [128 * dq, 128]                                               # its fc_q partials
        f32 += [(B * 16, 1, 0, 128)] * 3
        fcv = (B * 16, dq)
        posts.append((16, 128, dq, 1))
        sums.append(64 * dq)
    return bf16, f32, fcv, posts, sums, late, C


def plan(form, tables, cap=CAP, rode=False):
    bf16, f32, fcv, posts, sums, late, C = tables
    words = [form, cap, int(rode), len(bf16), len(f32), int(fcv is not None), fcv[0] if fcv else 0,
             fcv[1] if fcv else 0, len(posts), len(sums), len(late), C]
    for row in bf16 + f32 + posts:
        words += list(row)
    words += sums + late
    arr = (ctypes.c_int64 * len(words))(*words)
    out = (ctypes.c_int64 * 1024)()
    rc = pca_hip.lib().pca_debug_tail_plan(arr, len(words), out, 1024)
    if rc != 0:
        return rc
    o = list(out)
    p = dict(zip(("form", "rpw_bf16", "rpw_f32", "fcv", "post_fused", "nseq", "nslab", "nlate", "nlate2",
                  "nriders", "used"), o[:11]))
    at = 11

    def take(n, width):
        nonlocal at
        rows = [tuple(o[at + width * i: at + width * (i + 1)]) for i in range(n)]
        at += n * width
        return rows
    p["seq"] = take(p["nseq"], 3)
    p["slabs"] = take(p["nslab"], 4)            # (list, job, offset, bytes)
    p["late"] = take(p["nlate"], 4)             # (slab offset or -1 - pending index, output buffer, width, slabs)
    p["late2"] = take(p["nlate2"], 4)
    p["riders"] = [r[0] for r in take(p["nriders"], 1)]
    return p


def cdiv(a, b):
    return -(-a // b)


def list_bytes(jobs, rpw):
    return sum(cdiv(M, rpw) * ((hi - lo) * 128 + 128 * db) * 4 for M, db, lo, hi in jobs)


def expected_rows(tables, cap):
    """The rule as the issue states it: bf16 512 up to 98304 rows, then steps of 512 capped at 1024, doubled until
    the list fits three quarters of the room; fp32 128, doubled until it fits behind the bf16 list."""
    bf16, f32 = tables[0], tables[1]
    rows = sum(j[0] for j in bf16)
    rb = min(1024, max(512, 512 * ((rows + 98303) // 98304)))
    while list_bytes(bf16, rb) > cap * 3 // 4:
        rb *= 2
    used = (list_bytes(bf16, rb) + 255) & ~255 if bf16 else 0
    rf = 128
    while used + list_bytes(f32, rf) > cap:
        rf *= 2
    return rb, rf


def names(p):
    return [s[0] for s in p["seq"]]


def check_slabs(p, tables, cap):
    spans = sorted((off, off + n) for _, _, off, n in p["slabs"])
    for (a0, a1), (b0, b1) in zip(spans, spans[1:]):
        assert a1 <= b0, ("slabs overlap", spans)
    for lst, _, off, n in p["slabs"]:
        assert off % 256 == 0 and off >= 0 and off + n <= cap, (lst, off, n, cap)
        if lst == 0:
            assert off + n <= cap * 3 // 4
    assert p["used"] % 256 == 0 and p["used"] <= cap + 255
    # fixed order: bf16 list, fp32 list, fc_v job
    order = [lst for _, lst in sorted((off, lst) for lst, _, off, _ in p["slabs"])]
    assert order == sorted(order), order


def check_sums(p, tables, slab_mode):
    """Each placed job's sums once, in job order (a bf16 list's first), then the pending ones in their order."""
    bf16, f32, fcv, _, _, late, _ = tables
    assert p["nlate"] <= 40
    outs = [b for _, b, _, _ in p["late"]] + [b for _, b, _, _ in p["late2"]]
    assert len(outs) == len(set(outs)), outs
    want = []
    if slab_mode:
        for lst, jobs in ((0, bf16), (1, f32)):
            for i, (M, db, lo, hi) in enumerate(jobs):
                want += [2 * (16 * lst + i)] + ([2 * (16 * lst + i) + 1] if db else [])
    got = [b for b in outs if b < 64]
    assert got == want, (got, want)
    assert [b for b in outs if b >= 100] == [100 + i for i in range(len(late))]
    assert [s for s, _, _, _ in p["late"] if s < 0] == [-1 - i for i in range(len(late))]
    by_slab = {off: (lst, job) for lst, job, off, _ in p["slabs"]}
    for src, b, width, S in p["late"] + p["late2"]:
        if src >= 0 and b % 2 == 0:                      # a weight sum starts at its job's slab
            assert src in by_slab, (src, b)
    return outs


@pytest.mark.parametrize("case", CASES, ids=lambda c: "B%d-N%d-dq%d" % c)
def test_every_form(case):
    B, N, dq = case
    tables = step_tables(B, N, dq)
    ref = {}
    for form in consistent_forms():
        for rode in ([False, True] if form & RIDE else [False]):
            p = plan(form, tables, rode=rode)
            assert isinstance(p, dict), (form, rode, pca_hip.lib().pca_last_error())
            assert p["form"] == form
            slab_mode = bool(form & SLABS)
            check_slabs(p, tables, CAP)
            outs = check_sums(p, tables, slab_mode)
            if slab_mode:
                assert (p["rpw_bf16"], p["rpw_f32"]) == expected_rows(tables, CAP)
                assert len([s for s in p["slabs"] if s[0] < 2]) == len(tables[0]) + len(tables[1])
            else:
                assert p["slabs"] == [] and p["fcv"] == TERMINAL_ROWS and p["used"] == 0
            # where the fc_v job runs, and the launches DESIGN 6.1 names
            fused = bool(form & POST_FUSE)
            if slab_mode:
                assert p["fcv"] == (WGRAD_ROWS if fused else TERMINAL_ROWS_POST2_SUMS)
                assert (64 in outs and 65 in outs)
                assert p["nlate2"] == (0 if fused else 2)
            assert p["post_fused"] == fused
            wgrad = [STEP] if form & FOLD else [WG_BF16, WG_F32]
            assert names(p) == wgrad + [TERMINAL1] + ([] if fused else [POST2]), (form, names(p))
            # a launch per list: the fc_v sums precede the fp32 list's; one launch: they follow them
            if slab_mode and fused:
                first_f32 = outs.index(32)
                assert (outs.index(64) < first_f32) == (not form & FOLD)
            # the due sums ride in the first weight-gradient launch: whole, or (no bf16 rows beside them) cut
            # into ranges as wide as the fp32 rows
            sums = tables[4]
            if rode:
                width = 256 * cdiv(B * 16, p["rpw_f32"])
                want = [min(width, n - c) for n in sums for c in range(0, n, width)]
                assert p["riders"] == want
            else:
                assert p["riders"] == sums
            # the ride changes no placement: same rows, same slabs, same sums as the step planned without it
            key = form & ~RIDE
            if not form & RIDE:
                ref[key] = p
            elif key in ref:
                q = ref[key]
                for k in ("rpw_bf16", "rpw_f32", "slabs", "late", "late2", "fcv", "used"):
                    assert p[k] == q[k], (k, form, rode)
                if not rode:
                    assert p["seq"] == q["seq"]


def test_default_step_grids():
    """The default form of the (5, 512, 3) step, by hand: 3 x 2560 rows at 512 per workgroup, 80 fp32 rows."""
    tables = step_tables(5, 512, 3)
    form = SLABS | FOLD | RIDE | POST_FUSE | MID_WIDE | MID_SMALL | DZ_MASK
    whole = plan(form & ~RIDE, tables)
    # rows: 3 bf16 + 15 fp32 + 1 of the fc_v job (2 workgroups of 2 x 64 rows in a grid 32 wide) + 3 due sums
    assert whole["seq"][0] == (STEP, 32, 3 + 15 + 1 + 3)           # 8192-wide dG sum: 32 x 256 threads
    rode = plan(form, tables, rode=True)
    # no bf16 rows: the grid is as wide as the fp32 rows (1), the sums are cut into 256-wide ranges
    assert rode["seq"][0] == (STEP, 1, 15 + 1 + (2 + 32 + 1))
    # k_terminal1: 3 fused rows + 3 dWk rows + classifier + 34 sums (6 + 24 + 2 + 2); dWk of d x dk = 128 x 128
    # needs 64 workgroups
    assert whole["seq"][1] == rode["seq"][1] == (TERMINAL1, 64, 3 + 3 + 1 + 34)
    assert [s[:3] for s in whole["slabs"][:3]] == [(0, 0, 0), (0, 1, 5 * FULL), (0, 2, 10 * FULL)]


def test_rows_double_when_the_room_is_short():
    tables = step_tables(5, 512, 3)
    cap = 1200 * 1024                   # 3 x 5 full slabs (990720 bytes) pass three quarters of it, 3 x 3 fit
    form = SLABS | FOLD | POST_FUSE | MID_WIDE | MID_SMALL
    p = plan(form, tables, cap=cap)
    assert (p["rpw_bf16"], p["rpw_f32"]) == expected_rows(tables, cap) == (1024, 128)
    check_slabs(p, tables, cap)
    check_sums(p, tables, True)
    assert p["fcv"] == WGRAD_ROWS
    # the workload-sized step in 12 MiB: both lists' rows double
    big = step_tables(128, 512, 3)
    cap = 12 << 20
    p = plan(form, big, cap=cap)
    assert (p["rpw_bf16"], p["rpw_f32"]) == expected_rows(big, cap)
    assert p["rpw_bf16"] > 1024 and p["rpw_f32"] > 128
    check_slabs(p, big, cap)
    check_sums(p, big, True)
    # no room for even one slab per job: refused, not looped over
    assert plan(form, tables, cap=64 * 1024) == -1


def test_no_room_for_the_fc_v_slab():
    """The lists fit, the fc_v job's partials do not: it stays in k_terminal1 and adds atomically."""
    tables = step_tables(5, 512, 3)
    form = SLABS | FOLD | POST_FUSE | MID_WIDE | MID_SMALL
    full = plan(form, tables)
    lists = max(off + n for lst, _, off, n in full["slabs"] if lst < 2)
    p = plan(form, tables, cap=lists + 1024)
    assert p["fcv"] == TERMINAL_ROWS and p["post_fused"] == 1 and names(p) == [STEP, TERMINAL1]
    assert not [s for s in p["slabs"] if s[0] == 2]


@pytest.mark.parametrize("phase", [0, 1])
def test_split_step(phase):
    tables = step_tables(3, 256, 2, phase)
    for form in consistent_forms():
        rode = bool(form & RIDE) and phase == 1
        p = plan(form, tables, rode=rode)
        assert isinstance(p, dict), form
        check_slabs(p, tables, CAP)
        check_sums(p, tables, bool(form & SLABS))
        fused = bool(form & POST_FUSE)
        assert names(p) == ([STEP] if form & FOLD else [WG_BF16, WG_F32]) + [TERMINAL1] + ([] if fused else [POST2])
        assert p["fcv"] == (NOWHERE if phase == 0 else
                            TERMINAL_ROWS if not form & SLABS else WGRAD_ROWS if fused else TERMINAL_ROWS_POST2_SUMS)


def test_sum_table_overflow_is_refused():
    """6 + 24 + 2 sums of the step's own: 8 pending ones fill the 40 entries; with a 9th the fc_v job stays in
    k_terminal1 and leaves its two sums to k_mab0_post2; an 11th is refused."""
    bf16, f32, fcv, posts, sums, late, C = step_tables(3, 256, 2)
    form = SLABS | FOLD | POST_FUSE | MID_WIDE | MID_SMALL
    p = plan(form, (bf16, f32, fcv, posts, sums, [128] * 8, C))
    assert p["nlate"] == 40 and p["fcv"] == WGRAD_ROWS and names(p) == [STEP, TERMINAL1]
    p = plan(form, (bf16, f32, fcv, posts, sums, [128] * 9, C))
    assert p["nlate"] == 39 and p["fcv"] == TERMINAL_ROWS_POST2_SUMS and names(p) == [STEP, TERMINAL1, POST2]
    p = plan(form, (bf16, f32, fcv, posts, sums, [128] * 10, C))
    assert p["nlate"] == 40 and p["fcv"] == TERMINAL_ROWS_POST2_SUMS
    assert plan(form, (bf16, f32, fcv, posts, sums, [128] * 11, C)) == -1
    assert b"table full" in pca_hip.lib().pca_last_error()


def test_nothing_but_post_jobs():
    """No rider at all: the two post launches of a stand-alone block."""
    p = plan(SLABS | FOLD | POST_FUSE, ([], [], None, [(16, 128, 128, 1)], [], [], 0))
    assert p["seq"] == [(POST1, cdiv(128 * 128 + 16 * 128, 256), 1), (POST2, cdiv(128 * 128 + 128 + 16 * 128, 256), 1)]
    p = plan(SLABS | FOLD | POST_FUSE, ([], [], None, [(16, 128, 128, 1)], [512], [], 0))
    assert names(p) == [SUMS_DUE, POST1, POST2]


SPELLINGS = [None, "0", "1"]


@pytest.mark.parametrize("mid", [None, "0", "1", "wide", "small"])
def test_form_from_env(monkeypatch, mid):
    tables = step_tables(3, 256, 2)
    for slabs, fold, ride, post, dzm in itertools.product(SPELLINGS, repeat=5):
        env = {"PCA_WGRAD_SLABS": slabs, "PCA_WGRAD_FOLD": fold, "PCA_WGRAD_RIDE": ride, "PCA_POST_FUSE": post,
               "PCA_D128_DZ_MASK": dzm, "PCA_D128_MIDFUSE": mid}
        for k, v in env.items():
            if v is None:
                monkeypatch.delenv(k, raising=False)
            else:
                monkeypatch.setenv(k, v)
        on = lambda v: v != "0"
        want = (SLABS * on(slabs) | FOLD * on(fold) | POST_FUSE * on(post) | DZ_MASK * on(dzm) |
                MID_WIDE * (mid in (None, "1", "wide")) | MID_SMALL * (mid in (None, "1", "small")))
        if on(ride) and on(slabs) and on(fold) and mid in (None, "1", "small"):
            want |= RIDE
        got = plan(-1, tables)["form"]
        assert got == want, (env, got, want)
        assert got in set(consistent_forms())


def test_debug_entry_is_bound_outside_the_abi():
    assert "pca_debug_tail_plan" in _lib.DEBUG_SIGNATURES and "pca_debug_tail_plan" not in _lib.SIGNATURES
    assert pca_hip.lib().pca_debug_tail_plan(None, 0, None, 0) == -1
