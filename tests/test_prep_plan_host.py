"""The preparation launch's plan, seen from the host (csrc/prep_plan.hpp: prep_plan; pca_debug_prep_plan builds the
job tables from integers and made-up addresses and returns the plan as integers - no device).

An ITEM is one workgroup of the launch.  What an item covers is restated here from the bodies of prep_plan.hpp:
* query segment of a job (m, d, h, WvT asked for, dk, G images asked for): item x is live row x (m rows; m h at
  d > 128), then the 16 spare transposers where WvT is asked for, then the pad items: 256 elements each of the padding
  rows [h m, Rp) x dk of the bf16 G images, Rp = h m rounded up to 32;
* pack segment: item x is block x of the B bx blocks of pack_body;
* tile segment of a group: item t is source rows [32 t, 32 t + 32) x all columns, written to every target of the
  group (modes 0 / 1: dst rows 32 t .. 32 t + 31; modes 2 / 3: positions 32 t .. 32 t + 31 of each dst row);
* element segment of a job: item x is dst[1024 x .. 1024 x + 1023];
* clear segment of a job: item x is the 256 16-byte groups 256 x .. of the destination, word w lying in group
  (w + lead) // 8 where lead = (address of dst mod 16) / 2."""
import ctypes

import numpy as np
import pytest

import pca_hip
from pca_hip import _lib

QUERY, PACK, TILES, ELEMS, CLEAR = range(5)
SPARE = 16


def plan(query=(), jobs=(), pack=(0, 0, 0)):
    """query: (m, d, h, spare, dk, G images); jobs: (source id, source misalignment, dst misalignment, rows, cols, mode);
    pack: (kind, B, bx).  -> dict or the error code."""
    words = [len(query), len(jobs), *pack]
    for row in list(query) + list(jobs):
        words += list(row)
    arr = (ctypes.c_int64 * len(words))(*words)
    out = (ctypes.c_int64 * 512)()
    rc = pca_hip.lib().pca_debug_prep_plan(arr, len(words), out, 512)
    if rc != 0:
        return rc
    o = list(out)
    blocks, nseg, ngrp, lds = o[:4]
    segs = [tuple(o[4 + 3 * i: 7 + 3 * i]) for i in range(nseg)]
    at = 4 + 3 * nseg
    groups = [tuple(j for j in o[at + 4 * g + 1: at + 4 * g + 4][:o[at + 4 * g]]) for g in range(ngrp)]
    return {"blocks": blocks, "segs": segs, "groups": groups, "lds": lds}


def check(query, jobs, pack, p):
    """The assertions every plan must meet; returns the blocks per kind."""
    segs, groups = p["segs"], p["groups"]
    firsts = [s[2] for s in segs] + [p["blocks"]]
    assert firsts[0] == 0 and all(a < b for a, b in zip(firsts, firsts[1:])), firsts    # no empty segment
    order = [s[0] for s in segs]
    rank = {QUERY: 0, PACK: 1, TILES: 2, ELEMS: 2, CLEAR: 2}
    assert [rank[k] for k in order] == sorted(rank[k] for k in order), order
    assert [k for k in order if k != QUERY and k != PACK] == sorted(k for k in order if k not in (QUERY, PACK)), order
    cover = [np.zeros(max(r * c, 0), np.int32) for (_, _, _, r, c, _) in jobs]
    qseen = [0] * len(query)
    per_kind = [0] * 5
    packed = 0
    for (kind, job, first), end in zip(segs, firsts[1:]):
        n = end - first
        per_kind[kind] += n
        if kind == QUERY:
            m, d, h, spare, dk, images = query[job]
            pad = (-(-h * m // 32) * 32 - h * m) * dk if images else 0       # elements of the padding rows
            assert n == (m * h if d > 128 else m) + (SPARE if spare else 0) + -(-pad // 256)
            qseen[job] += 1
        elif kind == PACK:
            packed += n
        elif kind == TILES:
            g = groups[job]
            _, _, _, rows, cols, _ = jobs[g[0]]
            assert n == rows // 32
            for t in range(n):
                for j in g:
                    mode = jobs[j][5]
                    c = cover[j].reshape(rows, cols) if mode <= 1 else cover[j].reshape(cols, rows)
                    before = int(cover[j].sum())
                    if mode <= 1:
                        c[32 * t:32 * t + 32, :] += 1
                    else:
                        c[:, 32 * t:32 * t + 32] += 1
                    assert int(cover[j].sum()) > before
        elif kind == ELEMS:
            for x in range(n):
                assert 1024 * x < cover[job].size                             # the item is not empty
                cover[job][1024 * x:1024 * x + 1024] += 1
        else:
            lead = jobs[job][2] // 2
            size = cover[job].size
            for x in range(n):
                lo, hi = max(0, 2048 * x - lead), min(size, 2048 * (x + 1) - lead)
                assert lo < hi
                cover[job][lo:hi] += 1
    for i, c in enumerate(cover):
        assert (c == 1).all(), (i, jobs[i], np.unique(c))
    assert qseen == [1] * len(query)
    kind, B, bx = pack
    assert packed == (B * bx if kind else 0)
    assert p["blocks"] == sum(per_kind)
    assert p["lds"] == max([q[1] for q in query], default=0)
    # a source shared by several jobs is one group (of up to three targets)
    for g in groups:
        assert len({(jobs[j][0], jobs[j][1], jobs[j][3], jobs[j][4]) for j in g}) == 1
    tiled = [j for g in groups for j in g]
    assert len(tiled) == len(set(tiled))
    by_src = {}
    for j in tiled:
        by_src.setdefault((jobs[j][0], jobs[j][1], jobs[j][3], jobs[j][4]), []).append(j)
    assert len(groups) == sum(-(-len(v) // 3) for v in by_src.values())
    return per_kind


def isab_jobs(li, dk, training, need_dx, d=128):
    """isab_collect_prep (csrc/isab_bf16.hip): sources wv0, wo0, wk1, wv1, wq1, wo1 of layer li."""
    wv0, wo0, wk1, wv1, wq1, wo1 = range(10 * li, 10 * li + 6)
    J = []
    if dk > 4:
        J.append((wv0, d, dk, 0))
    J += [(wo0, d, d, 0), (wk1, d, d, 0), (wv1, d, d, 0)]
    if dk > 4:
        J.append((wq1, d, d, 0))
    J.append((wo1, d, d, 1))
    if training:
        J += [(wk1, d, d, 3), (wv1, d, d, 3), (wo0, d, d, 2)]
        if dk > 4:
            J += [(wv0, d, dk, 2), (wv0, d, dk, 3)]
        J.append((wo1, d, d, 2))
        if need_dx:
            J.append((wq1, d, d, 2))
    return [(s, 0, 0, r, c, mode) for s, r, c, mode in J]


def step128(training, din=2, flag_words=1016):
    jobs = isab_jobs(0, din, training, False) + isab_jobs(1, 128, training, True)
    jobs.append((99, 0, 0, 1, flag_words, 4))
    query = [(16, 128, 4, 0, din, 0), (16, 128, 4, 0, 128, 1), (1, 128, 4, 1, 128, 1)]
    return query, jobs


def step256():
    """images256_prepare and mab0_d256_prep_collect (csrc/st_engine.hip): m = 32, h = 8."""
    J = []
    for li in range(2):
        wo, wq, wk, wv = range(10 * li, 10 * li + 4)
        J += [(wo, 1)] + ([(wq, 0)] if li else []) + [(wo, 2)] + ([(wq, 2)] if li else [])
        J += [(wk, 0), (wv, 0), (wk, 2), (wv, 2)]
    jobs = [(s, 0, 0, 256, 256, mode) for s, mode in J]
    return [(32, 256, 8, 0, 3, 0), (32, 256, 8, 0, 256, 1), (1, 256, 8, 0, 256, 1)], jobs


def test_cfg2_training_step():
    query, jobs = step128(True)
    pack = (2, 128, 2)
    p = plan(query, jobs, pack)
    per = check(query, jobs, pack, p)
    assert len(jobs) == 22 and len(p["groups"]) == 10
    # 40 image workgroups in place of 1344; the PMA's 28 padding rows of G are 14 pad items
    assert per == [16 + 16 + 1 + SPARE + 14, 256, 40, 0, 1]
    assert sorted(len(g) for g in p["groups"]) == [2] * 9 + [3]       # layer 2's fc_v feeds Wv0, Wv0TP and Wv0T
    assert p["blocks"] == 63 + 256 + 40 + 1 <= 512                    # one round of resident workgroups


def test_inference_makes_no_transposed_images():
    query, jobs = step128(False)
    p = plan(query, jobs)
    per = check(query, jobs, (0, 0, 0), p)
    assert all(j[5] in (0, 1, 4) for j in jobs) and len(jobs) == 4 + 6 + 1
    assert len(p["groups"]) == 10 and per[TILES] == 40 and per[PACK] == 0


@pytest.mark.parametrize("dk", [128, 2, 4])
def test_one_layer(dk):
    jobs = isab_jobs(0, dk, True, dk > 4)
    query = [(16, 128, 4, 1, dk, 1)]
    p = plan(query, jobs)
    per = check(query, jobs, (0, 0, 0), p)
    assert per[QUERY] == 32 and per[ELEMS] == 0 and per[TILES] == 4 * (6 if dk > 4 else 4)


def test_d256_step():
    query, jobs = step256()
    p = plan(query, jobs, (2, 64, 2))
    per = check(query, jobs, (2, 64, 2), p)
    assert per[QUERY] == 256 + 256 + 8 + 24 and per[TILES] == 8 * 7 and per[PACK] == 128
    assert p["lds"] == 256


@pytest.mark.parametrize("pack", [(0, 0, 0), (2, 5, 2), (3, 4, 5)])
def test_pack_items(pack):
    query, jobs = step128(True, din=3)
    p = plan(query, jobs, pack)
    check(query, jobs, pack, p)
    p = plan((), jobs, pack)
    check((), jobs, pack, p)


@pytest.mark.parametrize("mode", [0, 1, 2, 3])
def test_element_fallback(mode):
    jobs = [(0, 0, 0, 48, 40, mode), (1, 0, 0, 128, 3, mode), (2, 0, 0, 128, 128, mode),
            (3, 4, 0, 128, 128, mode), (4, 0, 2, 128, 128, mode), (5, 0, 0, 32, 40, mode), (6, 0, 0, 32, 264, mode)]
    p = plan((), jobs)
    per = check((), jobs, (0, 0, 0), p)
    tiled = {j for g in p["groups"] for j in g}
    # 32 x 40 fits a tile but for mode 1, whose K permutation needs whole 32-blocks of columns
    assert tiled == ({2, 5} if mode != 1 else {2})
    assert per[ELEMS] == 2 + 1 + 16 + 16 + (2 if mode == 1 else 0) + 9


@pytest.mark.parametrize("lead", [0, 2, 8, 14])
@pytest.mark.parametrize("words", [1, 7, 8, 4097])
def test_clears(words, lead):
    jobs = [(0, 0, lead, 1, words, 4), (1, 0, 0, 32, 32, 0)]
    p = plan((), jobs)
    per = check((), jobs, (0, 0, 0), p)
    assert per[CLEAR] == -(-(words + lead // 2) // 2048)
    assert p["segs"][-1][0] == CLEAR


def test_empty_jobs_make_no_items():
    jobs = [(0, 0, 0, 0, 128, 0), (1, 0, 0, 1, 0, 4), (2, 0, 0, 32, 32, 3)]
    p = plan((), jobs)
    assert p["blocks"] == 1 and p["segs"] == [(TILES, 0, 0)]
    assert plan((), ())["blocks"] == 0


def test_outside_the_documented_abi():
    for name in ("pca_debug_prep_plan", "pca_debug_prep_images"):
        assert name in _lib.DEBUG_SIGNATURES and name not in _lib.SIGNATURES
    assert pca_hip.lib().pca_debug_prep_plan(None, 0, None, 0) == -1
    words = (ctypes.c_int64 * 5)(0, 33, 0, 0, 0)
    out = (ctypes.c_int64 * 8)()
    assert pca_hip.lib().pca_debug_prep_plan(words, 5, out, 8) != 0
