"""Whole calls after the preparation launch became a plan (csrc/prep_plan.hpp: segments over one flat block index,
weight images by tiles, the pack's requests re-ordered): nothing may move a bit.  Every pinned output of every case
of tests/prep_rebuild_cases.py has the SHA-256 that the PARENT commit's build produced
(tests/golden/prep_rebuild_sha256.json, recorded by scripts/prep_rebuild_golden.py from a library built from the
parent, never from this tree's), and two passes of this build agree.

Cases: the set-resident d = 128 step; the per-block d = 128 step, plain and padded with `lengths`; the cursor-mode
Trainer with the pack deferred into the preparation launch, three steps replayed from a graph (the packed batch,
its labels and the updated parameters are hashed as well); a forward-only call (no loss exists: logits alone);
d = 256, h = 8, m = 32 (logits and loss only: its weight gradients are summed by fp32 atomics)."""
import functools
import json
import os

import pytest
import torch

import prep_rebuild_cases as pc

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "prep_rebuild_sha256.json")


@functools.lru_cache(maxsize=None)
def _golden():
    with open(GOLDEN) as f:
        return json.load(f)


@functools.lru_cache(maxsize=None)
def _run(key):
    import pca_hip
    pca_hip.lib()
    dev = torch.device("cuda", 0)
    return pc.run(dev, key), pc.run(dev, key)


@pytest.mark.parametrize("key", list(pc.CASES))
def test_two_passes(key):
    a, b = _run(key)
    assert a.keys() == b.keys()
    for k in a:
        assert torch.isfinite(a[k].float()).all(), (key, k)
        assert torch.equal(a[k], b[k]), (key, k)


@pytest.mark.parametrize("key", list(pc.CASES))
def test_parent_hashes(key):
    a, _ = _run(key)
    want = _golden()["cases"][key]
    got = pc.hashes(a)
    assert "logits" in got and ("loss" in got or pc.CASES[key][0] == "forward")
    assert got.keys() == want.keys(), (sorted(got), sorted(want))
    if pc.CASES[key][0] != "forward" and key not in pc.LOGITS_AND_LOSS_ONLY:
        assert len(got) >= 47                                     # logits, loss and the 45 gradients
    moved = [k for k in want if got[k] != want[k]]
    assert not moved, (key, moved)
