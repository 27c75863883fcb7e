"""The three optimiser entry points (csrc/optim.hip) leave the bits that the build before they became one
translation unit left: per case of tests/optim_digest_cases.py, the SHA-256 of p, g, m, v, the averaged copy,
the step words and the state words after three launches equals tests/golden/optim_digest_sha256.json (recorded
by scripts/optim_digest_golden.py from that earlier build, which also checked that the guarded cases hold a
clipped step, an unclipped one and a skipped one)."""
import functools
import json
import os

import pytest
import torch

import optim_digest_cases as oc

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "optim_digest_sha256.json")


@functools.lru_cache(maxsize=None)
def _golden():
    with open(GOLDEN) as f:
        return json.load(f)["cases"]


@pytest.fixture(scope="module")
def dev():
    import pca_hip
    pca_hip.lib()
    return torch.device("cuda", 0)


def test_the_recording_holds_every_case():
    want = {oc.key(n, o, z, v) for n in oc.SIZES for o in oc.OFFSETS for z in oc.ZERO_GRAD for v in oc.VARIANTS}
    assert set(_golden()) == want


@pytest.mark.parametrize("variant", list(oc.VARIANTS))
@pytest.mark.parametrize("n", oc.SIZES)
def test_bits_of_the_earlier_build(dev, n, variant):
    moved = []
    for offset in oc.OFFSETS:
        for zg in oc.ZERO_GRAD:
            got, state = oc.run_case(dev, n, offset, zg, variant)
            if got != _golden()[oc.key(n, offset, zg, variant)]:
                moved.append((oc.key(n, offset, zg, variant), state))
    assert not moved, moved
