"""pca_st_step_reproducible without a GPU: the answer is host logic over the step's plan.  1 only in the bf16
mode, for the fused d = 128 / d = 256 plans on dense sets and for the d = 64 chain on the fused attention core
up to 256 sets (tests/test_gpu_sd64_reproducible.py holds every 1 to its word on the device)."""
import ctypes as C

import pytest

from pca_hip import _lib


def _ask(B, N, din, d, h, m, mode, lengths=0, k=1, Cc=10):
    return _lib.lib().pca_st_step_reproducible(C.byref(_lib.StConfig(B, N, din, d, h, m, k, Cc, mode)), lengths)


@pytest.mark.parametrize("cfg,lengths,want", [
    ((6, 1025, 2, 64, 8, 64), 0, 1),            # FST
    ((3, 5120, 3, 64, 8, 64), 0, 1),            # 3ST
    ((4, 300, 2, 64, 8, 64), 1, 1),             # padded sets
    ((5, 130, 2, 64, 4, 16), 0, 1),             # head dim 16
    ((256, 1025, 2, 64, 8, 64), 0, 1),
    ((257, 1025, 2, 64, 8, 64), 0, 0),          # colsum over more than 256 sets adds with atomics
    ((4, 300, 2, 64, 2, 64), 0, 0),             # head dim 32: not the fused core
    ((4, 300, 5, 64, 8, 64), 0, 0),             # din 5: layer 1's weight gradients on the split-K GEMM
    ((4, 77, 3, 32, 8, 24), 0, 0),              # another chain width
    ((128, 512, 2, 128, 4, 16), 0, 1),          # cfg2: fused d = 128
    ((128, 512, 2, 128, 4, 16), 1, 0),
    ((128, 512, 2, 128, 4, 20), 0, 0),          # m = 20: the chain at d = 128
    ((4, 128, 2, 256, 8, 32), 0, 1),            # fused d = 256
    ((4, 128, 2, 256, 8, 16), 0, 0),
], ids=str)
def test_answers(cfg, lengths, want):
    assert _ask(*cfg, _lib.MODE_BF16, lengths) == want
    assert _ask(*cfg, _lib.MODE_F32, lengths) == 0
    assert _ask(*cfg, _lib.MODE_FP8, lengths) == 0


def test_slab_switch_and_bad_configs(monkeypatch):
    monkeypatch.setenv("PCA_WGRAD_SLABS", "0")          # the d = 128 tail on fp32 atomics
    assert _ask(128, 512, 2, 128, 4, 16, _lib.MODE_BF16) == 0
    assert _ask(6, 1025, 2, 64, 8, 64, _lib.MODE_BF16) == 1
    monkeypatch.delenv("PCA_WGRAD_SLABS")
    assert _ask(128, 512, 2, 128, 4, 16, _lib.MODE_BF16) == 1
    assert _ask(6, 1025, 2, 64, 8, 64, _lib.MODE_BF16, k=2) == 0      # the train step needs k == 1
    assert _ask(0, 1025, 2, 64, 8, 64, _lib.MODE_BF16) == 0           # not a configuration
