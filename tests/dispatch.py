"""Dispatch witness: which kernel families an eager library call launched.

Built on the library's measurement hook (include/pca_hip.h, ``pca_prof_start`` / ``pca_prof_stop``):
while it is armed for one family, every eager launch of that family is recorded; launches onto a
stream that is being captured are not.  The hook is process-global and refuses a second arm, so the
witness always disarms it, also when the body raises.

Families (the ``ProfScope`` sites in csrc/):

* ``K_GEMM_F32``  k_gemm_f32 only.  The bf16 operand chain (gemm_bf16.hip) and the fused kernels are
  not counted, so in PCA_MODE_BF16 this counts the fp32 classifier Linear, and in PCA_MODE_F32 every
  GEMM of the exact chain;
* ``K_MAB1_FWD`` / ``K_MAB1_BWD`` / ``K_MAB0_FWD`` / ``K_MAB0_BWD``  the fused bf16 / fp8 blocks
  (d = 128: mab1_bf16.hip, mab0_bf16.hip, isab_bf16.hip; d = 256: d256_*.hip);
* ``K_WGRAD``  the bf16 weight-gradient GEMMs;
* ``K_SET_FWD``  the set-resident d = 128 forward (set128_fwd.hip).
"""
import contextlib
import ctypes as C

import torch

from pca_hip import _lib

FAMILIES = {
    "gemm_f32": _lib.K_GEMM_F32,
    "mab1_fwd": _lib.K_MAB1_FWD,
    "mab1_bwd": _lib.K_MAB1_BWD,
    "mab0_fwd": _lib.K_MAB0_FWD,
    "mab0_bwd": _lib.K_MAB0_BWD,
    "wgrad": _lib.K_WGRAD,
    "set_fwd": _lib.K_SET_FWD,
}

# launches recorded per arm; a count that reaches it would be a lower bound only
MAX_LAUNCHES = 1024


class Witness:
    def __init__(self, kernel_id):
        self.kernel_id = kernel_id
        self.launches = None


@contextlib.contextmanager
def witness(kernel_id, max_launches=MAX_LAUNCHES):
    """Count the eager launches of one kernel family inside the ``with`` body:

        with witness(_lib.K_SET_FWD) as w:
            eng.fwd_bwd(X, y)
        assert w.launches == 1
    """
    L = _lib.lib()
    torch.cuda.synchronize()
    _lib.check(L.pca_prof_start(kernel_id, max_launches), "pca_prof_start")
    w = Witness(kernel_id)
    ms, n, fl, by = C.c_double(), C.c_int64(), C.c_double(), C.c_double()
    try:
        yield w
    finally:
        torch.cuda.synchronize()
        rc = L.pca_prof_stop(C.byref(ms), C.byref(n), C.byref(fl), C.byref(by))
    _lib.check(rc, "pca_prof_stop")
    assert n.value < max_launches, f"kernel family {kernel_id}: {n.value} launches saturate the witness"
    w.launches = int(n.value)


def launches(fn, families=tuple(FAMILIES)):
    """Run the eager call ``fn()`` once per family (the hook watches one family at a time) and
    return {family name: launch count}."""
    out = {}
    for name in families:
        with witness(FAMILIES[name]) as w:
            fn()
        out[name] = w.launches
    return out
