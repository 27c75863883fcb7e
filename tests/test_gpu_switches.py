"""The A/B switches that select between two implementations of the SAME arithmetic must not move a
bit of the result: each case runs one forward + backward of the whole-model engine in a fresh
process per setting (the library reads these switches once per process) and compares SHA-256 of the
logits, the loss and the 45 gradients.

* ``PCA_D128_DZ_MASK`` / ``PCA_D256_DZ_MASK``: dZ = dY.[Z > 0] written by the backward and read back by
  the fc_o weight-gradient job, or that job masking dY with the forward's ReLU bits itself - the same
  bf16 values reach the same MFMAs in the same order.
* ``PCA_WGRAD256_DMA``: operand tiles of the 256-wide weight gradients through registers or by LDS-DMA.
* ``PCA_PACK_DEFER`` is covered in test_gpu_parity.py.
* ``PCA_WGRAD_SLABS`` (fixed-order slabs vs fp32 atomics) in tests/test_gpu_fullsize.py
  (test_d128_step_is_bit_reproducible), ``PCA_SET128`` / ``PCA_SET128_HEAD`` (the set-resident forward and
  its fused head stages against the per-block launches) in tests/test_gpu_set128.py.

Round 4 removed every other ``PCA_*`` switch of the library (22 of them: the defaults had been the measured
winners for a round or more).  The kernels only those switches could select went with them:
``k_attn1_bwd`` and ``k_attn1_bwd2``, every ``k_rowgemm`` instantiation (four modes, two wave counts, fp8),
``k_fq_attn_fwd<256, 2>`` / ``k_fq_attn_bwd<256, 2>``, and the ``k_mab1_fwd`` instantiations for bf16
activations at d = 256 and for fc_q in fp8.  What is left, all covered by a test:
PCA_SET128, PCA_SET128_HEAD, PCA_WGRAD_SLABS, PCA_D128_DZ_MASK, PCA_D256_DZ_MASK, PCA_WGRAD256_DMA,
PCA_D256_MID, PCA_D256_AB (+ PCA_PACK_DEFER in the Python trainer).  PCA_AB_ABLATE / PCA_AB_STAMPSEL /
PCA_AB_ABREAST / PCA_DBG_WG exist in the diagnostic builds of scripts/experiments only (#ifdef).

Switches between two implementations with a different summation order or operand rounding point
(``PCA_D256_MID``: the per-set mid stage in one launch or five; ``PCA_D256_AB``: the producer / consumer
forward kernel or the one-role kernel of round 2) are held to each other within the bf16 criterion the
oracle parity tests use (tests/util.py: close_robust) - both are also held to the oracle there.
"""
import os
import subprocess
import sys

import pytest

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)

SCRIPT = r"""
import hashlib, sys
sys.path.insert(0, {pkg!r}); sys.path.insert(0, {tests!r}); sys.path.insert(0, {golden!r})
import torch
import models, inputs as gi
from pca_hip import _lib, trainer
B, N, din, d, h, m, C = {shape}
dev = torch.device("cuda", 0)
torch.manual_seed(11)
net = models.ST(dim_input=din, num_outputs=1, dim_output=C, num_inds=m, dim_hidden=d, num_heads=h).to(dev)
X = torch.from_numpy(gi.pc_input(12, B, N, din)).to(dev)
y = torch.from_numpy(gi.labels(13, B, C)).to(dev)
eng = trainer.STEngine(net, B, N, _lib.MODE_BF16, training=True)
eng.fwd_bwd(X, y, phase=-1)
torch.cuda.synchronize()
assert torch.isfinite(eng.grads).all()
hsh = hashlib.sha256()
for t in (eng.logits, eng.loss, eng.grads):
    hsh.update(t.detach().cpu().numpy().tobytes())
print("HASH", hsh.hexdigest())
import numpy as np, os
if os.environ.get("PCA_TEST_DUMP"):
    np.savez(os.environ["PCA_TEST_DUMP"], logits=eng.logits.detach().cpu().numpy(),
             loss=eng.loss.detach().cpu().numpy(), grads=eng.grads.detach().cpu().numpy())
"""


def _run(shape, env):
    code = SCRIPT.format(pkg=os.path.join(ROOT, "point-cloud-audio_amd"), tests=HERE,
                         golden=os.path.join(HERE, "golden"), shape=shape)
    e = dict(os.environ)
    e.update(env)
    out = subprocess.run([sys.executable, "-c", code], env=e, capture_output=True, text=True, timeout=600)
    assert out.returncode == 0, out.stderr[-2000:]
    return [ln for ln in out.stdout.splitlines() if ln.startswith("HASH")][-1]


CASES = [
    # (shape, variable, why this shape)
    ((6, 512, 2, 128, 4, 16, 50), "PCA_D128_DZ_MASK", "configs[1] architecture: both d = 128 blocks take the masked job"),
    ((3, 384, 3, 256, 8, 32, 10), "PCA_D256_DZ_MASK", "configs[3] architecture, N % 128 == 0: masked job in k_wgrad256_dma"),
    ((3, 384, 3, 256, 8, 32, 10), "PCA_WGRAD256_DMA", "LDS-DMA ring against register staging (the latter forces dZ to be written)"),
]


@pytest.mark.parametrize("shape,var,why", CASES, ids=[c[1] for c in CASES])
def test_switch_is_bit_neutral(shape, var, why):
    on = _run(shape, {})
    off = _run(shape, {var: "0"})
    assert on == off, f"{var}=0 changes the result ({why})"


CLOSE_CASES = [
    ((3, 384, 3, 256, 8, 32, 10), "PCA_D256_MID"),
    ((3, 384, 3, 256, 8, 32, 10), "PCA_D256_AB"),
]


@pytest.mark.parametrize("shape,var", CLOSE_CASES, ids=[c[1] for c in CLOSE_CASES])
def test_switch_is_numerically_neutral(shape, var, tmp_path):
    import numpy as np
    import grad_bars as gb
    from oracle import st_oracle as orc
    from util import close, close_robust
    fa, fb = str(tmp_path / "a.npz"), str(tmp_path / "b.npz")
    _run(shape, {"PCA_TEST_DUMP": fa})
    _run(shape, {"PCA_TEST_DUMP": fb, var: "0"})
    a, b = np.load(fa), np.load(fb)
    close(a["logits"], b["logits"], 3e-2, f"{var}: logits")
    assert abs(float(a["loss"][0]) - float(b["loss"][0])) < 3e-2
    close_robust(a["grads"], b["grads"], 5e-2, f"{var}: gradients", outlier_frac=5e-3)
    # the same 45 gradients tensor by tensor, each on its own scale
    B, N, din, d, h, m, C = shape
    shapes = orc.st_param_shapes(din, 1, C, m, d)
    gb.judge(a["grads"], b["grads"], gb.PEER, shapes, f"{var}=1 vs {var}=0")
