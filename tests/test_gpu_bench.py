"""bench.py's plain run and --dump-outputs: a fresh process per run (the bench sets up the device
itself).  A plain run reports the headline line and nothing that needs runs of its own (--full's
windows, roofline and CPU baseline); the dump holds what the last timed step computed, float32,
within the 64 MB budget, and two runs with the same arguments write the same arrays."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DUMPED = ("logits", "loss", "params", "adam_m", "adam_v")


def _bench(out_dir, steps):
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps",
                        str(steps), "--warmup", "2", "--dump-outputs", str(out_dir)],
                       capture_output=True, text=True, timeout=300, cwd=ROOT)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-3000:]
    lines = [ln for ln in r.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1, r.stdout
    return json.loads(lines[0])


def test_plain_run_and_dumped_outputs(tmp_path):
    res = _bench(tmp_path / "a", 3)
    for k in ("metric", "value", "unit", "higher_is_better", "dtype", "ms_per_step"):
        assert k in res, k
    assert res["steps"] == 3 and res["warmup"] == 2 and res["ms_per_step"] > 0
    assert res["unit"] == "clips/s" and res["higher_is_better"] is True
    for k in ("windows", "roofline", "cpu_baseline"):
        assert k not in res, k
    total = 0
    for name in DUMPED:
        a = np.load(tmp_path / "a" / f"{name}.npy")
        assert a.dtype == np.float32 and a.size > 0 and np.isfinite(a).all(), name
        total += a.nbytes
    assert total <= 64 << 20
    assert np.load(tmp_path / "a" / "logits.npy").shape == (128, 50)       # cfg2: B x C
    _bench(tmp_path / "b", 3)
    for name in DUMPED:
        assert np.array_equal(np.load(tmp_path / "a" / f"{name}.npy"),
                              np.load(tmp_path / "b" / f"{name}.npy")), name
