"""What the pooling attention costs on top of an inference forward, on one GPU.

  python scripts/pool_attn_bench.py [--iters 20] [--windows 9] [--out FILE]

For the shipped FST shape (B = 128, N = 1025, din = 2, d = 64, h = 8, m = 64), the shipped 3ST shape
(B = 16, N = 5120, din = 3, same model) and cfg4's (B = 32, N = 4096, din = 3, d = 256, h = 8, m = 32),
random weights and seeded sets (the times do not depend on the values), in F32 mode:
  * pca_st_forward and pca_st_pool_attention (logits + attn + key): median over ``--windows`` HIP-event
    windows of ``--iters`` calls each, after a warm-up of every shape;
  * the added time per call = the difference of the two medians, and the effective rate of the attention
    launches over the bytes the algorithm must read, B N d 4 (the second ISAB's output, once), against the
    8 TB/s this project quotes for the MI355X's HBM.  attn itself (B k h N 4 bytes, written, read and
    written again) is not counted: the figure is the rate at which the map of a batch is produced.
Prints one JSON line (and writes it to --out).  A timing needs the GPU: without one this script fails."""
import argparse
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "point-cloud-audio_amd")]

HBM_PEAK = 8.0e12
SHAPES = {
    "fst": dict(B=128, N=1025, din=2, d=64, h=8, m=64),
    "3st": dict(B=16, N=5120, din=3, d=64, h=8, m=64),
    "cfg4": dict(B=32, N=4096, din=3, d=256, h=8, m=32),
}


def _median_ms(fn, iters, windows):
    """Median over ``windows`` of (HIP-event time of ``iters`` back-to-back calls) / iters, in ms."""
    out = []
    for _ in range(windows):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(iters):
            fn()
        b.record()
        b.synchronize()
        out.append(a.elapsed_time(b) / iters)
    return float(np.median(out)), float(np.min(out)), float(np.max(out))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--windows", type=int, default=9)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("pool_attn_bench: no GPU (a timing cannot be taken on the host)")

    import models
    from pca_hip import _lib
    from pca_hip.trainer import STEngine

    dev = torch.device("cuda", 0)
    res = {"device": torch.cuda.get_device_name(0), "iters": args.iters, "windows": args.windows,
           "mode": "f32", "shapes": {}}
    for name, s in SHAPES.items():
        torch.manual_seed(0)
        net = models.ST(dim_input=s["din"], dim_output=10, num_inds=s["m"], dim_hidden=s["d"],
                        num_heads=s["h"]).to(dev).eval()
        rng = np.random.Generator(np.random.PCG64(7))
        X = torch.from_numpy(rng.normal(-9, 3, size=(s["B"], s["N"], s["din"])).astype(np.float32)).to(dev)
        eng = STEngine(net, s["B"], s["N"], _lib.MODE_F32, training=False)
        for _ in range(3):                                     # warm-up: both calls, this shape
            eng.forward(X)
            eng.attention(X)
        torch.cuda.synchronize()
        fwd = _median_ms(lambda: eng.forward(X), args.iters, args.windows)
        att = _median_ms(lambda: eng.attention(X), args.iters, args.windows)
        added = att[0] - fwd[0]
        nbytes = s["B"] * s["N"] * s["d"] * 4
        res["shapes"][name] = dict(
            s, forward_ms=fwd[0], forward_ms_min_max=fwd[1:], pool_attention_ms=att[0],
            pool_attention_ms_min_max=att[1:], added_ms=added, x_bytes=nbytes,
            effective_GBps=(nbytes / (added * 1e-3) / 1e9) if added > 0 else None,
            share_of_8TBps=(nbytes / (added * 1e-3) / HBM_PEAK) if added > 0 else None)
    line = json.dumps(res)
    print(line)
    if args.out:
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
