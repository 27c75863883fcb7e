#!/usr/bin/env python3
"""Self-attention block SAB(X) = MAB(X, X) (set_transformer-master/modules.py:35-41): the bf16 path
(kind 4: projections on k_gemm_bf16, attention on the fused head-dim-32 core, no N x N matrix) against
the exact fp32 chain (which builds A[B h, N, N]).  Training forward, and forward + backward, timed with
HIP events: the median of WINDOWS single-call windows after warm-up.

FLOPs in the reference formulation: attention 4 B N^2 d forward and 10 B N^2 d backward; projections
2 B N (3 din d + d^2) forward and twice that backward.  One JSON line per (shape, mode, pass).
Run each invocation under its own time limit (timeout -k 10 ...)."""
import argparse
import json
import os
import statistics
import sys

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "point-cloud-audio_amd"))
import torch  # noqa: E402

import pca_hip  # noqa: E402
from pca_hip import ops  # noqa: E402

PEAK_TFLOPS = 2500.0          # MI355X dense bf16 MFMA
SHAPES = [(32, 2048, 128, 4), (16, 2048, 256, 8)]     # B, N, d, h (din = d)


def windows(fn, n, warm=3):
    for _ in range(warm):
        fn()
    torch.cuda.synchronize()
    ts = []
    for _ in range(n):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        e1.synchronize()
        ts.append(e0.elapsed_time(e1))
    return statistics.median(ts), min(ts), max(ts)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--windows", type=int, default=25)
    ap.add_argument("--modes", default="bf16,f32")
    ap.add_argument("--shape", default=None, help="B,N,d,h: this shape only (e.g. one per profile)")
    args = ap.parse_args()
    shapes = [tuple(int(v) for v in args.shape.split(","))] if args.shape else SHAPES
    dev = torch.device("cuda", 0)
    pca_hip.lib()
    res = {}
    for B, N, d, h in shapes:
        din = d
        g = torch.Generator().manual_seed(B + N + d)
        params = []
        for k in (din, din, din, d):
            params += [((torch.rand(d, k, generator=g) * 2 - 1) / k ** 0.5).to(dev),
                       ((torch.rand(d, generator=g) * 2 - 1) / k ** 0.5).to(dev)]
        X = torch.randn(B, N, din, generator=g).to(dev).requires_grad_(True)
        G = torch.randn(B, N, d, generator=g).to(dev)
        proj = 2.0 * B * N * (3 * din * d + d * d)
        flops = {"fwd": 4.0 * B * N * N * d + proj, "fwd+bwd": 14.0 * B * N * N * d + 3 * proj}
        for mode in args.modes.split(","):
            pca_hip.set_mode(mode)

            def fwd():
                return ops.mab(X, X, *params, h)

            def fwd_bwd():
                X.grad = None
                fwd().backward(G)

            for name, fn in (("fwd", fwd), ("fwd+bwd", fwd_bwd)):
                med, lo, hi = windows(fn, args.windows)
                tf = flops[name] / (med * 1e-3) / 1e12
                res[(B, N, d, h, mode, name)] = med
                print(json.dumps({"B": B, "N": N, "d": d, "h": h, "mode": mode, "pass": name,
                                  "ms_median": round(med, 4), "ms_min": round(lo, 4), "ms_max": round(hi, 4),
                                  "windows": args.windows, "tflops": round(tf, 2),
                                  "peak_frac": round(tf / PEAK_TFLOPS, 4)}), flush=True)
            torch.cuda.empty_cache()
        pca_hip.set_mode("f32")
        for name in ("fwd", "fwd+bwd"):
            a, b = res.get((B, N, d, h, "f32", name)), res.get((B, N, d, h, "bf16", name))
            if a and b:
                print(f"B={B} N={N} d={d} h={h} {name}: bf16 {b:.3f} ms, f32 chain {a:.3f} ms, "
                      f"speed-up {a / b:.1f}x", flush=True)


if __name__ == "__main__":
    main()
