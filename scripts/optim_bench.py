"""Time per train step at a bench.py configuration with the guarded optimiser step (max_grad_norm +
skip_nonfinite + lr_schedule: pca_grad_sumsq and pca_adam_step_ex) against the plain one (pca_adam_step).

bench.py's timing: wall time of a window of --steps graph replays between two device syncs.  The two
Trainers share the dataset, start from the same weights and take their windows in turn (A B A B ...), so
that clock and thermal drift fall on both alike; reported are the medians and the min - max of the windows.

    python scripts/optim_bench.py [--config cfg2] [--steps 200] [--windows 15]
"""
import argparse
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "point-cloud-audio_amd")]
import torch

import bench
import models
from pca_hip import _lib, trainer


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--config", default="cfg2", choices=sorted(bench.CONFIGS))
    ap.add_argument("--steps", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=50)
    ap.add_argument("--windows", type=int, default=15)
    ap.add_argument("--mode", default="bf16", choices=["f32", "bf16", "fp8"])
    args = ap.parse_args()
    dev = torch.device("cuda", 0)
    cfg = dict(bench.CONFIGS[args.config])
    mode = {"f32": _lib.MODE_F32, "bf16": _lib.MODE_BF16, "fp8": _lib.MODE_FP8}[args.mode]
    ds, _ = bench.build_dataset(cfg, 48, dev, seed=0)
    total = args.warmup + args.steps * args.windows

    def make(**options):
        torch.manual_seed(1)
        net = models.ST(dim_input=cfg["din"], num_outputs=1, dim_output=cfg["C"], num_inds=cfg["m"],
                        dim_hidden=cfg["d"], num_heads=cfg["h"]).to(dev)
        return trainer.Trainer(net, ds, cfg["B"], lr=1e-3, weight_decay=1e-3, mode=mode, seed=1, **options)

    runs = {"off": make(),
            "on": make(max_grad_norm=1.0, skip_nonfinite=True,
                       lr_schedule=trainer.warmup_cosine(1e-3, args.warmup, total))}
    for tr in runs.values():
        for _ in range(args.warmup):
            tr.step()
    torch.cuda.synchronize(dev)
    ms = {k: [] for k in runs}
    for _ in range(args.windows):
        for name, tr in runs.items():
            torch.cuda.synchronize(dev)
            t0 = time.perf_counter()
            for _ in range(args.steps):
                tr.step()
            torch.cuda.synchronize(dev)
            ms[name].append((time.perf_counter() - t0) / args.steps * 1e3)
    print(f"{args.config} {args.mode} B={cfg['B']} n_params={runs['on'].eng.flat.numel()} "
          f"partials={runs['on'].norm_partials.numel()}: {args.windows} windows of {args.steps} steps each")
    for name in runs:
        w = ms[name]
        print(f"  options {name:<3}: median {statistics.median(w):.4f} ms/step  (min {min(w):.4f}, max {max(w):.4f})")
    print(f"  difference of the medians: {(statistics.median(ms['on']) - statistics.median(ms['off'])) * 1e3:+.1f} us")
    print("  options on:", runs["on"].read_optim_stats())


if __name__ == "__main__":
    main()
