"""Time per train step at a bench.py configuration with the guarded optimiser step (max_grad_norm +
skip_nonfinite + lr_schedule: pca_grad_sumsq and pca_adam_step_ex; "on") and with AdamW, per-tensor groups
and the averaged copy (pca_adam_step_groups; "new") against the plain one (pca_adam_step; "off").

bench.py's timing: wall time of a window of --steps graph replays between two device syncs.  The
Trainers share the dataset, start from the same weights and take their windows in turn (A B A B ...), so
that clock and thermal drift fall on all alike; reported are the medians and the min - max of the windows.

    python scripts/optim_bench.py [--config cfg2] [--steps 200] [--windows 15]

``--launch``: the optimiser launch alone, at the parameter counts of cfg2 and cfg4 (BASELINE configs[3]):
pca_adam_step and pca_adam_step_ex against pca_adam_step_groups with no option, with the no_decay_groups()
table of that model, with the averaged copy, and with both under decoupled decay.  Each variant is a captured graph of
--steps launches on vectors of its own; the variants take their windows in turn, and the figure is the
window's wall time over its launches (so it holds the gap between two launches of a graph, as in a step).

    python scripts/optim_bench.py --launch [--steps 200] [--windows 15]
"""
import argparse
import ctypes as C
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


def launch_variants(n, groups, dev):
    """{name: enqueue()} of one optimiser launch on n-element vectors of its own, without the norm."""
    L = _lib.lib()
    ends = groups["seg_end"]
    ends_host = (C.c_int64 * len(ends))(*ends)
    ends_dev = torch.tensor(ends, dtype=torch.int64, device=dev)
    ls = torch.tensor(groups["lr_scale"], dtype=torch.float32, device=dev)
    ws = torch.tensor(groups["wd_scale"], dtype=torch.float32, device=dev)
    keep = [ends_host, ends_dev, ls, ws]
    gen = torch.Generator(device="cpu").manual_seed(0)

    def variant(entry, decoupled=False, table=False, avg=False):
        p = (torch.randn(n, generator=gen) * 0.05).to(dev)
        g = (torch.randn(n, generator=gen) * 0.01).to(dev)
        m, v = torch.zeros(n, device=dev), torch.zeros(n, device=dev)
        a = p.clone() if avg else None
        step = torch.zeros(2, dtype=torch.int32, device=dev)
        state = torch.zeros(8, dtype=torch.int32, device=dev)
        cfg = _lib.OptimCfg(1e-4, 0.9, 0.999, 1e-8, 1e-3, 1.0, 0.0, 0)
        gr = _lib.OptimGroups(int(decoupled), len(ends) if table else 0,
                              ends_dev.data_ptr() if table else None, ls.data_ptr() if table else None,
                              ws.data_ptr() if table else None, None if a is None else a.data_ptr(),
                              0.01, 1)
        keep.extend([p, g, m, v, a, step, state, cfg, gr])

        def enqueue():
            st = C.c_void_p(torch.cuda.current_stream(dev).cuda_stream)
            args = (p.data_ptr(), g.data_ptr(), m.data_ptr(), v.data_ptr(), n, C.byref(cfg), None, 0,
                    None, 0, step.data_ptr(), state.data_ptr(), 0)
            if entry == "plain":
                _lib.check(L.pca_adam_step(*args[:5], cfg.lr, cfg.beta1, cfg.beta2, cfg.eps, cfg.weight_decay,
                                           cfg.grad_scale, step.data_ptr(), 0, st), "pca_adam_step")
            elif entry == "ex":
                _lib.check(L.pca_adam_step_ex(*args, st), "pca_adam_step_ex")
            else:
                _lib.check(L.pca_adam_step_groups(*args, C.byref(gr), ends_host if table else None, st),
                           "pca_adam_step_groups")
        return enqueue

    out = {"adam_step": variant("plain"),
           "adam_step_ex": variant("ex"),
           "groups: no option": variant("groups"),
           "groups: table": variant("groups", table=True),
           "groups: average": variant("groups", avg=True),
           "groups: AdamW + table + average": variant("groups", decoupled=True, table=True, avg=True)}
    out["_keep"] = keep
    return out


def time_launches(args, dev):
    for name in ("cfg2", "cfg4"):
        cfg = bench.CONFIGS[name]
        net = models.ST(dim_input=cfg["din"], num_outputs=1, dim_output=cfg["C"], num_inds=cfg["m"],
                        dim_hidden=cfg["d"], num_heads=cfg["h"])
        n = sum(p.numel() for p in net.parameters())
        groups = trainer.resolve_param_groups(net, trainer.no_decay_groups())
        variants = launch_variants(n, groups, dev)
        variants.pop("_keep")
        graphs = {}
        for k, enqueue in variants.items():
            enqueue()                                       # loads the code object outside the capture
            torch.cuda.synchronize(dev)
            graphs[k] = torch.cuda.CUDAGraph()
            with torch.cuda.graph(graphs[k]):
                for _ in range(args.steps):
                    enqueue()
            graphs[k].replay()
        torch.cuda.synchronize(dev)
        us = {k: [] for k in graphs}
        for _ in range(args.windows):
            for k, gph in graphs.items():
                torch.cuda.synchronize(dev)
                t0 = time.perf_counter()
                for _ in range(5):
                    gph.replay()
                torch.cuda.synchronize(dev)
                us[k].append((time.perf_counter() - t0) / (5 * args.steps) * 1e6)
        print(f"{name}: n_params={n} ({4 * n / 1e6:.2f} MB), {len(groups['seg_end'])} segments, "
              f"{args.windows} windows of {5 * args.steps} launches each")
        base = statistics.median(us["adam_step_ex"])
        for k, w in us.items():
            print(f"  {k:<32} median {statistics.median(w):7.2f} us/launch  (min {min(w):.2f}, "
                  f"max {max(w):.2f})  {statistics.median(w) - base:+.2f} us")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--config", default="cfg2", choices=sorted(bench.CONFIGS))
    ap.add_argument("--steps", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=50)
    ap.add_argument("--windows", type=int, default=15)
    ap.add_argument("--mode", default="bf16", choices=["f32", "bf16", "fp8"])
    ap.add_argument("--launch", action="store_true", help="time the optimiser launch alone")
    args = ap.parse_args()
    dev = torch.device("cuda", 0)
    if args.launch:
        time_launches(args, dev)
        return
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
                       lr_schedule=trainer.warmup_cosine(1e-3, args.warmup, total)),
            # AdamW + no_decay_groups() + the averaged copy: pca_adam_step_groups, one launch, no norm
            "new": make(decoupled_weight_decay=True, param_groups=trainer.no_decay_groups(),
                        average_decay=0.99)}
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
    for name in ("on", "new"):
        print(f"  options {name} - off, difference of the medians: "
              f"{(statistics.median(ms[name]) - statistics.median(ms['off'])) * 1e3:+.1f} us")
    print("  options on:", runs["on"].read_optim_stats())


if __name__ == "__main__":
    main()
