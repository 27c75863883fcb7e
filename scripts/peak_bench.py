"""What spectral-peak point sets cost on one MI355X: the launch, the training step, the sweep.

    python scripts/peak_bench.py [--parts launch,step,sweep] [--out FILE]

  launch  pca_peak_points at B = 128 sets of (F, Nt) = (512, 1) and (512, 4) on bench.py's synthetic
          log-magnitude distribution, beside pca_subsample_points mode 0 (max-K) at K = N on the same values:
          --calls calls captured into one hipGraph (the device's time, not the host's launch rate), a
          replay between two HIP events, the launches taking their replays in turn, median and min - max
          of --windows replays.  The peak launch is timed at K = N (the same output size as the
          max-K launch) and at the K a user would keep (128 per frame), radius (1, 0) and (4, 1).
  step    the training step at the cfg2 model (d = 128, 4 heads, 16 inducing points, bf16, B = 128, hipGraph
          replay) over dataset.ESC_wave_pc with jitter, gain and three window lengths: the dense step on all
          512 points beside the step over PeakPoints(K = 128, radius_f = 1) - the frame launch, the peak
          launch and the step with lengths.  scripts/mask_bench.py's timing: wall time of windows of --steps
          replays between two device syncs, the Trainers in turn.  The dense Trainer runs no line this
          feature added: it is the parent's step.
  sweep   evalsweep.peak_sweep over the FST corpus of scripts/sweep_bench.py (8 clips of 5 s, 1728 frames of
          1025 bins, the shipped model shape, random weights) beside subsample_sweep's max-K and random-K
          passes on the same K grid, as wall time and per set evaluated.
Prints one JSON line per part (and appends them to --out)."""
import argparse
import json
import os
import statistics
import sys
import time

os.environ["PCA_PACK_DEFER"] = "0"
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "point-cloud-audio_amd"), os.path.join(ROOT, "scripts")]
import numpy as np
import torch

import bench
import dataset
import evalsweep
import models
import pca_hip
from pca_hip import _lib, trainer


def _summary(ms):
    return {"median": round(statistics.median(ms), 3), "min": round(min(ms), 3), "max": round(max(ms), 3)}


def _event_windows(fns, calls, windows, dev):
    """us per call of every fn: ``calls`` calls captured into one hipGraph (so that the device, not the
    host's launch rate, sets the time), ``windows`` replays of it between two HIP events, in turn."""
    graphs = {}
    side = torch.cuda.Stream(dev)
    for name, fn in fns.items():
        side.wait_stream(torch.cuda.current_stream(dev))
        with torch.cuda.stream(side):
            for _ in range(20):
                fn()
        torch.cuda.current_stream(dev).wait_stream(side)
        torch.cuda.synchronize(dev)
        graphs[name] = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graphs[name]):
            for _ in range(calls):
                fn()
        graphs[name].replay()
    torch.cuda.synchronize(dev)
    us = {k: [] for k in fns}
    for _ in range(windows):
        for name, g in graphs.items():
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            g.replay()
            b.record()
            b.synchronize()
            us[name].append(a.elapsed_time(b) / calls * 1e3)
    return {k: _summary(v) for k, v in us.items()}


def part_launch(args, dev):
    res = {}
    B = 128
    for F, Nt in ((512, 1), (512, 4)):
        N, din = F * Nt, 2 if Nt == 1 else 3
        g = torch.Generator(device="cpu").manual_seed(F + Nt)
        v = torch.clamp(torch.randn((B, Nt, F), generator=g) * 3.0 - 9.0, -18.4, 0.0).to(dev)
        farr = torch.linspace(0, 0.5, F, device=dev)
        tarr = torch.linspace(0, 0.1, Nt, device=dev) if Nt > 1 else None
        idx = torch.arange(B, device=dev)
        if Nt == 1:
            spec = v[:, 0, :].t()                                   # [F, T] view, one set contiguous
            X = pca_hip.pack_points_2d(spec, farr, idx)[0]
        else:
            spec = v.permute(2, 1, 0)                               # [F, Nt, S] view
            X = pca_hip.pack_points_3d(spec, farr, tarr, idx)[0]
        out_sub = torch.empty((B, N, din), device=dev)
        fns = {"maxk_K=N": lambda: pca_hip.subsample_points(spec, farr, tarr, idx, N, pca_hip.MAXK, 0, 0,
                                                            out=out_sub)}
        counts = {}
        for rf, rt in ((1, 0), (4, 1)):
            for K in (N, 128 * Nt):
                out = torch.empty((B, K, din), device=dev)
                ln = torch.empty(B, dtype=torch.int32, device=dev)
                fns[f"peak_r{rf}_{rt}_K={K}"] = (lambda K=K, rf=rf, rt=rt, out=out, ln=ln: pca_hip.peak_points(
                    X, F, Nt, K, rf, rt, out=out, lengths_out=ln))
            c = pca_hip.peak_points(X, F, Nt, N, rf, rt, want_count=True)[2].float()
            counts[f"r{rf}_{rt}"] = {"mean": round(c.mean().item(), 1), "max": int(c.max())}
        res[f"{F}x{Nt}"] = {"us_per_call": _event_windows(fns, args.calls, args.windows, dev),
                            "peaks_per_set": counts}
    return {"launch": dict(res, B=B, calls=args.calls, windows=args.windows)}


def part_step(args, dev):
    cfg = dict(bench.CONFIGS["cfg2"])
    n_fft, B, C_ = cfg["n_fft"], cfg["B"], cfg["C"]
    assert cfg["din"] == 2 and cfg["ntemp"] == 1
    classes = [i % C_ for i in range(args.clips)]
    clips = [torch.from_numpy(bench.synth_clip(i, c)).to(dev) for i, c in enumerate(classes)]
    base = dict(drop_nyquist=True, jitter=n_fft // 4, gain_db=6.0,
                win_lengths=(n_fft, n_fft // 2, 3 * n_fft // 4), seed=1, device=dev)

    def make(peaks):
        ds = dataset.ESC_wave_pc(clips, classes, bench.FS, n_fft, **base)
        assert ds.num_points == 512
        if peaks:
            ds = dataset.PeakPoints(ds, 128, radius_f=1)
        torch.manual_seed(1)
        net = models.ST(dim_input=2, num_outputs=1, dim_output=C_, num_inds=cfg["m"],
                        dim_hidden=cfg["d"], num_heads=cfg["h"]).to(dev)
        return trainer.Trainer(net, ds, B, lr=1e-3, weight_decay=1e-3, mode=_lib.MODE_BF16, seed=1)

    runs = {"dense": make(False), "peaks": make(True)}
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
    for name, tr in runs.items():
        loss, _ = tr.read_stats()
        assert loss == loss, f"non-finite training loss ({name})"
    ln = runs["peaks"].lengths.float()
    return {"step": {"ms_per_step": {k: _summary(v) for k, v in ms.items()}, "B": B, "steps": args.steps,
                     "windows": args.windows,
                     "peaks_kept_last_step": {"mean": round(ln.mean().item(), 1), "min": int(ln.min()),
                                              "max": int(ln.max())}}}


def part_sweep(args, dev):
    import sweep_bench
    C_ = 10
    waves = [torch.from_numpy(sweep_bench.synth_clip(i, i % C_)).to(dev) for i in range(8)]
    spec, foff = pca_hip.stft_logmag_batch(waves, 2048, 2048, 1024, drop_nyquist=False, frame_major=True)
    F = spec.shape[1]
    y = np.concatenate([np.full(foff[c + 1] - foff[c], c % C_) for c in range(len(waves))])
    x, farr = spec.t(), np.linspace(0, sweep_bench.FS / 2, F) / sweep_bench.FS
    torch.manual_seed(0)
    net = models.ST(dim_input=2, dim_output=C_, num_inds=64, dim_hidden=64, num_heads=8).to(dev)
    list_K = evalsweep.default_list_K(evalsweep.most_peaks(F))
    full = (x.shape[1] // 8) * 8
    runs = {"peak_sweep": lambda: evalsweep.peak_sweep(net, x, y, farr, list_K=list_K),
            "subsample_sweep": lambda: evalsweep.subsample_sweep(net, x, y, farr, list_K=list_K, n_runs=1)}
    evals = {"peak_sweep": full * len(list_K), "subsample_sweep": 2 * full * len(list_K)}
    secs = {k: [] for k in runs}
    out = None
    for rep in range(args.sweep_reps + 1):
        for name, fn in runs.items():
            torch.cuda.synchronize(dev)
            t0 = time.perf_counter()
            r = fn()
            torch.cuda.synchronize(dev)
            if rep:                                               # the first pass builds the engines
                secs[name].append(time.perf_counter() - t0)
            if name == "peak_sweep":
                out = r
    res = {name: {"wall_s": _summary(v), "sets_evaluated": evals[name],
                  "us_per_set": round(1e6 * statistics.median(v) / evals[name], 2)}
           for name, v in secs.items()}
    res["list_K"] = list_K
    res["mean_points"] = {k: round(v, 1) for k, v in out["mean_points"].items()}
    res["frames"], res["bins"] = int(x.shape[1]), int(F)
    return {"sweep": res}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--parts", default="launch,step,sweep")
    ap.add_argument("--calls", type=int, default=1000)
    ap.add_argument("--windows", type=int, default=9)
    ap.add_argument("--steps", type=int, default=1000)
    ap.add_argument("--warmup", type=int, default=100)
    ap.add_argument("--clips", type=int, default=48)
    ap.add_argument("--sweep-reps", type=int, default=3)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    dev = torch.device("cuda", 0)
    parts = dict(launch=part_launch, step=part_step, sweep=part_sweep)
    for name in args.parts.split(","):
        line = json.dumps(parts[name](args, dev))
        print(line, flush=True)
        if args.out:
            with open(args.out, "a") as f:
                f.write(line + "\n")


if __name__ == "__main__":
    main()
