"""What reassigned point sets cost on one MI355X: the launch and the training step.

    python scripts/reassign_bench.py [--parts launch,step] [--out FILE]

  launch  pca_frame_points_reassigned beside pca_frame_points in the same run, on the same resident corpus
          and the same batch: n_fft 1024 with the Nyquist bin dropped (512 bins), B = 128, Nt = 1 (axes "f")
          and Nt = 8 (axes "ft"), jitter and gain on.  scripts/peak_bench.py's timing: --calls calls captured
          into one hipGraph (the device's time, not the host's launch rate), a replay between two HIP
          events, the launches taking their replays in turn, median and min - max of --windows replays.
          The reassigned launch runs two transforms where the plain one runs one.
  step    the training step at the cfg2 model (d = 128, 4 heads, 16 inducing points, bf16, B = 128, hipGraph
          replay) over dataset.ESC_wave_pc with jitter, gain and three window lengths, with and without
          ``reassign=True``: wall time of windows of --steps replays between two device syncs, the Trainers
          in turn.  The Trainer without the switch runs no line this feature added.
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
import torch

import bench
import dataset
import models
import pca_hip
from pca_hip import _lib, trainer
from peak_bench import _event_windows, _summary


def part_launch(args, dev):
    n_fft, B = 1024, 128
    classes = [i % 10 for i in range(args.clips)]
    clips = [torch.from_numpy(bench.synth_clip(i, c)).to(dev) for i, c in enumerate(classes)]
    res = {}
    for Nt in (1, 8):
        kw = dict(jitter=n_fft // 4, gain_db=6.0, seed=1, device=dev)
        ds = (dataset.ESC_wave_pc(clips, classes, bench.FS, n_fft, drop_nyquist=True, **kw) if Nt == 1
              else dataset.ESC_wave_pc_temp(clips, classes, bench.FS, n_fft, Nt, **kw))
        assert ds.F == 512 and len(ds) >= B
        waves, woff, soff, f32, t32, lab = ds._resident()
        g = torch.Generator(device="cpu").manual_seed(Nt)
        idx = torch.randint(0, len(ds), (B,), generator=g).to(dev)
        win = torch.tensor([n_fft], dtype=torch.int32, device=dev)
        out = {k: torch.empty((B, Nt * ds.F, 2 if Nt == 1 else 3), device=dev) for k in ("plain", "reassigned")}
        lab_out = torch.empty(B, dtype=torch.int64, device=dev)
        pos = (waves, woff, soff, idx, n_fft, ds.hop, ds.F, f32, t32, Nt)
        common = dict(max_len=ds._max_len, min_len=ds._min_len, clip_labels=lab, jitter=ds.jitter,
                      gain_db=ds.gain_db, win_lengths=win, seed=1, draw=1, labels_out=lab_out)
        axes = "f" if Nt == 1 else "ft"
        fns = {"plain": lambda: pca_hip.frame_points(*pos, out=out["plain"], **common),
               "reassigned": lambda: pca_hip.frame_points_reassigned(*pos, out=out["reassigned"], axes=axes,
                                                                     **common)}
        us = _event_windows(fns, args.calls, args.windows, dev)
        moved = (out["reassigned"][:, :, 0] != out["plain"][:, :, 0]).float().mean().item()
        assert torch.equal(out["reassigned"][:, :, -1], out["plain"][:, :, -1])
        res[f"Nt={Nt}"] = {"us_per_call": us, "frames": B * Nt, "points_moved": round(moved, 3),
                           "ratio": round(us["reassigned"]["median"] / us["plain"]["median"], 3)}
    return {"launch": dict(res, n_fft=n_fft, bins=512, B=B, calls=args.calls, windows=args.windows)}


def part_step(args, dev):
    cfg = dict(bench.CONFIGS["cfg2"])
    n_fft, B, C_ = cfg["n_fft"], cfg["B"], cfg["C"]
    assert cfg["din"] == 2 and cfg["ntemp"] == 1
    classes = [i % C_ for i in range(args.clips)]
    clips = [torch.from_numpy(bench.synth_clip(i, c)).to(dev) for i, c in enumerate(classes)]
    base = dict(drop_nyquist=True, jitter=n_fft // 4, gain_db=6.0,
                win_lengths=(n_fft, n_fft // 2, 3 * n_fft // 4), seed=1, device=dev)

    def make(reassign):
        ds = dataset.ESC_wave_pc(clips, classes, bench.FS, n_fft, reassign=reassign, **base)
        assert ds.num_points == 512
        torch.manual_seed(1)
        net = models.ST(dim_input=2, num_outputs=1, dim_output=C_, num_inds=cfg["m"],
                        dim_hidden=cfg["d"], num_heads=cfg["h"]).to(dev)
        return trainer.Trainer(net, ds, B, lr=1e-3, weight_decay=1e-3, mode=_lib.MODE_BF16, seed=1)

    runs = {"grid": make(None), "reassigned": make(True)}
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
    return {"step": {"ms_per_step": {k: _summary(v) for k, v in ms.items()}, "B": B, "steps": args.steps,
                     "windows": args.windows}}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--parts", default="launch,step")
    ap.add_argument("--calls", type=int, default=200)
    ap.add_argument("--windows", type=int, default=9)
    ap.add_argument("--steps", type=int, default=500)
    ap.add_argument("--warmup", type=int, default=100)
    ap.add_argument("--clips", type=int, default=48)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    dev = torch.device("cuda", 0)
    parts = dict(launch=part_launch, step=part_step)
    for name in args.parts.split(","):
        line = json.dumps(parts[name](args, dev))
        print(line, flush=True)
        if args.out:
            with open(args.out, "a") as f:
                f.write(line + "\n")


if __name__ == "__main__":
    main()
