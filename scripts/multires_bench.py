"""What multi-resolution point sets cost on one MI355X: the launch and the training step.

    python scripts/multires_bench.py [--parts launch,step] [--out FILE]

  launch  pca_frame_points_multires beside what a caller could do without it - one pca_frame_points per level
          into separate buffers, then torch.cat into the batch - in the same run, on the same resident corpus,
          the same batch and the same draws, B = 128, din = 3, jitter and gain on:
            512pt   (n_fft 512, hop 256, Nt 1) + (n_fft 256, hop 128, Nt 2) at span 256:  512 points a set
            2048pt  (1024, 512, 2) + (256, 128, 8) at span 1024:                         2048 points a set
          Both sides run the same transforms; the single launch skips the batch's round trip through HBM, and
          its small-n_fft workgroups reserve the LDS of the largest level.  scripts/peak_bench.py's timing:
          --calls calls captured into one hipGraph (the device's time, not the host's launch rate), a replay
          between two HIP events, the two sides taking their replays in turn, median and min - max of
          --windows replays.  The two sides' batches are compared bit for bit.
  step    the training step at d = 128, 4 heads, 16 inducing points, bf16, B = 128, hipGraph replay, over
          dataset.ESC_wave_pc_multires (the 512pt levels) and over dataset.ESC_wave_pc_temp sets of 512 points
          (n_fft 256, Ntemp 4), both with jitter, gain and two window lengths: wall time of windows of --steps
          replays between two device syncs, the Trainers in turn.
Prints one JSON line per part (and appends them to --out)."""
import argparse
import json
import os
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

CONFIGS = {"512pt": (256, [dict(n_fft=512, hop=256, Ntemp=1), dict(n_fft=256, hop=128, Ntemp=2)]),
           "2048pt": (1024, [dict(n_fft=1024, hop=512, Ntemp=2), dict(n_fft=256, hop=128, Ntemp=8)])}


def _corpus(args, dev, n_classes=10):
    classes = [i % n_classes for i in range(args.clips)]
    return [torch.from_numpy(bench.synth_clip(i, c)).to(dev) for i, c in enumerate(classes)], classes


def part_launch(args, dev):
    B = 128
    clips, classes = _corpus(args, dev)
    res = {}
    for name, (span, levels) in CONFIGS.items():
        ds = dataset.ESC_wave_pc_multires(clips, classes, bench.FS, levels, span, jitter=span // 4, gain_db=6.0,
                                          seed=1, device=dev)
        N = ds.num_points
        assert len(ds) >= B and N == int(name[:-2])
        waves, woff, soff, lab = ds._resident()
        lv = ds._levels_dev(dev)
        assert all(l.Nt * l.hop == span and l.offset == 0 for l in lv)   # the plain launch cuts the same frames
        g = torch.Generator(device="cpu").manual_seed(span)
        idx = torch.randint(0, len(ds), (B,), generator=g).to(dev)
        one = torch.empty((B, N, 3), device=dev)
        cat = torch.empty((B, N, 3), device=dev)
        parts = [torch.empty((B, l.Nt * l.n_bins, 3), device=dev) for l in lv]
        lab_out = torch.empty(B, dtype=torch.int64, device=dev)
        common = dict(max_len=ds._max_len, min_len=ds._min_len, clip_labels=lab, jitter=ds.jitter,
                      gain_db=ds.gain_db, seed=1, draw=1, labels_out=lab_out)

        def single():
            pca_hip.frame_points_multires(waves, woff, soff, idx, lv, span, out=one, **common)

        def separate():
            for l, buf in zip(lv, parts):
                pca_hip.frame_points(waves, woff, soff, idx, l.n_fft, l.hop, l.n_bins, l.farr, l.tarr, l.Nt,
                                     win_lengths=l.win_lengths, out=buf, **common)
            torch.cat(parts, dim=1, out=cat)

        us = _event_windows({"single": single, "separate_cat": separate}, args.calls, args.windows, dev)
        assert torch.equal(one.view(torch.int32), cat.view(torch.int32))
        res[name] = {"us_per_call": us, "points": N, "frames": B * sum(l.Nt for l in lv),
                     "ratio": round(us["single"]["median"] / us["separate_cat"]["median"], 3)}
    return {"launch": dict(res, B=B, calls=args.calls, windows=args.windows)}


def part_step(args, dev):
    B, C_ = 128, 50
    clips, classes = _corpus(args, dev, C_)
    span, levels = CONFIGS["512pt"]
    levels = [dict(l, win_lengths=(l["n_fft"], 3 * l["n_fft"] // 4)) for l in levels]

    def make(kind):
        if kind == "multires":
            ds = dataset.ESC_wave_pc_multires(clips, classes, bench.FS, levels, span, jitter=64, gain_db=6.0,
                                              seed=1, device=dev)
        else:
            ds = dataset.ESC_wave_pc_temp(clips, classes, bench.FS, 256, 4, jitter=64, gain_db=6.0,
                                          win_lengths=(256, 192), seed=1, device=dev)
        assert ds.num_points == 512
        torch.manual_seed(1)
        net = models.ST(dim_input=3, num_outputs=1, dim_output=C_, num_inds=16, dim_hidden=128,
                        num_heads=4).to(dev)
        return trainer.Trainer(net, ds, B, lr=1e-3, weight_decay=1e-3, mode=_lib.MODE_BF16, seed=1)

    runs = {"temp_512": make("temp"), "multires_512": make("multires")}
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
    out = {k: _summary(v) for k, v in ms.items()}
    return {"step": {"ms_per_step": out, "B": B, "steps": args.steps, "windows": args.windows,
                     "ratio": round(out["multires_512"]["median"] / out["temp_512"]["median"], 3)}}


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
