"""What band (log-mel) point sets cost on one MI355X: the launch and the training step.

    python scripts/bands_bench.py [--parts launch,step] [--out FILE]

  launch  pca_frame_points_bands beside the plain launch and beside what a caller could do without it, in the
          same run, on the same resident corpus, the same batch and the same draws, B = 128, jitter and gain on:
            2048-128  n_fft 2048, hop 1024, Nt 1, 128 Slaney mel bands, 2-D rows:    128 points a set
            512-64x8  n_fft 512,  hop 256,  Nt 8, 64 Slaney mel bands,  3-D rows:    512 points a set
          (a) bands        one pca_frame_points_bands launch
          (b) plain        one pca_frame_points launch at the same n_fft, all n_fft/2 + 1 bins (the same FFTs,
                           8 / 4 times the rows)
          (c) plain_torch  (b), then the chain a caller would write on its batch: exp -> square -> matmul with
                           the dense bank -> log -> stack with the band axes
          scripts/peak_bench.py's timing: --calls calls captured into one hipGraph (the device's time, not the
          host's launch rate), a replay between two HIP events, the sides taking their replays in turn, median
          and min - max of --windows replays.  (a) and (c) are compared: the same values to 1e-3 (the chain
          undoes the plain launch's log in fp32).
  step    the training step at d = 128, 4 heads, 16 inducing points, bf16, B = 128, hipGraph replay, over
          dataset.ESC_wave_pc_temp(n_fft 512, Ntemp 8, bands = 64 mel) - 512 points a set - and over the dense
          512-point sets of ESC_wave_pc_temp(n_fft 256, Ntemp 4), both with jitter, gain and two window
          lengths: wall time of windows of --steps replays between two device syncs, the Trainers in turn.
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

CONFIGS = {"2048-128": (2048, 128, 1), "512-64x8": (512, 64, 8)}       # n_fft, n_mels, Nt


def _corpus(args, dev, n_classes=10):
    classes = [i % n_classes for i in range(args.clips)]
    return [torch.from_numpy(bench.synth_clip(i, c)).to(dev) for i, c in enumerate(classes)], classes


def part_launch(args, dev):
    B = 128
    clips, classes = _corpus(args, dev)
    res = {}
    for name, (n_fft, n_mels, Nt) in CONFIGS.items():
        bank = pca_hip.mel_bank(bench.FS, n_fft, n_mels)
        kw = dict(jitter=n_fft // 8, gain_db=6.0, seed=1, device=dev, bands=bank)
        ds = (dataset.ESC_wave_pc(clips, classes, bench.FS, n_fft, **kw) if Nt == 1
              else dataset.ESC_wave_pc_temp(clips, classes, bench.FS, n_fft, Nt, **kw))
        assert len(ds) >= B and ds.num_points == Nt * n_mels
        waves, woff, soff, _, t32, lab = ds._resident()
        din, hop, n_src = (2 if Nt == 1 else 3), ds.hop, n_fft // 2 + 1
        f_band = ds._bands_farr(dev)
        f_grid = torch.linspace(0, 0.5, n_src, device=dev)
        wins = ds._win_dev(dev)
        g = torch.Generator(device="cpu").manual_seed(n_fft)
        idx = torch.randint(0, len(ds), (B,), generator=g).to(dev)
        out_a = torch.empty((B, Nt * n_mels, din), device=dev)
        out_c = torch.empty((B, Nt * n_mels, din), device=dev)
        grid = torch.empty((B, Nt * n_src, din), device=dev)
        lab_out = torch.empty(B, dtype=torch.int64, device=dev)
        Wt = torch.from_numpy(bank.dense()).float().to(dev).t().contiguous()         # [n_src, n_mels]
        coords = out_c.view(B, Nt, n_mels, din)
        common = dict(max_len=ds._max_len, min_len=ds._min_len, clip_labels=lab, jitter=ds.jitter,
                      gain_db=ds.gain_db, win_lengths=wins, seed=1, draw=1, labels_out=lab_out)

        def bands():
            pca_hip.frame_points_bands(waves, woff, soff, idx, n_fft, hop, bank, f_band, t32, Nt, out=out_a,
                                       **common)

        def plain():
            pca_hip.frame_points(waves, woff, soff, idx, n_fft, hop, n_src, f_grid, t32, Nt, out=grid, **common)

        def plain_torch():
            plain()
            mag = torch.exp(grid.view(B, Nt, n_src, din)[..., -1]) - 1e-8
            val = torch.log(torch.matmul(mag * mag, Wt) + bank.amin)                 # [B, Nt, n_mels]
            cols = [f_band.expand(B, Nt, n_mels)]
            if Nt > 1:
                cols.append(t32[:Nt, None].expand(B, Nt, n_mels))
            torch.stack(cols + [val], dim=-1, out=coords)

        us = _event_windows({"bands": bands, "plain": plain, "plain_torch": plain_torch}, args.calls,
                            args.windows, dev)
        # the chain undoes a log in fp32, so near the floor it differs from the launch's fp64 sums
        loud = out_a[..., -1] > -12.0
        err = float((out_a[..., -1] - out_c[..., -1])[loud].abs().max())
        assert torch.equal(out_a[..., :-1], out_c[..., :-1]) and err < 1e-3, err
        res[name] = {"us_per_call": us, "points": Nt * n_mels, "frames": B * Nt, "nnz": bank.nnz,
                     "max_abs_diff_bands_vs_chain": err,
                     "bands_over_plain": round(us["bands"]["median"] / us["plain"]["median"], 3),
                     "bands_over_plain_torch": round(us["bands"]["median"] / us["plain_torch"]["median"], 3)}
    return {"launch": dict(res, B=B, calls=args.calls, windows=args.windows)}


def part_step(args, dev):
    B, C_ = 128, 50
    clips, classes = _corpus(args, dev, C_)

    def make(kind):
        if kind == "mel":
            ds = dataset.ESC_wave_pc_temp(clips, classes, bench.FS, 512, 8, jitter=64, gain_db=6.0,
                                          win_lengths=(512, 384), seed=1, device=dev,
                                          bands=pca_hip.mel_bank(bench.FS, 512, 64))
        else:
            ds = dataset.ESC_wave_pc_temp(clips, classes, bench.FS, 256, 4, jitter=64, gain_db=6.0,
                                          win_lengths=(256, 192), seed=1, device=dev)
        assert ds.num_points == 512 and len(ds) >= B
        torch.manual_seed(1)
        net = models.ST(dim_input=3, num_outputs=1, dim_output=C_, num_inds=16, dim_hidden=128,
                        num_heads=4).to(dev)
        return trainer.Trainer(net, ds, B, lr=1e-3, weight_decay=1e-3, mode=_lib.MODE_BF16, seed=1)

    runs = {"dense_512": make("dense"), "mel_512": make("mel")}
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
                     "ratio": round(out["mel_512"]["median"] / out["dense_512"]["median"], 3)}}


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
