"""What PCEN point sets cost on one MI355X: the launch and the training step.

    python scripts/pcen_bench.py [--parts launch,step] [--out FILE]

  launch  pca_frame_points_pcen beside the band launch and beside what a caller could do without it, in the same
          run, on the same resident corpus and batch, B = 128, jitter and gain on, n_fft 1024, hop 512, 64
          Slaney mel bands x Nt = 8 frames = 512 points a set, for a context of W = 0, 8 and 32 frames:
          (a) pcen         one pca_frame_points_pcen launch, grid (W + 8, 128)
          (b) bands        one pca_frame_points_bands launch at the same shape, grid (8, 128): the log-mel set
          (c) bands_torch  one pca_frame_points_bands launch over W + 8 frames a set, then the chain a caller
                           would write on its batch: exp -> the smoother, a Python loop over the W + 8 frames
                           -> pow -> the last 8 frames stacked with the band axes
          scripts/peak_bench.py's timing: --calls calls captured into one hipGraph (the device's time, not the
          host's launch rate), a replay between two HIP events, the sides taking their replays in turn, median
          and min - max of --windows replays.  (a) and (c) are compared once with the augmentation off, on sets
          that cover the same frames; the largest difference, relative to the largest value, is reported
          (the chain undoes the band launch's log in fp32) and a gross mismatch (5e-2) stops the run.
  step    the training step at d = 128, 4 heads, 16 inducing points, bf16, B = 128, hipGraph replay, over
          dataset.ESC_wave_pc_temp(n_fft 1024, Ntemp 8, bands = 64 mel) with pcen = Pcen() (32 frames of context)
          and without (log-mel), both with jitter, gain and two window lengths: wall time of windows of --steps
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
import numpy as np
import torch

import bench
import dataset
import models
import pca_hip
from pca_hip import _lib, trainer
from peak_bench import _event_windows, _summary

N_FFT, N_MELS, NT = 1024, 64, 8
CONTEXTS = (0, 8, 32)


def _corpus(args, dev, n_classes=10):
    classes = [i % n_classes for i in range(args.clips)]
    return [torch.from_numpy(bench.synth_clip(i, c)).to(dev) for i, c in enumerate(classes)], classes


def part_launch(args, dev):
    B, hop = 128, N_FFT // 2
    clips, classes = _corpus(args, dev)
    bank = pca_hip.mel_bank(bench.FS, N_FFT, N_MELS)
    ds = dataset.ESC_wave_pc_temp(clips, classes, bench.FS, N_FFT, NT, jitter=N_FFT // 8, gain_db=6.0, seed=1,
                                  device=dev, bands=bank)
    assert len(ds) >= B and ds.num_points == NT * N_MELS
    waves, woff, soff, _, t32, lab = ds._resident()
    f_band, wins = ds._bands_farr(dev), ds._win_dev(dev)
    lens = [int(c.shape[0]) for c in clips]
    lab_out = torch.empty(B, dtype=torch.int64, device=dev)
    common = dict(max_len=ds._max_len, min_len=ds._min_len, clip_labels=lab, win_lengths=wins, seed=1, draw=1,
                  labels_out=lab_out)
    aug = dict(jitter=ds.jitter, gain_db=ds.gain_db)
    res = {}
    for W in CONTEXTS:
        T = W + NT
        spec = pca_hip.Pcen(context=W)
        s = spec.coefficient(bench.FS, hop)
        # the long sets of (c), and the sets of (a) / (b) that end where they end
        long_off = dataset.wave_set_offsets(lens, hop, T)
        g = torch.Generator(device="cpu").manual_seed(W)
        idx_long = torch.randint(0, long_off[-1], (B,), generator=g).numpy()
        clip = np.searchsorted(np.asarray(long_off), idx_long, side="right") - 1
        idx_np = np.asarray(ds.set_off)[clip] + (idx_long - np.asarray(long_off)[clip]) * (T // NT) + W // NT
        assert T % NT == 0 and (idx_np < np.asarray(ds.set_off)[clip + 1]).all()
        idx, idx_long = torch.from_numpy(idx_np).to(dev), torch.from_numpy(idx_long).to(dev)
        soff_long = torch.as_tensor(np.asarray(long_off, dtype=np.int64)).to(dev)
        t_long = torch.linspace(0, 1, T, device=dev)
        out_a = torch.empty((B, NT * N_MELS, 3), device=dev)
        out_b = torch.empty((B, NT * N_MELS, 3), device=dev)
        out_c = torch.empty((B, NT * N_MELS, 3), device=dev)
        long = torch.empty((B, T * N_MELS, 3), device=dev)
        coords = out_c.view(B, NT, N_MELS, 3)
        floor_r = spec.bias ** spec.power

        def pcen(kw=aug):
            pca_hip.frame_points_pcen(waves, woff, soff, idx, N_FFT, hop, bank, f_band, t32, NT, pcen=spec,
                                      fs=bench.FS, out=out_a, **common, **kw)

        def bands(kw=aug):
            pca_hip.frame_points_bands(waves, woff, soff, idx, N_FFT, hop, bank, f_band, t32, NT, out=out_b,
                                       **common, **kw)

        def bands_torch(kw=aug):
            pca_hip.frame_points_bands(waves, woff, soff_long, idx_long, N_FFT, hop, bank, f_band, t_long, T,
                                       out=long, **common, **kw)
            x = (torch.exp(long.view(B, T, N_MELS, 3)[..., -1]) - bank.amin) * spec.scale
            M, ys = x[:, 0], []
            for u in range(T):                                     # the smoother is a recursion
                if u:
                    M = (1.0 - s) * M + s * x[:, u]
                if u >= W:
                    ys.append(torch.pow(spec.bias + x[:, u] * torch.exp(-spec.gain * torch.log(spec.eps + M)),
                                        spec.power) - floor_r)
            val = torch.stack(ys, dim=1)                           # [B, NT, n_mels]
            torch.stack([f_band.expand(B, NT, N_MELS), t32[:NT, None].expand(B, NT, N_MELS), val], dim=-1,
                        out=coords)

        pcen({})
        bands_torch({})
        torch.cuda.synchronize(dev)
        err = float((out_a[..., -1] - out_c[..., -1]).abs().max() / out_a[..., -1].abs().max())
        assert torch.equal(out_a[..., :-1], out_c[..., :-1]) and err < 5e-2, err
        us = _event_windows({"pcen": pcen, "bands": bands, "bands_torch": bands_torch}, args.calls,
                            args.windows, dev)
        res[f"W{W}"] = {"us_per_call": us, "frames_per_set": T, "points": NT * N_MELS, "s": round(s, 5),
                        "max_rel_diff_pcen_vs_chain": err,
                        "pcen_over_bands": round(us["pcen"]["median"] / us["bands"]["median"], 3),
                        "expected_(W+Nt)/Nt": round(T / NT, 3),
                        "pcen_over_bands_torch": round(us["pcen"]["median"] / us["bands_torch"]["median"], 3)}
    return {"launch": dict(res, B=B, n_fft=N_FFT, n_mels=N_MELS, Nt=NT, calls=args.calls, windows=args.windows)}


def part_step(args, dev):
    B, C_ = 128, 50
    clips, classes = _corpus(args, dev, C_)

    def make(spec):
        ds = dataset.ESC_wave_pc_temp(clips, classes, bench.FS, N_FFT, NT, jitter=64, gain_db=6.0,
                                      win_lengths=(N_FFT, N_FFT * 3 // 4), seed=1, device=dev,
                                      bands=pca_hip.mel_bank(bench.FS, N_FFT, N_MELS), pcen=spec)
        assert ds.num_points == 512 and len(ds) >= B
        torch.manual_seed(1)
        net = models.ST(dim_input=3, num_outputs=1, dim_output=C_, num_inds=16, dim_hidden=128,
                        num_heads=4).to(dev)
        return trainer.Trainer(net, ds, B, lr=1e-3, weight_decay=1e-3, mode=_lib.MODE_BF16, seed=1)

    runs = {"logmel_512": make(None), "pcen_512": make(pca_hip.Pcen())}
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
    return {"step": {"ms_per_step": out, "B": B, "steps": args.steps, "windows": args.windows, "context": 32,
                     "ratio": round(out["pcen_512"]["median"] / out["logmel_512"]["median"], 3)}}


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
