"""What delta point sets cost on one MI355X: the launch and the training step.

    python scripts/delta_bench.py [--parts mel,grid,step] [--out FILE]

  mel     pca_frame_points_delta (axes "t") beside the band launch, in the same run, on the same resident corpus
          and batch, B = 128, jitter and gain on, n_fft 1024, hop 512, 64 Slaney mel bands x Nt = 8 frames = 512
          points a set, for a width of W = 1, 2 and 4:
          (a) delta   one pca_frame_points_delta launch, grid (8 + 2 W, 128), rows (f, t, v, dt)
          (b) base    one pca_frame_points_bands launch at the same arguments, grid (8, 128), rows (f, t, v)
          The value column of (a) must be (b)'s bits, or the run stops.
  grid    the same on the grid: n_fft 512, hop 256, 256 bins (the Nyquist bin dropped) x Nt = 8 frames = 2048
          points a set, beside pca_frame_points.
          scripts/peak_bench.py's timing: --calls calls captured into one hipGraph (the device's time, not the
          host's launch rate), a replay between two HIP events, the sides taking their replays in turn, median
          and min - max of --windows replays.  Every width reports its ratio to the base launch beside the ratio
          of the frames transformed, (Nt + 2 W) / Nt.
  step    the training step at d = 128, 4 heads, 16 inducing points, bf16, B = 128, hipGraph replay, over
          dataset.ESC_wave_pc_temp(n_fft 1024, Ntemp 8, bands = 64 mel): N = 512 sets at din 4 with
          deltas = Deltas("t", 2), beside the same sets without the column (din 3), both with jitter, gain and two
          window lengths: wall time of windows of --steps replays between two device syncs, the Trainers in turn.
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

NT = 8
WIDTHS = (1, 2, 4)


def _corpus(args, dev, n_classes=10):
    classes = [i % n_classes for i in range(args.clips)]
    return [torch.from_numpy(bench.synth_clip(i, c)).to(dev) for i, c in enumerate(classes)], classes


def _launch(args, dev, n_fft, bank):
    """The delta launch for every width beside its base launch, on one dataset's resident corpus."""
    B, hop = 128, n_fft // 2
    clips, classes = _corpus(args, dev)
    ds = dataset.ESC_wave_pc_temp(clips, classes, bench.FS, n_fft, NT, jitter=n_fft // 8, gain_db=6.0, seed=1,
                                  device=dev, bands=bank)
    F = ds.F
    assert len(ds) >= B and ds.num_points == NT * F
    waves, woff, soff, f32, t32, lab = ds._resident()
    farr = f32 if bank is None else ds._bands_farr(dev)
    lab_out = torch.empty(B, dtype=torch.int64, device=dev)
    common = dict(max_len=ds._max_len, min_len=ds._min_len, clip_labels=lab, win_lengths=ds._win_dev(dev), seed=1,
                  draw=1, labels_out=lab_out, jitter=ds.jitter, gain_db=ds.gain_db)
    g = torch.Generator(device="cpu").manual_seed(3)
    idx = torch.randint(0, len(ds), (B,), generator=g).to(dev)
    out_b = torch.empty((B, NT * F, 3), device=dev)

    def base():
        if bank is None:
            pca_hip.frame_points(waves, woff, soff, idx, n_fft, hop, F, farr, t32, NT, out=out_b, **common)
        else:
            pca_hip.frame_points_bands(waves, woff, soff, idx, n_fft, hop, bank, farr, t32, NT, out=out_b, **common)

    res = {}
    for W in WIDTHS:
        spec = pca_hip.Deltas("t", W)
        T = NT + 2 * W
        out_a = torch.empty((B, NT * F, 4), device=dev)
        ws = (torch.empty((B, T, F), dtype=torch.float32, device=dev),
              torch.zeros(B, dtype=torch.int32, device=dev))

        def delta():
            pca_hip.frame_points_delta(waves, woff, soff, idx, n_fft, hop, F, farr, t32, NT, deltas=spec, bank=bank,
                                       out=out_a, workspace=ws, **common)

        delta()
        base()
        torch.cuda.synchronize(dev)
        assert torch.equal(out_a[..., :3].contiguous().view(torch.int32), out_b.view(torch.int32))
        assert int(ws[1].abs().sum()) == 0 and bool(torch.isfinite(out_a).all())
        us = _event_windows({"delta": delta, "base": base}, args.calls, args.windows, dev)
        res[f"W{W}"] = {"us_per_call": us, "frames_per_set": T, "points": NT * F,
                        "delta_over_base": round(us["delta"]["median"] / us["base"]["median"], 3),
                        "expected_(Nt+2W)/Nt": round(T / NT, 3)}
    return dict(res, B=B, n_fft=n_fft, rows_per_frame=F, Nt=NT, calls=args.calls, windows=args.windows)


def part_mel(args, dev):
    return {"mel": _launch(args, dev, 1024, pca_hip.mel_bank(bench.FS, 1024, 64))}


def part_grid(args, dev):
    return {"grid": _launch(args, dev, 512, None)}


def part_step(args, dev):
    B, C_, n_fft = 128, 50, 1024
    clips, classes = _corpus(args, dev, C_)

    def make(spec):
        ds = dataset.ESC_wave_pc_temp(clips, classes, bench.FS, n_fft, NT, jitter=64, gain_db=6.0,
                                      win_lengths=(n_fft, n_fft * 3 // 4), seed=1, device=dev,
                                      bands=pca_hip.mel_bank(bench.FS, n_fft, 64), deltas=spec)
        assert ds.num_points == 512 and len(ds) >= B
        torch.manual_seed(1)
        net = models.ST(dim_input=ds.din, num_outputs=1, dim_output=C_, num_inds=16, dim_hidden=128,
                        num_heads=4).to(dev)
        return trainer.Trainer(net, ds, B, lr=1e-3, weight_decay=1e-3, mode=_lib.MODE_BF16, seed=1)

    runs = {"logmel_512_din3": make(None), "delta_512_din4": make(pca_hip.Deltas("t", 2))}
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
    return {"step": {"ms_per_step": out, "B": B, "steps": args.steps, "windows": args.windows, "width": 2,
                     "ratio": round(out["delta_512_din4"]["median"] / out["logmel_512_din3"]["median"], 3)}}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--parts", default="mel,grid,step")
    ap.add_argument("--calls", type=int, default=200)
    ap.add_argument("--windows", type=int, default=9)
    ap.add_argument("--steps", type=int, default=500)
    ap.add_argument("--warmup", type=int, default=100)
    ap.add_argument("--clips", type=int, default=48)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    dev = torch.device("cuda", 0)
    parts = dict(mel=part_mel, grid=part_grid, step=part_step)
    for name in args.parts.split(","):
        line = json.dumps(parts[name](args, dev))
        print(line, flush=True)
        if args.out:
            with open(args.out, "a") as f:
                f.write(line + "\n")


if __name__ == "__main__":
    main()
