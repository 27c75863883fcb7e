"""Cost of the speed change and the background mix of dataset.ESC_wave_pc (k_frame_points_ex) beside the
framed step without them (k_frame_points), at scripts/frame_bench.py's shape and with its timing: cfg2 -
B = 128 sets of N = 512 points (n_fft = 1024, Nyquist bin dropped), d = 128, bf16, one GPU, hipGraph replay,
the synthetic corpus of bench.build_dataset; wall time of a window of --steps replays between two device
syncs, the Trainers taking their windows in turn (A B C D E A B ...) so that drift falls on all alike:

    wave_off    ESC_wave_pc, every augmentation off              (frame_bench.py's case (ii): k_frame_points)
    wave_aug    jitter + gain + three window lengths             (its case (iii): k_frame_points)
    aug_speed   wave_aug + speeds (1.0, 0.9, 1.1)                (k_frame_points_ex)
    aug_mix     wave_aug + mix_clips="self", mix_prob 0.5, SNR 0 .. 20 dB
    aug_both    wave_aug + both

and, by device events over launches back to back, the launch alone for one batch: pca_frame_points against
pca_frame_points_ex with everything the latter adds switched off, then with speed, mix and both on.

    python scripts/frame_aug_bench.py [--steps 200] [--windows 15]
    rocprofv3 --kernel-trace --stats -d OUT -- python scripts/frame_aug_bench.py --profile --runs wave_aug,aug_both
        (one short window per Trainer named in --runs and nothing else: with one k_frame_points Trainer and
         one k_frame_points_ex Trainer, OUT's kernel statistics hold each kernel's time for that case)
"""
import argparse
import os
import statistics
import sys
import time

os.environ["PCA_PACK_DEFER"] = "0"
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "point-cloud-audio_amd")]
import torch

import bench
import dataset
import models
import pca_hip
from pca_hip import _lib, trainer


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=50)
    ap.add_argument("--windows", type=int, default=15)
    ap.add_argument("--clips", type=int, default=48)
    ap.add_argument("--profile", action="store_true",
                    help="one window per Trainer and no launches of their own, for a kernel trace")
    ap.add_argument("--runs", default="wave_off,wave_aug,aug_speed,aug_mix,aug_both",
                    help="the Trainers to time, comma-separated")
    args = ap.parse_args()
    if args.profile:
        args.windows = 1
    dev = torch.device("cuda", 0)
    cfg = dict(bench.CONFIGS["cfg2"])
    n_fft, B, C_ = cfg["n_fft"], cfg["B"], cfg["C"]
    assert cfg["din"] == 2 and cfg["ntemp"] == 1
    hop = n_fft // 2

    classes = [i % C_ for i in range(args.clips)]
    clips = [torch.from_numpy(bench.synth_clip(i, c)).to(dev) for i, c in enumerate(classes)]
    base = dict(drop_nyquist=True, jitter=hop // 2, gain_db=6.0,
                win_lengths=(n_fft, n_fft // 2, 3 * n_fft // 4), seed=1, device=dev)
    speed = dict(speeds=(1.0, 0.9, 1.1))
    mix = dict(mix_clips="self", mix_prob=0.5, mix_snr_db=(0.0, 20.0))
    sets = {"wave_aug": dataset.ESC_wave_pc(clips, classes, bench.FS, n_fft, **base),
            "aug_speed": dataset.ESC_wave_pc(clips, classes, bench.FS, n_fft, **base, **speed),
            "aug_mix": dataset.ESC_wave_pc(clips, classes, bench.FS, n_fft, **base, **mix),
            "aug_both": dataset.ESC_wave_pc(clips, classes, bench.FS, n_fft, **base, **speed, **mix)}
    sets = {"wave_off": sets["wave_aug"].plain(), **sets}
    assert sets["wave_off"].num_points == 512

    def make(ds):
        torch.manual_seed(1)
        net = models.ST(dim_input=2, num_outputs=1, dim_output=C_, num_inds=cfg["m"],
                        dim_hidden=cfg["d"], num_heads=cfg["h"]).to(dev)
        return trainer.Trainer(net, ds, B, lr=1e-3, weight_decay=1e-3, mode=_lib.MODE_BF16, seed=1)

    runs = {name: make(sets[name]) for name in args.runs.split(",")}
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

    print(f"cfg2 bf16 B={B} N=512 n_fft={n_fft}, {args.clips} clips, {len(sets['wave_off'])} sets: "
          f"{args.windows} windows of {args.steps} steps each")
    med = {}
    for name, w in ms.items():
        med[name] = statistics.median(w)
        print(f"  {name:<9}: median {med[name]:.4f} ms/step  (min {min(w):.4f}, max {max(w):.4f})")
    for name in ("aug_speed", "aug_mix", "aug_both"):
        if name in med and "wave_aug" in med:
            print(f"  {name} - wave_aug: {(med[name] - med['wave_aug']) * 1e3:+.1f} us")
    for tr in runs.values():
        loss, _ = tr.read_stats()
        assert loss == loss, "non-finite training loss"
    if args.profile:
        return

    # the launch alone, one batch of B sets spread over the corpus
    ds = sets["aug_both"]
    waves, woff, soff, f32, t32, lab = ds._resident()
    rms, bg, boff, brms, bmax = ds._mix_resident()
    idx = (torch.arange(B, device=dev) * 161) % len(ds)
    out = torch.empty((B, ds.num_points, 2), dtype=torch.float32, device=dev)
    lout = torch.empty(B, dtype=torch.int64, device=dev)
    a = (waves, woff, soff, idx, n_fft, hop, ds.F, f32, t32, 1)
    kw = dict(max_len=ds._max_len, min_len=ds._min_len, clip_labels=lab, jitter=ds.jitter,
              gain_db=ds.gain_db, win_lengths=ds._win_dev(dev), seed=1, draw=3, out=out, labels_out=lout)
    kmix = dict(clip_rms=rms, bg_waves=bg, bg_off=boff, bg_rms=brms, bg_max_len=bmax, mix_prob=0.5,
                mix_snr_db=(0.0, 20.0))
    calls = {"frame_points": lambda: pca_hip.frame_points(*a, **kw),
             "frame_points_ex, all off": lambda: pca_hip.frame_points_ex(*a, **kw),
             "frame_points_ex, speed": lambda: pca_hip.frame_points_ex(*a, ratios=ds.ratios, **kw),
             "frame_points_ex, mix": lambda: pca_hip.frame_points_ex(*a, **kmix, **kw),
             "frame_points_ex, both": lambda: pca_hip.frame_points_ex(*a, ratios=ds.ratios, **kmix, **kw)}
    want = calls["frame_points"]()[0].clone()
    assert torch.equal(calls["frame_points_ex, all off"]()[0], want), "ex with all off is not frame_points"
    reps = 200
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    us = {k: [] for k in calls}
    for fn in calls.values():
        for _ in range(20):
            fn()
    for _ in range(max(3, args.windows // 3)):
        for name, fn in calls.items():
            e0.record()
            for _ in range(reps):
                fn()
            e1.record()
            torch.cuda.synchronize(dev)
            us[name].append(e0.elapsed_time(e1) / reps * 1e3)

    print(f"  one launch for {B} frames of {n_fft} ({reps} launches back to back, device events, launch gaps "
          "and the host's argument set-up included):")
    for name, w in us.items():
        print(f"    {name:<26}: median {statistics.median(w):.1f} us  (min {min(w):.1f}, max {max(w):.1f})")


if __name__ == "__main__":
    main()
