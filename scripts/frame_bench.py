"""Cost of framing the training batch from the resident waveforms (dataset.ESC_wave_pc, k_frame_points)
against packing it from a resident spectrogram (dataset.ESC_pc, k_pack), at bench.py's cfg2 shape: B = 128
sets of N = 512 points (n_fft = 1024, Nyquist bin dropped), d = 128, bf16, one GPU, the synthetic corpus of
bench.build_dataset.

Per train step, bench.py's timing (wall time of a window of --steps graph replays between two device
syncs), the Trainers taking their windows in turn (A B C D A B ...) so that drift falls on all alike:

    pc_cursor   ESC_pc, device cursor, PCA_PACK_DEFER=0: k_pack as a launch of its own
    pc_plain    ESC_pc without batch_seq: an index batch uploaded per step, then k_pack - the step form
                a dataset that draws per call has, so the one the next two compare with
    wave_off    ESC_wave_pc, every augmentation off
    wave_aug    ESC_wave_pc, jitter + gain + three window lengths

and, by device events, k_stft_logmag over one clip of exactly B frames: what the transform itself costs
for a batch, the floor of wave_* - pc_plain without a faster FFT.

    python scripts/frame_bench.py [--steps 200] [--windows 15]
    rocprofv3 --kernel-trace --stats -d OUT -- python scripts/frame_bench.py --profile
        (one short window per Trainer: k_frame_points against k_pack in OUT's kernel statistics)
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


class PlainIndexPC(dataset.ESC_pc):
    batch_seq = None            # the Trainer then uploads an index batch per step and calls batch()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=50)
    ap.add_argument("--windows", type=int, default=15)
    ap.add_argument("--clips", type=int, default=48)
    ap.add_argument("--profile", action="store_true", help="one window per Trainer, for a kernel trace")
    args = ap.parse_args()
    if args.profile:
        args.windows = 1
    dev = torch.device("cuda", 0)
    cfg = dict(bench.CONFIGS["cfg2"])
    n_fft, B, C_ = cfg["n_fft"], cfg["B"], cfg["C"]
    assert cfg["din"] == 2 and cfg["ntemp"] == 1
    hop = n_fft // 2

    pc, _ = bench.build_dataset(cfg, args.clips, dev, seed=0)
    spec_tf, _, lab = pc._resident()
    plain = PlainIndexPC.from_device(spec_tf, lab, pc.farr)
    # the same clips (bench.build_dataset, seed 0) as waveforms
    classes = [i % C_ for i in range(args.clips)]
    clips = [torch.from_numpy(bench.synth_clip(i, c)).to(dev) for i, c in enumerate(classes)]
    aug = dataset.ESC_wave_pc(clips, classes, bench.FS, n_fft, drop_nyquist=True, jitter=hop // 2,
                              gain_db=6.0, win_lengths=(n_fft, n_fft // 2, 3 * n_fft // 4), seed=1,
                              device=dev)
    off = aug.plain()
    assert len(off) == len(pc) and off.num_points == pc.num_points == 512
    ids = torch.arange(0, len(pc), 97, device=dev)
    assert torch.equal(off.batch(ids)[0], pc.batch(ids)[0]), "wave_off is not the spectrogram pipeline"

    def make(ds):
        torch.manual_seed(1)
        net = models.ST(dim_input=2, num_outputs=1, dim_output=C_, num_inds=cfg["m"],
                        dim_hidden=cfg["d"], num_heads=cfg["h"]).to(dev)
        return trainer.Trainer(net, ds, B, lr=1e-3, weight_decay=1e-3, mode=_lib.MODE_BF16, seed=1)

    runs = {"pc_cursor": make(pc), "pc_plain": make(plain), "wave_off": make(off), "wave_aug": make(aug)}
    assert runs["pc_cursor"]._cursor_mode and not runs["pc_plain"]._cursor_mode
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

    # the transform alone: one clip that yields exactly B frames
    wave = clips[0][:(B - 1) * hop]
    assert 1 + wave.numel() // hop == B
    for _ in range(20):
        pca_hip.stft_logmag(wave, n_fft, n_fft, hop, drop_nyquist=True, frame_major=True)
    reps = 200
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    stft_us = []
    for _ in range(max(3, args.windows // 3)):
        e0.record()
        for _ in range(reps):
            pca_hip.stft_logmag(wave, n_fft, n_fft, hop, drop_nyquist=True, frame_major=True)
        e1.record()
        torch.cuda.synchronize(dev)
        stft_us.append(e0.elapsed_time(e1) / reps * 1e3)

    print(f"cfg2 bf16 B={B} N=512 n_fft={n_fft}, {args.clips} clips, {len(pc)} sets: "
          f"{args.windows} windows of {args.steps} steps each")
    med = {}
    for name, w in ms.items():
        med[name] = statistics.median(w)
        print(f"  {name:<9}: median {med[name]:.4f} ms/step  (min {min(w):.4f}, max {max(w):.4f})")
    for name in ("wave_off", "wave_aug"):
        print(f"  {name} - pc_plain: {(med[name] - med['pc_plain']) * 1e3:+.1f} us")
    print(f"  k_stft_logmag, {B} frames ({reps} launches back to back, device events): "
          f"median {statistics.median(stft_us):.1f} us  (min {min(stft_us):.1f}, max {max(stft_us):.1f})")
    for tr in runs.values():
        loss, _ = tr.read_stats()
        assert loss == loss, "non-finite training loss"


if __name__ == "__main__":
    main()
