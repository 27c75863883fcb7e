"""Cost of the point masks of dataset.ESC_wave_pc (frequency bands drawn and removed inside the frame
launch) on the training step, at scripts/frame_aug_bench.py's shape and with its timing: cfg2 - B = 128 sets
of N = 512 points (n_fft = 1024, Nyquist bin dropped; one frame per set, so bands only), d = 128, bf16, one
GPU, hipGraph replay, the synthetic corpus of bench.build_dataset; wall time of a window of --steps replays
between two device syncs, the Trainers taking their windows in turn (A B C A B ...) so that drift falls on
all alike:

    off      jitter + gain + three window lengths, no mask     (k_frame_points, the dense step)
    floor    off + 2 bands of up to 64 bins, mask_mode="floor"  (k_frame_points_ex, the dense step)
    drop     off + the same bands, mask_mode="drop"             (k_frame_points_ex, the step with lengths)

    python scripts/mask_bench.py [--steps 1000] [--windows 9] [--runs off,floor,drop]

``--runs off`` builds nothing the masks added, so the same file times a tree from before them: run the two
trees in turn in one session to compare "off" with the parent.
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
from pca_hip import _lib, trainer

MASK = dict(freq_masks=2, freq_mask_width=64)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=1000)
    ap.add_argument("--warmup", type=int, default=100)
    ap.add_argument("--windows", type=int, default=9)
    ap.add_argument("--clips", type=int, default=48)
    ap.add_argument("--runs", default="off,floor,drop", help="the Trainers to time, comma-separated")
    args = ap.parse_args()
    dev = torch.device("cuda", 0)
    cfg = dict(bench.CONFIGS["cfg2"])
    n_fft, B, C_ = cfg["n_fft"], cfg["B"], cfg["C"]
    assert cfg["din"] == 2 and cfg["ntemp"] == 1
    hop = n_fft // 2

    classes = [i % C_ for i in range(args.clips)]
    clips = [torch.from_numpy(bench.synth_clip(i, c)).to(dev) for i, c in enumerate(classes)]
    base = dict(drop_nyquist=True, jitter=hop // 2, gain_db=6.0,
                win_lengths=(n_fft, n_fft // 2, 3 * n_fft // 4), seed=1, device=dev)
    extra = {"off": {}, "floor": dict(MASK, mask_mode="floor"), "drop": dict(MASK, mask_mode="drop")}

    def make(name):
        ds = dataset.ESC_wave_pc(clips, classes, bench.FS, n_fft, **base, **extra[name])
        assert ds.num_points == 512
        torch.manual_seed(1)
        net = models.ST(dim_input=2, num_outputs=1, dim_output=C_, num_inds=cfg["m"],
                        dim_hidden=cfg["d"], num_heads=cfg["h"]).to(dev)
        return trainer.Trainer(net, ds, B, lr=1e-3, weight_decay=1e-3, mode=_lib.MODE_BF16, seed=1)

    runs = {name: make(name) for name in args.runs.split(",")}
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

    print(f"cfg2 bf16 B={B} N=512 n_fft={n_fft}, {args.clips} clips: {args.windows} windows of {args.steps} "
          f"steps each")
    med = {}
    for name, w in ms.items():
        med[name] = statistics.median(w)
        print(f"  {name:<6}: median {med[name]:.4f} ms/step  (min {min(w):.4f}, max {max(w):.4f})")
    for name in ("floor", "drop"):
        if name in med and "off" in med:
            print(f"  {name} / off: {med[name] / med['off']:.3f}  ({(med[name] - med['off']) * 1e3:+.1f} us)")
    for name, tr in runs.items():
        loss, _ = tr.read_stats()
        assert loss == loss, f"non-finite training loss ({name})"
        if name == "drop":
            ln = tr.lengths.float()
            print(f"  drop: {ln.mean().item():.1f} of 512 points kept per set on the last step "
                  f"(min {int(ln.min())}, max {int(ln.max())})")


if __name__ == "__main__":
    main()
