"""Time of the clip-level aggregation (pca_clip_aggregate: k_clip_aggregate) on one GPU.

  python scripts/clip_bench.py [--clips 2000] [--frames 431] [--classes 50] [--windows 15] [--out FILE]

Logits: --clips clips of --frames frames each, N(0, 1) with 3 added on the clip's class, made on the
device.  The ESC-50-shaped [862000, 50] logits are 172 MB, less than the 256 MiB Infinity Cache, so the
calls of a window rotate over --copies buffers (default: enough for 1 GiB, at most 8) and every call
reads logits that have left the cache; a small case stays cache-resident, as it is right after the engine
wrote it.  Measured: the ABI call with all three outputs and the tally, as the median over
--windows HIP-event windows of --calls calls each (0: sized to about 20 ms) after a warm-up; next to it
the logits' bytes / 8 TB/s, the time HBM alone would take.  The predictions of the first buffer are
compared with torch's on the same logits (float64 log_softmax, mean, argmax; votes by bincount)."""
import argparse
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "point-cloud-audio_amd")]

HBM_PEAK = 8.0e12


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--clips", type=int, default=2000)
    ap.add_argument("--frames", type=int, default=431)
    ap.add_argument("--classes", type=int, default=50)
    ap.add_argument("--copies", type=int, default=0)
    ap.add_argument("--windows", type=int, default=15)
    ap.add_argument("--calls", type=int, default=0)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()

    import pca_hip
    from pca_hip import _lib

    assert torch.cuda.is_available(), "clip_bench needs a GPU"
    dev = torch.device("cuda", 0)
    L = pca_hip.lib()
    n_clips, T, C = args.clips, args.frames, args.classes
    n_sets = n_clips * T
    nbytes = 4.0 * n_sets * C
    copies = args.copies if args.copies > 0 else min(8, max(1, int(np.ceil(2 ** 30 / nbytes))))
    g = torch.Generator(device=dev).manual_seed(0)
    own = torch.randint(0, C, (n_clips,), generator=g, device=dev)
    bufs = []
    for _ in range(copies):
        x = torch.randn((n_sets, C), generator=g, device=dev)
        x.view(n_clips, T, C).scatter_add_(2, own.view(-1, 1, 1).expand(-1, T, 1),
                                           torch.full((n_clips, T, 1), 3.0, device=dev))
        bufs.append(x)
    off = torch.arange(0, n_sets + 1, T, dtype=torch.int64, device=dev)
    mean = torch.empty((n_clips, C), dtype=torch.float32, device=dev)
    votes = torch.empty((n_clips, C), dtype=torch.int32, device=dev)
    pred = torch.empty((n_clips, 2), dtype=torch.int64, device=dev)
    counts = torch.zeros(2, dtype=torch.int64, device=dev)
    stream = torch.cuda.current_stream().cuda_stream

    def call(i):
        _lib.check(L.pca_clip_aggregate(bufs[i % copies].data_ptr(), n_sets, C, off.data_ptr(), n_clips,
                                        own.data_ptr(), mean.data_ptr(), votes.data_ptr(),
                                        pred.data_ptr(), counts.data_ptr(), 0, stream),
                   "pca_clip_aggregate")

    call(0)
    lp = torch.log_softmax(bufs[0].double(), 1).view(n_clips, T, C).mean(1)
    am = bufs[0].view(n_clips, T, C).argmax(2)
    ref_votes = torch.zeros((n_clips, C), dtype=torch.int64, device=dev).scatter_add_(
        1, am, torch.ones_like(am))
    same_votes = bool((votes.long() == ref_votes).all())
    agree_mean = float((pred[:, 1] == lp.argmax(1)).double().mean())
    err = float((mean.double() - lp).abs().max())

    for i in range(5):
        call(i)
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    calls = args.calls
    if calls <= 0:
        e0.record()
        for i in range(10):
            call(i)
        e1.record()
        torch.cuda.synchronize()
        calls = max(10, int(20.0 / max(e0.elapsed_time(e1) / 10, 1e-4)))
    per_call = []
    for _ in range(args.windows):
        e0.record()
        for i in range(calls):
            call(i)
        e1.record()
        torch.cuda.synchronize()
        per_call.append(e0.elapsed_time(e1) * 1e-3 / calls)
    per_call.sort()
    med, lo, hi = per_call[len(per_call) // 2], per_call[0], per_call[-1]

    lines = [
        f"logits [{n_sets}, {C}] = {n_clips} clips x {T} frames, {nbytes / 1e6:.3f} MB; {copies} "
        f"buffer(s) in rotation ({copies * nbytes / 2 ** 20:.0f} MiB against the 256 MiB Infinity Cache)",
        f"pca_clip_aggregate (k_clip_aggregate, all outputs + tally), HIP-event windows of {calls} calls"
        f" x {args.windows}: median {med * 1e6:.2f} us per call (min {lo * 1e6:.2f}, max {hi * 1e6:.2f})",
        f"logits' bytes / 8 TB/s = {nbytes / HBM_PEAK * 1e6:.2f} us; achieved {nbytes / med / 1e12:.3f} "
        f"TB/s = {nbytes / med / HBM_PEAK:.3f} of the HBM peak",
        f"votes equal torch's: {same_votes}; mean-rule predictions equal torch's float64 on "
        f"{agree_mean:.4f} of the clips; max |mean_logprob - float64| = {err:.2e}",
    ]
    text = "\n".join(lines)
    print(text)
    if args.out:
        with open(args.out, "w") as f:
            f.write(text + "\n")
    assert same_votes and err < 1e-4 * max(1.0, float(lp.abs().max()))


if __name__ == "__main__":
    main()
