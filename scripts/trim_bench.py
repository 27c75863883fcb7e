"""Time of the silence trim (pca_trim_bounds: k_trim_segsum + k_trim_bounds) on one GPU.

  python scripts/trim_bench.py [--clips 8] [--windows 15] [--calls 0] [--host-clips 8] [--out FILE]
  rocprofv3 --kernel-trace --stats --output-format csv -d DIR -- \\
      python scripts/trim_bench.py --clips 2000 --profile-only

Corpus: --clips 5-s clips at 44.1 kHz.  Up to 8 clips are bench.py's synthetic clips; more (the
ESC-50-shaped 2000 x 5 s = 1.76 GB of samples, past the 256 MiB Infinity Cache) are those 8 scaled by a
per-clip gain plus seeded noise, made on the device.  Every clip gets digital silence of uneven length
written over both ends so that there is something to trim.

Measured: the ABI call on a pre-concatenated corpus, as the median over --windows HIP-event windows of
--calls calls each (0: sized to about 20 ms of work) after a warm-up; achieved bytes/s with algorithmic
bytes = 4 x samples, as a fraction of the 8 TB/s HBM peak; the wall time of pca_hip.trim_batch (one
torch.cat, the launches, one host read); and the wall time of the numpy restatement (tests/trim_ref.py)
on --host-clips clips of the same corpus on this host, scaled to the corpus - the host route a user
would otherwise write, NOT a librosa timing.  The bounds of those clips are compared with the
restatement's.  --profile-only: warm-up + 20 calls and nothing else, for a rocprofv3 kernel trace."""
import argparse
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "point-cloud-audio_amd"), os.path.join(ROOT, "scripts"),
                os.path.join(ROOT, "tests")]

from sweep_bench import FS, synth_clip  # noqa: E402

HBM_PEAK = 8.0e12


def corpus(n, dev):
    base = [torch.from_numpy(synth_clip(i, i % 10)).to(dev) for i in range(min(n, 8))]
    g = torch.Generator(device=dev).manual_seed(0)
    clips = []
    for i in range(n):
        if i < 8:
            x = base[i].clone()
        else:
            gain = 0.25 + 0.75 * float(torch.rand((), generator=g, device=dev))
            x = base[i % 8] * gain + 1e-3 * torch.randn(base[i % 8].numel(), generator=g, device=dev)
        x[:(i * 7919) % 30011] = 0.0
        x[x.numel() - (i * 104729) % 20011:] = 0.0
        clips.append(x)
    return clips


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--clips", type=int, default=8)
    ap.add_argument("--windows", type=int, default=15)
    ap.add_argument("--calls", type=int, default=0)
    ap.add_argument("--host-clips", type=int, default=8)
    ap.add_argument("--top-db", type=float, default=60.0)
    ap.add_argument("--profile-only", action="store_true")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()

    import pca_hip
    from pca_hip import _lib

    assert torch.cuda.is_available(), "trim_bench needs a GPU"
    dev = torch.device("cuda", 0)
    L = pca_hip.lib()
    clips = corpus(args.clips, dev)
    lens = [int(c.numel()) for c in clips]
    cat = torch.cat(clips)
    woff = torch.tensor(np.concatenate([[0], np.cumsum(lens)]), dtype=torch.int64, device=dev)
    bounds = torch.empty((len(clips), 2), dtype=torch.int64, device=dev)
    ws = torch.empty(L.pca_trim_ws_bytes(cat.numel(), len(clips), 2048, 512), dtype=torch.uint8,
                     device=dev)
    stream = torch.cuda.current_stream().cuda_stream

    def call():
        _lib.check(L.pca_trim_bounds(cat.data_ptr(), woff.data_ptr(), len(clips), max(lens), min(lens),
                                     2048, 512, args.top_db, bounds.data_ptr(), ws.data_ptr(), stream),
                   "pca_trim_bounds")

    for _ in range(5):
        call()
    torch.cuda.synchronize()
    if args.profile_only:
        for _ in range(20):
            call()
        torch.cuda.synchronize()
        return

    nbytes = 4.0 * cat.numel()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    calls = args.calls
    if calls <= 0:                       # size a window to ~20 ms from a first 10-call window
        e0.record()
        for _ in range(10):
            call()
        e1.record()
        torch.cuda.synchronize()
        calls = max(10, int(20.0 / max(e0.elapsed_time(e1) / 10, 1e-4)))
    per_call = []
    for _ in range(args.windows):
        e0.record()
        for _ in range(calls):
            call()
        e1.record()
        torch.cuda.synchronize()
        per_call.append(e0.elapsed_time(e1) * 1e-3 / calls)
    per_call.sort()
    med, lo, hi = per_call[len(per_call) // 2], per_call[0], per_call[-1]

    pca_hip.trim_batch(clips, args.top_db)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    _, b = pca_hip.trim_batch(clips, args.top_db)
    t_batch = time.perf_counter() - t0

    import trim_ref
    nh = min(args.host_clips, len(clips))
    host = [c.cpu().numpy() for c in clips[:nh]]
    t0 = time.perf_counter()
    ref = [trim_ref.trim_ref(y, args.top_db) for y in host]
    t_host = time.perf_counter() - t0
    same = [tuple(x) for x in b[:nh].tolist()] == ref
    margin = min(trim_ref.decision_margin(y, args.top_db) for y in host)

    lines = [
        f"corpus: {len(clips)} clips x 5 s at {FS} Hz = {cat.numel()} samples, {nbytes / 1e9:.4f} GB"
        f" (algorithmic bytes = 4 x samples); frame 2048, hop 512, top_db {args.top_db:g}",
        f"pca_trim_bounds (k_trim_segsum + k_trim_bounds), HIP-event windows of {calls} calls x "
        f"{args.windows}: median {med * 1e6:.2f} us per call (min {lo * 1e6:.2f}, max {hi * 1e6:.2f})",
        f"achieved {nbytes / med / 1e12:.3f} TB/s = {nbytes / med / HBM_PEAK:.3f} of the 8 TB/s HBM peak"
        + (" (the corpus fits the 256 MiB Infinity Cache: repeated calls do not read HBM)"
           if nbytes < 256 * 2 ** 20 else ""),
        f"pca_hip.trim_batch wall (torch.cat + launches + one host read of the bounds): "
        f"{t_batch * 1e3:.3f} ms",
        f"numpy restatement on this host (not a librosa timing): {t_host * 1e3:.1f} ms for {nh} clips"
        f" -> {t_host / nh * len(clips) * 1e3:.1f} ms scaled to the corpus",
        f"bounds of the first {nh} clips equal the restatement's: {same} (smallest decision margin "
        f"{margin:.3g} dB); kept samples {int((b[:, 1] - b[:, 0]).sum())} of {cat.numel()}",
    ]
    text = "\n".join(lines)
    print(text)
    if args.out:
        with open(args.out, "w") as f:
            f.write(text + "\n")
    assert same, (b[:nh].tolist(), ref)


if __name__ == "__main__":
    main()
