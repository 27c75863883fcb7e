"""Time of the held-out metrics kernel (pca_eval_metrics) and of one held-out pass on one GPU.

  python scripts/eval_bench.py [--windows 15] [--passes 7] [--out FILE]

Kernel: the whole ABI call (rows, counters, confusion matrix, loss sum) on [862000, 50] logits, rotated
over enough buffers to leave the 256 MiB Infinity Cache between calls, and on the cache-resident
[4096, 10], as the median of --windows HIP-event windows (as scripts/clip_bench.py, whose committed
figures for k_clip_aggregate on the same shapes are printed next to it, with logits' bytes / 8 TB/s).
Pass: one trainer.Evaluator.run() against one trainer.evaluate() call in this process, on bench.py's
synthetic corpus at the cfg2 shape: the median, minimum and maximum of --passes passes after one warm-up."""
import argparse
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "point-cloud-audio_amd")]

HBM_PEAK = 8.0e12
CLIP_US = {(862000, 50): 251.5, (4096, 10): 20.1}      # profiles/clip_bench.txt


def kernel_time(n, C, windows, dev):
    import pca_hip
    from pca_hip import _lib
    L = pca_hip.lib()
    nbytes = 4.0 * n * C
    copies = min(8, max(1, int(np.ceil(2 ** 30 / nbytes)))) if nbytes > 2 ** 24 else 1
    g = torch.Generator(device=dev).manual_seed(0)
    labels = torch.randint(0, C, (n,), generator=g, device=dev)
    bufs = []
    for _ in range(copies):
        x = torch.randn((n, C), generator=g, device=dev)
        x.scatter_add_(1, labels.view(-1, 1), torch.full((n, 1), 3.0, device=dev))
        bufs.append(x)
    loss = torch.empty(n, dtype=torch.float32, device=dev)
    pred = torch.empty(n, dtype=torch.int64, device=dev)
    rank = torch.empty(n, dtype=torch.int32, device=dev)
    counts = torch.zeros(4, dtype=torch.int64, device=dev)
    conf = torch.zeros((C, C), dtype=torch.int64, device=dev)
    lsum = torch.zeros(1, dtype=torch.float64, device=dev)
    ws = torch.empty(max(256, L.pca_eval_metrics_ws_bytes(n)), dtype=torch.uint8, device=dev)
    stream = torch.cuda.current_stream().cuda_stream

    def call(i):
        _lib.check(L.pca_eval_metrics(bufs[i % copies].data_ptr(), labels.data_ptr(), n, C, 5,
                                      loss.data_ptr(), pred.data_ptr(), rank.data_ptr(), counts.data_ptr(),
                                      0, conf.data_ptr(), lsum.data_ptr(), ws.data_ptr(), stream),
                   "pca_eval_metrics")

    call(0)
    ref = torch.nn.functional.cross_entropy(bufs[0].double(), labels, reduction="none")
    err = float((loss.double() - ref).abs().max())
    same = bool((pred == bufs[0].argmax(1)).all()) and int(counts[0]) == n
    for i in range(5):
        call(i)
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for i in range(10):
        call(i)
    e1.record()
    torch.cuda.synchronize()
    calls = max(10, int(20.0 / max(e0.elapsed_time(e1) / 10, 1e-4)))
    per = []
    for _ in range(windows):
        e0.record()
        for i in range(calls):
            call(i)
        e1.record()
        torch.cuda.synchronize()
        per.append(e0.elapsed_time(e1) * 1e3 / calls)
    per.sort()
    med = per[len(per) // 2]
    assert same and err < 1e-4 * max(1.0, float(ref.abs().max()))
    return [
        f"logits [{n}, {C}], {nbytes / 1e6:.3f} MB, {copies} buffer(s) in rotation: pca_eval_metrics (all "
        f"outputs), windows of {calls} calls x {windows}: median {med:.2f} us per call (min {per[0]:.2f}, "
        f"max {per[-1]:.2f})",
        f"  logits' bytes / 8 TB/s = {nbytes / HBM_PEAK * 1e6:.2f} us ({nbytes / HBM_PEAK * 1e6 / med:.3f} "
        f"of the HBM peak); k_clip_aggregate on this shape (profiles/clip_bench.txt): "
        f"{CLIP_US.get((n, C), float('nan')):.1f} us; predictions equal torch's: {same}; "
        f"max |row_loss - float64| = {err:.2e}",
    ]


def pass_time(passes, dev):
    import bench
    import models
    from pca_hip import _lib, trainer
    cfg = dict(bench.CONFIGS["cfg2"])
    ds, _ = bench.build_dataset(cfg, 8, dev, seed=0)
    torch.manual_seed(1)
    net = models.ST(dim_input=cfg["din"], dim_output=cfg["C"], num_inds=cfg["m"], dim_hidden=cfg["d"],
                    num_heads=cfg["h"]).to(dev)
    B, mode = cfg["B"], _lib.MODE_BF16

    def timed(fn):
        fn()                                           # warm-up
        ts = []
        for _ in range(passes):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            fn()
            torch.cuda.synchronize()
            ts.append((time.perf_counter() - t0) * 1e3)
        ts.sort()
        return ts[len(ts) // 2], ts[0], ts[-1]

    ev = trainer.Evaluator(net, ds, B, mode)
    acc_old = trainer.evaluate(net, ds, B, mode)[0]
    acc_new = ev.run()["acc"]
    old = timed(lambda: trainer.evaluate(net, ds, B, mode))
    new = timed(ev.run)
    return [
        f"held-out pass, cfg2 shape ({len(ds)} sets of {ds.num_points} points, batch {B}, bf16), wall time "
        f"of one call, {passes} passes after a warm-up: median (min, max) in ms",
        f"  trainer.evaluate : {old[0]:.2f} ({old[1]:.2f}, {old[2]:.2f})   accuracy {acc_old:.6f}",
        f"  Evaluator.run    : {new[0]:.2f} ({new[1]:.2f}, {new[2]:.2f})   accuracy {acc_new:.6f}",
    ]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--windows", type=int, default=15)
    ap.add_argument("--passes", type=int, default=7)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    assert torch.cuda.is_available(), "eval_bench needs a GPU"
    dev = torch.device("cuda", 0)
    lines = []
    for n, C in ((862000, 50), (4096, 10)):
        lines += kernel_time(n, C, args.windows, dev)
    lines += pass_time(args.passes, dev)
    text = "\n".join(lines)
    print(text)
    if args.out:
        with open(args.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
