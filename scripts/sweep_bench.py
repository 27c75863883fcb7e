"""Wall time of the batch-scale evaluation sweeps (evalsweep.py) on one GPU, against the item-level
route they replace, on the synthetic ESC-shaped corpus of bench.py (its generator restated here).

  python scripts/sweep_bench.py [--clips 8] [--k-stride 1] [--n-runs 10] [--out FILE]

Times, with random weights (accuracies are meaningless; the work is not):
  * subsample_sweep at the shipped FST shape (N = 1025, d = 64, h = 8, m = 64) and 3ST shape
    (N = 5120 = 512 bins x 10 frames, same model), list_K = default_list_K(n)[::k_stride], n_runs
    random-K runs + one max-K pass per K;
  * reframe_sweep_temporal over the 13 analysis lengths of Code/pc_temp3d_eval.py:59 at one rate;
  * the item-level route on a slice (utils.pc_randK -> ESC_pc_ss -> DataLoader(batch_size=8) ->
    model(imgs) for FST; ESC_pc_temp_randKSS[i] -> DataLoader -> model(imgs) for 3ST), extrapolated
    per set.
Prints one JSON line (and writes it to --out).
"""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "point-cloud-audio_amd")]

FS = 44100


def synth_clip(clip_id: int, cls: int, seconds: float = 5.0, fs: int = FS) -> np.ndarray:
    """bench.py's generator: 3 harmonics of f0(c) = 110*2^(c/12) Hz with seeded phases + low-passed
    noise, PCG64(seed = 1000 + clip_id); float32 in [-1, 1]."""
    rng = np.random.Generator(np.random.PCG64(1000 + clip_id))
    L = int(round(seconds * fs))
    t = np.arange(L) / fs
    f0 = 110.0 * 2.0 ** (cls / 12.0)
    x = np.zeros(L)
    for k in range(1, 4):
        x += (0.5 / k) * np.sin(2 * np.pi * f0 * k * t + rng.uniform(0, 2 * np.pi))
    noise = np.convolve(rng.standard_normal(L), np.ones(8) / 8.0, mode="same")
    x = x + 0.1 * noise
    x = x / (np.max(np.abs(x)) + 1e-9) * 0.9
    return x.astype(np.float32)


def _sync_time(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    r = fn()
    torch.cuda.synchronize()
    return time.perf_counter() - t0, r


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--clips", type=int, default=8, help="5-s clips in the corpus")
    ap.add_argument("--k-stride", type=int, default=1, help="every k-th K of default_list_K")
    ap.add_argument("--n-runs", type=int, default=10)
    ap.add_argument("--item-sets", type=int, default=64, help="sets timed on the item-level route")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()

    import dataset
    import evalsweep
    import models
    import pca_hip
    import utils

    dev = torch.device("cuda", 0)
    C_ = 10
    waves = [torch.from_numpy(synth_clip(i, i % C_)).to(dev) for i in range(args.clips)]
    labels = [i % C_ for i in range(args.clips)]
    res = {"clips": args.clips, "clip_seconds": 5.0, "fs": FS, "n_runs": args.n_runs,
           "k_stride": args.k_stride}

    def corpus(n_fft, drop, ntemp):
        spec, foff = pca_hip.stft_logmag_batch(waves, n_fft, n_fft, n_fft // 2,
                                               drop_nyquist=drop, frame_major=True)
        F = spec.shape[1]
        if ntemp == 1:
            y = np.concatenate([np.full(foff[c + 1] - foff[c], labels[c]) for c in range(len(waves))])
            return spec.t(), y, np.linspace(0, FS / 2, F) / FS, None
        chunks, y = [], []
        for c in range(len(waves)):
            s = spec[foff[c]:foff[c + 1]]
            S = s.shape[0] // ntemp
            chunks.append(s[:S * ntemp].reshape(S, ntemp, F))
            y += [labels[c]] * S
        x = torch.cat(chunks).permute(2, 1, 0)                       # [F, Nt, S] view
        return x, np.asarray(y), np.linspace(0, FS / 2, F) / FS, \
            np.linspace(0, (n_fft // 2 / FS) * ntemp, ntemp)

    for tag, din, n_fft, drop, ntemp in (("fst", 2, 2048, False, 1), ("3st", 3, 1024, True, 10)):
        torch.manual_seed(0)
        net = models.ST(dim_input=din, dim_output=C_, num_inds=64, dim_hidden=64,
                        num_heads=8).to(dev)
        x, y, farr, tarr = corpus(n_fft, drop, ntemp)
        n_sets = x.shape[-1]
        n = (x.shape[0] - 1) if ntemp == 1 else x.shape[0] * x.shape[1]
        list_K = evalsweep.default_list_K(n)[::args.k_stride]
        # warm-up: first launches, engine construction
        evalsweep.subsample_sweep(net, x, y, farr, tarr, list_K=list_K[:1], n_runs=1)
        t, _ = _sync_time(lambda: evalsweep.subsample_sweep(net, x, y, farr, tarr, list_K=list_K,
                                                            n_runs=args.n_runs))
        full = (n_sets // 8) * 8
        n_eval = full * (args.n_runs + 1) * len(list_K)
        res[tag] = {"sets": int(n_sets), "points_per_set": int(np.prod(x.shape[:-1])),
                    "max_K": int(n), "n_K": len(list_K),
                    "sweep_s": round(t, 3), "sets_evaluated": int(n_eval),
                    "sweep_us_per_set": round(1e6 * t / n_eval, 3)}
        # item-level route on a slice, random-K at the middle K of the grid
        Km = list_K[len(list_K) // 2]
        m = args.item_sets
        net.eval()
        with torch.no_grad():
            if ntemp == 1:
                xs_np = x[:, :m].cpu().numpy()

                def item_route():
                    xs, fs_ = utils.pc_randK(xs_np, farr, Km)
                    ds = dataset.ESC_pc_ss(xs, y[:m], fs_, device=dev)
                    dl = torch.utils.data.DataLoader(ds, batch_size=8, shuffle=True)
                    c = 0
                    for imgs, lbls in dl:
                        c += (net(imgs.to(dev)).argmax(1) == lbls.to(dev)).sum().item()
                    return c
            else:
                x_np = x[:, :, :m].cpu().numpy()

                def item_route():
                    ds = dataset.ESC_pc_temp_randKSS(x_np, y[:m], farr, tarr, Km, device=dev)
                    dl = torch.utils.data.DataLoader(ds, batch_size=8, shuffle=True)
                    c = 0
                    for imgs, lbls in dl:
                        c += (net(imgs.float().to(dev)).argmax(1) == lbls.to(dev)).sum().item()
                    return c
            item_route()
            ti, _ = _sync_time(item_route)
        per = ti / m
        res[tag].update({"item_K": int(Km), "item_sets": m, "item_us_per_set": round(1e6 * per, 1),
                         "item_extrapolated_s": round(per * n_eval, 1)})
        print(json.dumps({tag: res[tag]}), flush=True)

    # 3-D re-framing at the recorded rate, the 13 lengths of Code/pc_temp3d_eval.py:59 (Nfft = 1024)
    torch.manual_seed(0)
    net = models.ST(dim_input=3, dim_output=C_, num_inds=64, dim_hidden=64, num_heads=8).to(dev)
    Nf = 1024
    list_N = [2 * Nf, int(1.5 * Nf), int(1.25 * Nf), int(1.05 * Nf), Nf, int(0.95 * Nf),
              int(0.9 * Nf), int(0.8 * Nf), int(0.7 * Nf), int(0.6 * Nf), int(0.5 * Nf),
              int(0.25 * Nf), int(0.1 * Nf)]
    evalsweep.reframe_sweep_temporal(net, waves, labels, FS, list_N[-1:])
    t, _ = _sync_time(lambda: evalsweep.reframe_sweep_temporal(net, waves, labels, FS, list_N))
    res["reframe_temporal"] = {"list_N": list_N, "sweep_s": round(t, 3)}
    line = json.dumps(res)
    print(line)
    if args.out:
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
