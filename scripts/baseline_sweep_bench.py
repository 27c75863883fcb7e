"""Wall time of the baselines' device sweeps (evalsweep.baseline_*) on one GPU, against the item-level
host route of Code/baseline_eval.py / Code/baseline_temp_eval.py, on sweep_bench.py's synthetic corpus.

  python scripts/baseline_sweep_bench.py [--clips 8] [--n-runs 10] [--item-sets 256] [--out FILE]

Times, with random weights at the shipped shapes (FB [1025, 513, 256] -> 10; CNN_temp Nt 10, Nf 512,
[512, 256, 100] -> 10; accuracies are meaningless, the work is not):
  * baseline_subsample_sweep over default_list_K (FB: 21 K of 1024, CNN_temp: 103 K of 5120),
    n_runs random-K runs + one max-K pass per K;
  * baseline_reframe_sweep / _temporal over the 9 analysis lengths of Code/baseline_eval.py:51;
  * the host route: FB Experiment 2 = utils.pc_randK_replace over the whole corpus + ESC_baseline +
    DataLoader(batch 128) + model, timed for one run and multiplied by the passes; CNN_temp
    Experiment 2 = ESC_baseline_temporal_maxK(flag "rand") items + DataLoader(batch 2) + model on
    --item-sets chunks, extrapolated per set; Experiment 1 = per-clip STFT copied to the host,
    framed / chunked there, DataLoader + model, timed over all lengths.
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
sys.path[:0] = [ROOT, os.path.join(ROOT, "point-cloud-audio_amd"), os.path.join(ROOT, "scripts")]

from sweep_bench import FS, _sync_time, synth_clip  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--clips", type=int, default=8, help="5-s clips in the corpus")
    ap.add_argument("--n-runs", type=int, default=10)
    ap.add_argument("--item-sets", type=int, default=256, help="CNN_temp chunks timed on the host route")
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
    res = {"clips": args.clips, "clip_seconds": 5.0, "fs": FS, "n_runs": args.n_runs}
    torch.manual_seed(0)
    fb = models.baseline_ff([1025, 513, 256], C_).to(dev).eval()
    cnn = models.CNN_classifier(10, 512, [512, 256, 100], C_).to(dev).eval()

    def loader_correct(model, ds, bs, skip_short):
        c = 0
        for lbls, imgs in torch.utils.data.DataLoader(ds, batch_size=bs, shuffle=True):
            if skip_short and lbls.shape[0] < bs:
                continue
            c += (model(imgs.float().to(dev)).argmax(dim=1) == lbls.to(dev)).sum().item()
        return c

    # ---- Experiment 2 -------------------------------------------------------------------------
    spec, foff = pca_hip.stft_logmag_batch(waves, 2048, 2048, 1024, frame_major=True)
    xf = spec.t()                                                       # [1025, T]
    yf = np.concatenate([np.full(foff[c + 1] - foff[c], labels[c]) for c in range(len(waves))])
    spec, foff = pca_hip.stft_logmag_batch(waves, 1024, 1024, 512, drop_nyquist=True,
                                           frame_major=True)
    chunks, yc = [], []
    for c in range(len(waves)):
        s = spec[foff[c]:foff[c + 1]]
        S = s.shape[0] // 10
        chunks.append(s[:S * 10].reshape(S, 10, 512))
        yc += [labels[c]] * S
    xc, yc = torch.cat(chunks).permute(2, 1, 0), np.asarray(yc)         # [512, 10, S]
    with torch.no_grad():
        for tag, model, x, y in (("fb", fb, xf, yf), ("cnn_temp", cnn, xc, yc)):
            eng = pca_hip.BaselineEngine(model)
            n_sets = x.shape[-1]
            list_K = evalsweep.default_list_K(x.shape[0] - 1 if tag == "fb" else 5120)
            evalsweep.baseline_subsample_sweep(eng, x, y, list_K[:1], n_runs=1)   # warm-up
            t, _ = _sync_time(lambda: evalsweep.baseline_subsample_sweep(eng, x, y, list_K,
                                                                         n_runs=args.n_runs))
            passes = (args.n_runs + 1) * len(list_K)
            n_eval = passes * (n_sets if tag == "fb" else (n_sets // 2) * 2)
            Km = list_K[len(list_K) // 2]
            if tag == "fb":
                x_np = x.cpu().numpy()

                def host():
                    xss = utils.pc_randK_replace(x_np, Km)
                    return loader_correct(model, dataset.ESC_baseline(xss, y), 128, False)
                host()
                th, _ = _sync_time(host)
                host_s, item_sets = th * passes, n_sets
            else:
                m = min(args.item_sets, n_sets)
                x_np = x[:, :, :m].cpu().numpy()

                def host():
                    ds = dataset.ESC_baseline_temporal_maxK(x_np, y[:m], Km, flag="rand")
                    return loader_correct(model, ds, 2, True)
                host()
                th, _ = _sync_time(host)
                host_s, item_sets = th / m * n_eval, m
            res[tag] = {"sets": int(n_sets), "cells": int(np.prod(x.shape[:-1])), "n_K": len(list_K),
                        "sweep_s": round(t, 3), "sets_evaluated": int(n_eval),
                        "sweep_us_per_set": round(1e6 * t / n_eval, 3), "host_K": int(Km),
                        "host_sets_timed": int(item_sets), "host_s": round(host_s, 1)}
            print(json.dumps({tag: res[tag]}), flush=True)

        # ---- Experiment 1: the 9 lengths of Code/baseline_eval.py:51 at the recorded rate -------
        for tag, model, n_fft in (("fb_reframe", fb, 2048), ("cnn_temp_reframe", cnn, 1024)):
            eng = pca_hip.BaselineEngine(model)
            list_N = [n_fft] + [int(f * n_fft) for f in (0.95, 0.9, 0.8, 0.7, 0.6, 0.5, 0.25, 0.1)]
            sweep = evalsweep.baseline_reframe_sweep if tag == "fb_reframe" \
                else evalsweep.baseline_reframe_sweep_temporal
            sweep(eng, waves, labels, FS, list_N[:1])
            t, _ = _sync_time(lambda: sweep(eng, waves, labels, FS, list_N))

            def host():
                for N in list_N:
                    d, ls = [], []
                    for w, lab in zip(waves, labels):
                        a = pca_hip.stft_logmag(w, n_fft, win_length=N, hop=int(N * 0.5),
                                                drop_nyquist=tag != "fb_reframe").cpu().numpy()
                        if tag == "fb_reframe":
                            d.append(a)
                            ls.append(lab * np.ones(a.shape[1]))
                        else:
                            for ss in np.hsplit(a, np.arange(0, a.shape[1], 10)):
                                if ss.shape[1] == 10:
                                    d.append(ss)
                                    ls.append(lab)
                    if tag == "fb_reframe":
                        ds = dataset.ESC_baseline(np.concatenate(d, 1),
                                                  np.concatenate(ls).astype(int))
                        loader_correct(model, ds, 128, False)
                    else:
                        ds = dataset.ESC_baseline_temporal(np.dstack(d), np.array(ls).astype(int))
                        loader_correct(model, ds, 2, True)
            th, _ = _sync_time(host)
            res[tag] = {"list_N": list_N, "sweep_s": round(t, 3), "host_s": round(th, 2)}
            print(json.dumps({tag: res[tag]}), flush=True)
    line = json.dumps(res)
    print(line)
    if args.out:
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
