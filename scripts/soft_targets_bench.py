"""Soft targets at the headline configuration (cfg2: B=128, N=512, d=128, h=4, m=16, C=50, bf16, hipGraph):
the train step on ESC_wave_pc with the background mix - hard labels against mix_targets=True with
label_smoothing=0.1, windows of 200 steps, the two Trainers taking turns - and the frame launch alone with
and without the two target outputs (300 eager calls between device events).  Prints one JSON line.
DESIGN 4.3, profiles/soft_targets_bench.txt."""
import json, os, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "point-cloud-audio_amd")):
    sys.path.insert(0, p)
import numpy as np
import torch
import bench
import dataset, models, pca_hip
from pca_hip import _lib, trainer

dev = torch.device("cuda", 0)
cfg = bench.CONFIGS["cfg2"]
clips = [bench.synth_clip(i, i % 50, seconds=5.0) for i in range(24)]
y = [i % 50 for i in range(24)]

def make(**kw):
    return dataset.ESC_wave_pc(clips, y, bench.FS, 1024, drop_nyquist=True, device=dev, seed=3, **kw)

def time_steps(tr, n=200, warm=30):
    for _ in range(warm):
        tr.step()
    torch.cuda.synchronize()
    out = []
    for _ in range(5):
        t0 = time.perf_counter()
        for _ in range(n):
            tr.step()
        torch.cuda.synchronize()
        out.append((time.perf_counter() - t0) / n * 1e3)
    return out

def trainer_of(ds, ls):
    torch.manual_seed(0)
    net = models.ST(dim_input=2, dim_output=50, num_inds=16, dim_hidden=128, num_heads=4).to(dev)
    return trainer.Trainer(net, ds, batch_size=128, mode=_lib.MODE_BF16, use_graph=True, seed=1, label_smoothing=ls)

res = {}
mix = dict(mix_clips="self", mix_prob=0.5, mix_snr_db=(-20.0, 20.0))
# alternate the two trainers' windows
a = trainer_of(make(**mix), 0.0)
b = trainer_of(make(mix_targets=True, **mix), 0.1)
ta, tb = [], []
for r in range(2):
    ta += time_steps(a, warm=30 if r == 0 else 5)
    tb += time_steps(b, warm=30 if r == 0 else 5)
res["step_ms_mix_hard_labels"] = ta
res["step_ms_mix_targets_eps0.1"] = tb

# the frame launch alone (events over 300 launches), with and without the two outputs, alternating
dh, ds = make(**mix), make(mix_targets=True, **mix)
idx = torch.randint(0, len(dh), (128,), device=dev)
X = torch.empty((128, 512, 2), device=dev); lab = torch.empty(128, dtype=torch.int64, device=dev)
l2 = torch.empty(128, dtype=torch.int64, device=dev); w = torch.empty(128, device=dev)
def frame_time(d, kw, n=300):
    for _ in range(20):
        d.batch(idx, out=X, labels_out=lab, **kw)
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize(); e0.record()
    for _ in range(n):
        d.batch(idx, out=X, labels_out=lab, **kw)
    e1.record(); torch.cuda.synchronize()
    return e0.elapsed_time(e1) / n * 1e3
fa, fb = [], []
for r in range(4):
    fa.append(frame_time(dh, {}))
    fb.append(frame_time(ds, dict(labels2_out=l2, weight_out=w)))
res["frame_launch_us_eager_without_targets"] = fa
res["frame_launch_us_eager_with_targets"] = fb
print(json.dumps(res))
