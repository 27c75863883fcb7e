#!/usr/bin/env python3
"""golden_baselines.npz + golden_baselines_fb{0,1,2}.npz: the shipped FB and CNN_temp checkpoints
and the REAL reference's outputs for them, on CPU.  Run in the build container only:
``python tests/golden/make_golden_baselines.py``.

  * the shipped state_dicts as flat fp32 vectors in state_dict order (the FB one, 2.6 MB, split over
    three files so that no file passes 1 MiB; the key names and shapes are in golden_base.npz);
  * eval-mode outputs of the reference's baseline_ff / CNN_classifier (Code/models.py:47-119) on
    the seeded inputs of inputs_baselines.py (FB probabilities, CNN_temp logits);
  * max-K zero-filled items for K in {1, 51, 501, all}: CNN_temp from the reference's
    ESC_baseline_temporal_maxK(flag="max") (Code/dataset.py:101-135); FB from pc_maxK_replace,
    restated from Code/utils.py:86-96's numpy lines (the module imports prettytable, absent here).
Only data is stored: inputs come from seeds, outputs from the reference."""
import os
import sys
import warnings

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
REF = os.environ.get("PCA_REFERENCE", "/root/reference")
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.join(REF, "set_transformer-master"))
sys.path.insert(0, os.path.join(REF, "Code"))
os.chdir(os.path.join(REF, "Code"))

import inputs_baselines as gi  # noqa: E402
import models as ref_models  # noqa: E402  (reference)
import dataset as ref_dataset  # noqa: E402


def pc_maxK_replace(x, Kmax):
    # Code/utils.py:86-96, verbatim numpy
    xreplace = []
    for i in range(x.shape[1]):
        temp = np.zeros(x[:, i].shape[0])
        indices = (-x[:, i]).argsort()[:Kmax]
        temp[indices] = x[:, i][indices]
        xreplace.append(temp)
    return np.array(xreplace).T


def _load(tag):
    return torch.load(os.path.join(REF, "Code", "model_saves", tag + "_net.pth"),
                      weights_only=True, map_location="cpu")


def main():
    out = {}
    fb = ref_models.baseline_ff(gi.FB_DIMS, gi.NCLASS, p=0.5)
    fb.load_state_dict(_load(gi.FB_CKPT))
    fb.eval()
    cnn = ref_models.CNN_classifier(gi.NT, gi.NF, gi.CNN_DIMS, gi.NCLASS, 0.5)
    cnn.load_state_dict(_load(gi.CNN_CKPT))
    cnn.eval()
    fb_flat = torch.cat([v.reshape(-1) for v in fb.state_dict().values()]).numpy()
    out["cnn/flat"] = torch.cat([v.reshape(-1) for v in cnn.state_dict().values()]).numpy()
    xf, xc = gi.fb_frames(), gi.cnn_chunks()
    with warnings.catch_warnings(), torch.no_grad():
        warnings.simplefilter("ignore")                    # nn.Softmax() without dim
        out["fb/y"] = fb(torch.from_numpy(xf)).numpy()
        out["cnn/y"] = cnn(torch.from_numpy(xc)).numpy()
    # max-K items of the first MAXK_SETS sets
    frames = xf[:gi.MAXK_SETS].T                           # [F, T], the reference's x_test layout
    chunks = np.ascontiguousarray(xc[:gi.MAXK_SETS].transpose(2, 1, 0))   # [Nf, Nt, S]
    for K in gi.MAXK_K["fb"]:
        out[f"fb/maxK{K}"] = pc_maxK_replace(frames, K).T.astype(np.float32)      # [S, F]
    for K in gi.MAXK_K["cnn"]:
        ds = ref_dataset.ESC_baseline_temporal_maxK(chunks, np.zeros(gi.MAXK_SETS, int), K, "max")
        out[f"cnn/maxK{K}"] = np.stack([ds[i][1].numpy() for i in range(gi.MAXK_SETS)])  # [S, Nt, Nf]
    np.savez_compressed(os.path.join(HERE, "golden_baselines.npz"), **out)
    for i, part in enumerate(np.array_split(fb_flat, gi.FB_PARTS)):
        np.savez_compressed(os.path.join(HERE, f"golden_baselines_fb{i}.npz"), flat=part)
    print("wrote golden_baselines*.npz:", {k: v.shape for k, v in out.items()}, fb_flat.shape)


if __name__ == "__main__":
    main()
