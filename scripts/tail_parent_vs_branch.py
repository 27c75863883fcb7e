#!/usr/bin/env python3
"""d = 128 backward tail: same launches and same bits from two builds of libpca_hip.so (a parent's and a branch's).

  python scripts/tail_parent_vs_branch.py run --lib PARENT.so --out parent.json     # one fresh process per
  python scripts/tail_parent_vs_branch.py run --lib BRANCH.so --out branch.json     # library, each under its
  python scripts/tail_parent_vs_branch.py compare parent.json branch.json           # own timeout, chained by &&

`run` loads the given library and, for every case and form below, runs one eager train step (the switches are
read per call) and one more under the profiler; it records the ordered library kernels with their grids and the
sha256 of logits, loss and gradients.  `compare` prints one line per case and form and exits 1 on a difference.
PCA_WGRAD_SLABS=0 adds with fp32 atomics and is not bit-stable: names and grids only."""
import argparse
import hashlib
import json
import os
import re
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (os.path.join(ROOT, "point-cloud-audio_amd"), os.path.join(ROOT, "tests", "golden"), ROOT):
    sys.path.insert(0, p)

D, H, M, C = 128, 4, 16, 10
CASES = [(3, 256, 2, None), (5, 512, 3, None), (3, 300, 2, (300, 257, 33)), (9, 128, 2, None)]   # B, N, din, lengths
SWITCHES = ("PCA_POST_FUSE", "PCA_WGRAD_RIDE", "PCA_WGRAD_FOLD", "PCA_D128_MIDFUSE", "PCA_WGRAD_SLABS")
FORMS = [("default", {}, False), ("PCA_POST_FUSE=0", {"PCA_POST_FUSE": "0"}, False),
         ("PCA_WGRAD_RIDE=0", {"PCA_WGRAD_RIDE": "0"}, False), ("PCA_WGRAD_FOLD=0", {"PCA_WGRAD_FOLD": "0"}, False),
         ("PCA_D128_MIDFUSE=0", {"PCA_D128_MIDFUSE": "0"}, False),
         ("PCA_WGRAD_FOLD=0 PCA_POST_FUSE=1", {"PCA_WGRAD_FOLD": "0", "PCA_POST_FUSE": "1"}, False),
         ("split step", {}, True), ("PCA_WGRAD_SLABS=0", {"PCA_WGRAD_SLABS": "0"}, False)]
NOT_BIT_STABLE = {"PCA_WGRAD_SLABS=0"}


def case_id(c):
    return f"B{c[0]}-N{c[1]}-din{c[2]}" + ("-lengths" if c[3] else "")


def kernels_with_grids(fn):
    import torch
    from torch.profiler import ProfilerActivity, profile
    torch.cuda.synchronize()
    with profile(activities=[ProfilerActivity.CPU, ProfilerActivity.CUDA]) as prof:
        fn()
        torch.cuda.synchronize()
    with tempfile.TemporaryDirectory() as td:
        path = os.path.join(td, "trace.json")
        prof.export_chrome_trace(path)
        events = json.load(open(path))["traceEvents"]
    ks = [e for e in events if e.get("cat") == "kernel" and "pca" in e.get("name", "")]
    ks.sort(key=lambda e: e["ts"])
    return [[e["name"]] + list(e.get("args", {}).get("grid", ["?"])) for e in ks]


def run(lib, out):
    import torch
    import inputs as gi
    import models
    from pca_hip import _lib, trainer
    _lib.LIB_PATH = os.path.abspath(lib)
    import ctypes
    handle = ctypes.CDLL(_lib.LIB_PATH)
    _lib.DEBUG_SIGNATURES = {k: v for k, v in getattr(_lib, "DEBUG_SIGNATURES", {}).items() if hasattr(handle, k)}
    _lib.lib()
    dev = torch.device("cuda", 0)
    res = {}
    for case in CASES:
        B, N, din, lengths = case
        torch.manual_seed(900 + N + din)
        net = models.ST(dim_input=din, num_outputs=1, dim_output=C, num_inds=M, dim_hidden=D, num_heads=H).to(dev)
        Xn = gi.pc_input(9100 + N + B, B, N, din)
        if lengths is not None:
            for b, L in enumerate(lengths):
                Xn[b, L:] = 0.0
        X = torch.from_numpy(Xn).to(dev)
        y = torch.from_numpy(gi.labels(9101 + N + B, B, C)).to(dev)
        ld = None if lengths is None else torch.tensor(lengths, dtype=torch.int32, device=dev)
        for name, env, split in FORMS:
            for k in SWITCHES:
                os.environ.pop(k, None)
            os.environ.update(env)
            eng = trainer.STEngine(net, B, N, _lib.MODE_BF16, training=True)

            def step():
                for ph in ((0, 1) if split else (-1,)):
                    eng.fwd_bwd(X, y, phase=ph, lengths=ld)
            step()
            torch.cuda.synchronize()
            sha = {k: hashlib.sha256(getattr(eng, k).detach().cpu().numpy().tobytes()).hexdigest()
                   for k in ("logits", "loss", "grads")}
            res[f"{case_id(case)} | {name}"] = {"sha": sha, "kernels": kernels_with_grids(step)}
    for k in SWITCHES:
        os.environ.pop(k, None)
    json.dump(res, open(out, "w"), indent=1)
    print(f"{len(res)} steps recorded -> {out}")


def compare(a_path, b_path):
    a, b = json.load(open(a_path)), json.load(open(b_path))
    bad = 0
    assert list(a) == list(b), "different cases"
    for key in a:
        ka, kb = a[key]["kernels"], b[key]["kernels"]
        form = key.split(" | ")[1]
        same_k = ka == kb
        same_b = a[key]["sha"] == b[key]["sha"]
        ok = same_k and (same_b or form in NOT_BIT_STABLE)
        bad += not ok
        bits = "same bits" if same_b else ("bits differ (atomics: not compared)" if form in NOT_BIT_STABLE else "BITS DIFFER")
        tail = [k for k in ka if any(s in k[0] for s in ("wgrad128", "terminal1", "mab0_post", "small_ride", "slab_sum"))]
        short = " ".join(f"{re.search('k_[a-z0-9_]+', k[0]).group(0)}{tuple(k[1:3])}" for k in tail)
        print(f"{key:52s} kernels {len(ka):3d} / {len(kb):3d} {'same names and grids' if same_k else 'LAUNCHES DIFFER'}; "
              f"{bits}\n    tail: {short}")
    print("RESULT:", "met" if bad == 0 else f"{bad} case(s) differ")
    return 1 if bad else 0


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    sub = ap.add_subparsers(dest="cmd", required=True)
    r = sub.add_parser("run")
    r.add_argument("--lib", required=True)
    r.add_argument("--out", required=True)
    c = sub.add_parser("compare")
    c.add_argument("a")
    c.add_argument("b")
    args = ap.parse_args()
    sys.exit(run(args.lib, args.out) if args.cmd == "run" else compare(args.a, args.b))
