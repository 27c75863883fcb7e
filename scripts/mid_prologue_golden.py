#!/usr/bin/env python3
"""Record tests/golden/mid_prologue_sha256.json: the SHA-256 of logits, loss and each gradient of the cases of
tests/test_gpu_mid_prologue.py, from a given build of libpca_hip.so (the parent commit's, built into a directory
of its own with PCA_BUILD_DIR / PCA_OUT).  One fresh process:

  python scripts/mid_prologue_golden.py --lib PARENT.so --commit SHA --out tests/golden/mid_prologue_sha256.json

The default path and PCA_D128_MIDFUSE=0 must agree in that build too; the script refuses to write otherwise."""
import argparse
import ctypes
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (os.path.join(ROOT, "point-cloud-audio_amd"), os.path.join(ROOT, "tests", "golden"),
          os.path.join(ROOT, "tests"), ROOT):
    sys.path.insert(0, p)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--lib", required=True)
    ap.add_argument("--commit", required=True)
    ap.add_argument("--out", required=True)
    args = ap.parse_args()
    import torch
    import mid_prologue_cases as mc
    from pca_hip import _lib
    _lib.LIB_PATH = os.path.abspath(args.lib)
    handle = ctypes.CDLL(_lib.LIB_PATH)
    # (an older build may lack a debug entry point that this tree binds)
    _lib.DEBUG_SIGNATURES = {k: v for k, v in _lib.DEBUG_SIGNATURES.items() if hasattr(handle, k)}
    _lib.lib()
    dev = torch.device("cuda", 0)
    cases = {}
    for B, N, din in mc.CASES + mc.EXTRA:
        net = mc.net_of(dev, din, 900 + N + din)
        Xn, yn = mc.inputs_of(B, N, din)
        X, y = torch.from_numpy(Xn).to(dev), torch.from_numpy(yn).to(dev)
        for set128 in mc.paths(N):
            h1 = mc.hashes(net, mc.run(net, X, y, B, N, fuse=True, set128=set128))
            h0 = mc.hashes(net, mc.run(net, X, y, B, N, fuse=False, set128=set128))
            if h1 != h0:
                print(f"{mc.key(B, N, din, set128)}: fused and launches differ in this build", file=sys.stderr)
                return 1
            cases[mc.key(B, N, din, set128)] = h1
            print(mc.key(B, N, din, set128), h1["logits"][:16], h1["loss"][:16], flush=True)
    doc = {"produced_by": f"commit {args.commit} (the parent of the mid-prologue change), bf16 mode, one MI355X",
           "what": "sha256 of the bytes of logits, loss and each gradient after one eager train step",
           "cases": cases}
    with open(args.out, "w") as f:
        json.dump(doc, f, indent=1, sort_keys=True)
        f.write("\n")
    print(f"{len(cases)} cases -> {args.out}")
    return 0


if __name__ == "__main__":
    sys.exit(main())
