#!/usr/bin/env python3
"""Record tests/golden/set128_handoff2_sha256.json: the SHA-256 of logits, loss and each of the 45 gradients for the
cases of tests/test_gpu_set128_handoff2.py, from a given build of libpca_hip.so (the parent commit's, built into a
directory of its own with PCA_BUILD_DIR / PCA_OUT).  One fresh process:

  python scripts/set128_handoff2_golden.py --lib PARENT.so --commit SHA --out tests/golden/set128_handoff2_sha256.json

Before anything is recorded three passes of the given build must agree on every output that the test pins
(tests/set128_handoff2_cases.UNPINNED names the others), so that what the test then asks of a later build is what
its parent did."""
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
    import mab1_bwd_loads_cases as lc
    import set128_handoff2_cases as hc
    from pca_hip import _lib
    _lib.LIB_PATH = os.path.abspath(args.lib)
    handle = ctypes.CDLL(_lib.LIB_PATH)
    # (an older build may lack a debug entry point that this tree binds)
    _lib.DEBUG_SIGNATURES = {k: v for k, v in _lib.DEBUG_SIGNATURES.items() if hasattr(handle, k)}
    _lib.lib()
    dev = torch.device("cuda", 0)
    cases = {}
    bad = False
    for key in hc.CASES:
        net = hc.engine_net(dev, key)
        Xn, yn = hc.engine_inputs(key)
        X, y = torch.from_numpy(Xn).to(dev), torch.from_numpy(yn).to(dev)
        hs = [lc.hashes(hc.run(net, key, X, y)[0]) for _ in range(3)]
        moved = sorted(k for k in hs[0] if any(h[k] != hs[0][k] for h in hs[1:]))
        free = hc.UNPINNED.get(key, ())
        if moved and set(moved) <= set(free):
            print(f"{key}: passes differ in the outputs the test leaves unpinned: {moved}", flush=True)
        elif moved:
            print(f"{key}: passes differ in this build: {moved}", file=sys.stderr, flush=True)
            bad = True
        cases[key] = {k: v for k, v in hs[0].items() if k not in free}
        print(key, len(cases[key]), "outputs", flush=True)
    if bad:
        return 1
    doc = {"produced_by": f"commit {args.commit} (the parent of the change that runs round B of layer 2's quad merge, "
                          "the publish of pair hand-off 2, the fetch and the cross-half merge on all sixteen waves), "
                          "bf16 mode, one MI355X",
           "what": "sha256 of the bytes of every output: logits, loss and each gradient after one eager train step",
           "cases": cases}
    with open(args.out, "w") as f:
        json.dump(doc, f, indent=1, sort_keys=True)
        f.write("\n")
    print(f"{len(cases)} cases -> {args.out}")
    return 0


if __name__ == "__main__":
    sys.exit(main())
