#!/usr/bin/env python3
"""Record tests/golden/prep_rebuild_sha256.json: the SHA-256 of every pinned output of the cases of
tests/test_gpu_prep_rebuild.py (tests/prep_rebuild_cases.py), from a given build of libpca_hip.so - the parent
commit's, built into a directory of its own with PCA_BUILD_DIR / PCA_OUT.  One fresh process:

  python scripts/prep_rebuild_golden.py --lib PARENT.so --commit SHA --out tests/golden/prep_rebuild_sha256.json

Two passes of the given build must agree on every pinned output before anything counts as recorded; a tensor that
moves between them is named in the file ("differs_between_passes") and the script fails."""
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
    import prep_rebuild_cases as pc
    from pca_hip import _lib
    _lib.LIB_PATH = os.path.abspath(args.lib)
    handle = ctypes.CDLL(_lib.LIB_PATH)
    # (an older build lacks the debug entry points that this tree binds)
    _lib.DEBUG_SIGNATURES = {k: v for k, v in _lib.DEBUG_SIGNATURES.items() if hasattr(handle, k)}
    _lib.lib()
    dev = torch.device("cuda", 0)
    cases, moved = {}, {}
    for key in pc.CASES:
        a, b = pc.hashes(pc.run(dev, key)), pc.hashes(pc.run(dev, key))
        assert a.keys() == b.keys() and "logits" in a and ("loss" in a or pc.CASES[key][0] == "forward")
        diff = sorted(k for k in a if a[k] != b[k])
        if diff:
            moved[key] = diff
            print(f"{key}: passes of this build differ in {diff}", file=sys.stderr, flush=True)
        cases[key] = a
        print(key, len(a), "outputs", flush=True)
    doc = {"produced_by": f"commit {args.commit} (the parent of the preparation plan), bf16 mode, one MI355X",
           "what": "sha256 of the bytes of every pinned output of a case: logits, loss and each gradient (the "
                   "Trainer case: after three replayed steps, with the packed batch, its labels and the parameters)",
           "cases": cases}
    if moved:
        doc["differs_between_passes"] = moved
    with open(args.out, "w") as f:
        json.dump(doc, f, indent=1, sort_keys=True)
        f.write("\n")
    print(f"{len(cases)} cases -> {args.out}")
    return 1 if moved else 0


if __name__ == "__main__":
    sys.exit(main())
