#!/usr/bin/env python3
"""Record tests/golden/optim_digest_sha256.json: the SHA-256 of what three launches of each optimiser entry
point leave behind, for the cases of tests/optim_digest_cases.py, from a given build of libpca_hip.so (the
parent commit's, built into a directory of its own with PCA_BUILD_DIR / PCA_OUT).  One fresh process:

  python scripts/optim_digest_golden.py --lib PARENT.so --commit SHA --out tests/golden/optim_digest_sha256.json

Refuses to write unless, in that build, two eager repeats of every case agree and every guarded case with
n > 0 shows one clipped and one skipped step in its state words (so the three launches held a clip factor
below 1, a factor of exactly 1 and a skip)."""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (os.path.join(ROOT, "point-cloud-audio_amd"), os.path.join(ROOT, "tests"), ROOT):
    sys.path.insert(0, p)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--lib", required=True)
    ap.add_argument("--commit", required=True)
    ap.add_argument("--out", required=True)
    args = ap.parse_args()
    import torch
    import optim_digest_cases as oc
    from pca_hip import _lib
    _lib.LIB_PATH = os.path.abspath(args.lib)
    _lib.lib()
    dev = torch.device("cuda", 0)
    cases = {}
    for n in oc.SIZES:
        for variant in oc.VARIANTS:
            for offset in oc.OFFSETS:
                for zg in oc.ZERO_GRAD:
                    k = oc.key(n, offset, zg, variant)
                    h1, state = oc.run_case(dev, n, offset, zg, variant)
                    h2, _ = oc.run_case(dev, n, offset, zg, variant)
                    if h1 != h2:
                        print(f"{k}: two eager repeats differ in this build", file=sys.stderr)
                        return 1
                    skipped, clipped = state[0], state[1]
                    want = (1, 1) if variant in oc.GUARDED and n > 0 else (0, 0)
                    if (skipped, clipped) != want:
                        print(f"{k}: skipped={skipped} clipped={clipped}, the case needs {want}", file=sys.stderr)
                        return 1
                    cases[k] = h1
            print(n, variant, cases[oc.key(n, 0, 0, variant)][:16], flush=True)
    doc = {"produced_by": f"commit {args.commit} (the parent of the one-translation-unit optimiser), one MI355X",
           "what": "sha256 of the bytes of p, g, m, v, the averaged copy where there is one, the two step words "
                   "and the eight state words after three eager launches",
           "cases": cases}
    with open(args.out, "w") as f:
        json.dump(doc, f, indent=1, sort_keys=True)
        f.write("\n")
    print(f"{len(cases)} cases -> {args.out}")
    return 0


if __name__ == "__main__":
    sys.exit(main())
