#!/usr/bin/env python3
"""Record tests/golden/mab1_bwd_wide_sha256.json: the SHA-256 of logits, loss and each gradient of the cases of
tests/test_gpu_mab1_bwd_wide.py, from a given build of libpca_hip.so (the parent commit's, built into a directory
of its own with PCA_BUILD_DIR / PCA_OUT).  One fresh process:

  python scripts/mab1_bwd_wide_golden.py --lib PARENT.so --commit SHA --out tests/golden/mab1_bwd_wide_sha256.json

Before anything is recorded the CPU oracle of every case must be finite and its loss away from both 0 and the
uniform guess ln C; three passes of the given build must agree on every output; and for the cases that the test
runs again in two surroundings (X inside a NaN tensor, the workspace filled with 0xFF bytes) the given build must
give the same hashes there, so that what the test then asks of a later build is what its parent did.

A case that the given build refuses (dim_input = 1, if it does) is reported and left out."""
import argparse
import ctypes
import json
import math
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (os.path.join(ROOT, "point-cloud-audio_amd"), os.path.join(ROOT, "tests", "golden"),
          os.path.join(ROOT, "tests"), ROOT):
    sys.path.insert(0, p)


def oracle_is_sound():
    """The CPU side alone (no GPU needed: --check-oracle)."""
    import torch
    import mab1_bwd_wide_cases as wc
    ok = True
    cpu = torch.device("cpu")
    for key in wc.CASES:
        Xn, yn = wc.engine_inputs(key)
        loss, lg, g = wc.oracle(wc.engine_net(cpu, key), key, Xn, yn)
        fin = bool(torch.isfinite(lg).all()) and all(bool(torch.isfinite(v).all()) for v in g.values())
        live = all(float(v.abs().max()) > 0 for k, v in g.items() if not k.endswith("fc_k.bias"))
        sound = fin and live and math.isfinite(loss) and 0.05 < loss and abs(loss - math.log(wc.C)) > 1e-3
        print(f"{key}: oracle loss {loss:.4f} (ln C = {math.log(wc.C):.4f}), finite {fin}, every gradient non-zero "
              f"{live}", flush=True)
        ok = ok and sound
    return ok


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--lib")
    ap.add_argument("--commit")
    ap.add_argument("--out")
    ap.add_argument("--check-oracle", action="store_true", help="only the CPU checks of the cases")
    args = ap.parse_args()
    if not oracle_is_sound():
        print("a case's oracle is not finite or its loss is degenerate", file=sys.stderr)
        return 1
    if args.check_oracle:
        return 0
    if not (args.lib and args.commit and args.out):
        ap.error("--lib, --commit and --out are required")
    import torch
    import mab1_bwd_loads_cases as lc
    import mab1_bwd_wide_cases as wc
    from pca_hip import _lib
    _lib.LIB_PATH = os.path.abspath(args.lib)
    handle = ctypes.CDLL(_lib.LIB_PATH)
    # (an older build may lack a debug entry point that this tree binds)
    _lib.DEBUG_SIGNATURES = {k: v for k, v in _lib.DEBUG_SIGNATURES.items() if hasattr(handle, k)}
    _lib.lib()
    dev = torch.device("cuda", 0)
    cases = {}
    refused = {}
    bad = False
    for key in wc.CASES:
        net = wc.engine_net(dev, key)
        Xn, yn = wc.engine_inputs(key)
        X, y = torch.from_numpy(Xn).to(dev), torch.from_numpy(yn).to(dev)
        try:
            hs = [lc.hashes(wc.run(net, key, X, y)[0]) for _ in range(3)]
        except _lib.PcaHipError as e:
            refused[key] = str(e)
            print(f"{key}: refused by this build: {e}", flush=True)
            continue
        moved = sorted(k for k in hs[0] if any(h[k] != hs[0][k] for h in hs[1:]))
        if moved:
            print(f"{key}: passes differ in this build: {moved}", file=sys.stderr, flush=True)
            bad = True
        if key in wc.SURROUNDED:
            Xs, keep = wc.surrounded(Xn, dev)
            for what, h in (("X surrounded by NaN", lc.hashes(wc.run(net, key, Xs, y)[0])),
                            ("workspace filled", lc.hashes(wc.run(net, key, X, y, fill_ws=True)[0]))):
                diff = sorted(k for k in hs[0] if h[k] != hs[0][k])
                print(f"{key}: {what}: {'same hashes' if not diff else 'DIFFERENT: %s' % diff}", flush=True)
                bad = bad or bool(diff)
            del keep
        cases[key] = hs[0]
        print(key, len(cases[key]), "outputs", flush=True)
    if bad:
        return 1
    doc = {"produced_by": f"commit {args.commit} (the parent of the change to k_mab1_bwd's tile loads and stores), "
                          "bf16 mode, one MI355X",
           "what": "sha256 of the bytes of every output: logits, loss and each gradient after one eager train step",
           "refused": refused,
           "cases": cases}
    with open(args.out, "w") as f:
        json.dump(doc, f, indent=1, sort_keys=True)
        f.write("\n")
    print(f"{len(cases)} cases -> {args.out}")
    return 0


if __name__ == "__main__":
    sys.exit(main())
