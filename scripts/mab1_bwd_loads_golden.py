#!/usr/bin/env python3
"""Record tests/golden/mab1_bwd_loads_sha256.json: the SHA-256 of every output (logits, loss and each gradient of
the engine cases; Y and each gradient of the module cases) of the cases of tests/test_gpu_mab1_bwd_loads.py, from
a given build of libpca_hip.so (the parent commit's, built into a directory of its own with PCA_BUILD_DIR /
PCA_OUT).  One fresh process:

  python scripts/mab1_bwd_loads_golden.py --lib PARENT.so --commit SHA --out tests/golden/mab1_bwd_loads_sha256.json

Before anything is recorded the CPU oracle of every case must be finite and its loss away from both 0 and the
uniform guess ln C (a degenerate case pins nothing); three passes of the given build must agree as well, on every
output but the ones tests/mab1_bwd_loads_cases.py lists as summed by fp32 atomics (UNPINNED: not recorded)."""
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
    import mab1_bwd_loads_cases as lc
    ok = True
    cpu = torch.device("cpu")
    for key in lc.ENGINE:
        Xn, yn = lc.engine_inputs(key)
        loss, lg, g = lc.engine_oracle(lc.engine_net(cpu, key), key, Xn, yn)
        fin = bool(torch.isfinite(lg).all()) and all(bool(torch.isfinite(v).all()) for v in g.values())
        live = all(float(v.abs().max()) > 0 for k, v in g.items() if not k.endswith("fc_k.bias"))
        sound = fin and live and math.isfinite(loss) and 0.05 < loss and abs(loss - math.log(lc.C)) > 1e-3
        print(f"{key}: oracle loss {loss:.4f} (ln C = {math.log(lc.C):.4f}), finite {fin}, every gradient non-zero "
              f"{live}", flush=True)
        ok = ok and sound
    for key in lc.MODULE:
        ref = lc.module_oracle(key)
        fin = all(bool(torch.isfinite(v).all()) for v in ref.values())
        live = all(float(v.abs().max()) > 0 for k, v in ref.items() if k != "fc_k.bias")
        print(f"{key}: oracle finite {fin}, every output non-zero {live}", flush=True)
        ok = ok and fin and live
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
    from pca_hip import _lib
    _lib.LIB_PATH = os.path.abspath(args.lib)
    handle = ctypes.CDLL(_lib.LIB_PATH)
    # (an older build may lack a debug entry point that this tree binds)
    _lib.DEBUG_SIGNATURES = {k: v for k, v in _lib.DEBUG_SIGNATURES.items() if hasattr(handle, k)}
    _lib.lib()
    dev = torch.device("cuda", 0)
    cases = {}
    bad = False

    def record(key, run):
        """Three passes of the given build: all outputs but the case's unpinned ones (sums by fp32 atomics) must
        have the same bits each time."""
        nonlocal bad
        hs = [lc.hashes(run()) for _ in range(3)]
        moved = sorted(k for k in hs[0] if any(h[k] != hs[0][k] for h in hs[1:]))
        free = lc.UNPINNED.get(key, ())
        if any(k not in free for k in moved):
            print(f"{key}: passes differ in this build: {moved}", file=sys.stderr, flush=True)
            bad = True
        cases[key] = {k: v for k, v in hs[0].items() if k not in free}
        print(key, len(cases[key]), "outputs", "(differing between passes: %s)" % moved if moved else "", flush=True)

    for key in lc.ENGINE:
        net = lc.engine_net(dev, key)
        Xn, yn = lc.engine_inputs(key)
        X, y = torch.from_numpy(Xn).to(dev), torch.from_numpy(yn).to(dev)
        record(key, lambda: lc.engine_run(net, key, X, y)[0])
    for key in lc.MODULE:
        record(key, lambda: lc.module_run(dev, key)[0])
    if bad:
        return 1
    doc = {"produced_by": f"commit {args.commit} (the parent of the change to k_mab1_bwd's loads), bf16 mode, "
                          "one MI355X",
           "what": "sha256 of the bytes of every output: logits, loss and each gradient after one eager train step "
                   "(engine cases); Y, dK, dQ where asked for, and each parameter gradient of one MAB (module cases)",
           "cases": cases}
    with open(args.out, "w") as f:
        json.dump(doc, f, indent=1, sort_keys=True)
        f.write("\n")
    print(f"{len(cases)} cases -> {args.out}")
    return 0


if __name__ == "__main__":
    sys.exit(main())
