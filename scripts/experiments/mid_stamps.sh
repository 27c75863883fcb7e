#!/bin/bash
# On a machine with the GPU: phase stamps of the backward mid chain in the prologue of its carrying kernels
# (csrc/mid_bwd_body.hpp names the phases), cfg2, eager steps.  The diagnostic library is built into a
# directory of its own and swapped in for the measurement; the product library is restored on every exit path.
#   usage (from the repository root): scripts/experiments/mid_stamps.sh [set ...]
set -e
D=point-cloud-audio_amd/pca_hip
T=$(mktemp -d)
cp $D/libpca_hip.so $T/lib_keep.so
trap 'cp $T/lib_keep.so $D/libpca_hip.so; rm -rf $T' EXIT
PCA_EXTRA_FLAGS="-DPCA_DEBUG_CLOCKS" PCA_BUILD_DIR=$T/build PCA_OUT=$T/libpca_clocks.so \
  bash point-cloud-audio_amd/csrc/build.sh > /dev/null
cp $T/libpca_clocks.so $D/libpca_hip.so
for set in "${@:-0}"; do
  PCA_DBG_WG=$set timeout -k 10 150 python bench.py --steps 3 --warmup 2 --windows 1 --no-graph 2>&1 >/dev/null |
    grep "mid chain stamps" | sed "s/^/set $set: /"
done
