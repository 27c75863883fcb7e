#!/usr/bin/env python3
"""From hipcc -S listings: for every kernel whose demangled name contains one of the given substrings, the
order of global loads, vmcnt waits, LDS stores and barriers from the kernel's entry to its first s_barrier
(runs of the same instruction are counted), and its register / scratch / spill figures.

  hipcc -O3 -std=c++17 --offload-arch=gfx950 -Iinclude -Ipoint-cloud-audio_amd/csrc --cuda-device-only -S \
      point-cloud-audio_amd/csrc/mab0_bwd_bf16.hip -o mab0_bwd_bf16.s
  scripts/experiments/isa_prologue.py mab0_bwd_bf16.s 'k_mab0_bwd<64, true>' 'k_mab0_bwd_small<true>'
"""
import re
import subprocess
import sys


def demangle(sym):
    try:
        return subprocess.run(["c++filt", sym], capture_output=True, text=True, check=True).stdout.strip()
    except (OSError, subprocess.CalledProcessError):
        return sym


def kernels(text):
    """{symbol: (lines of the body, {metadata key: value})}"""
    out = {}
    meta = {}
    for blk in re.split(r"\n\s*- \.agpr_count:", text)[1:]:
        name = re.search(r"\.name:\s+(\S+)", blk)
        if name is None:
            continue
        keys = {k: re.search(r"\.%s:\s+(\d+)" % k, blk) for k in
                ("vgpr_count", "sgpr_count", "vgpr_spill_count", "sgpr_spill_count",
                 "private_segment_fixed_size", "group_segment_fixed_size")}
        meta[name.group(1)] = {k: int(v.group(1)) for k, v in keys.items() if v}
    for sym in meta:
        m = re.search(r"^%s:.*?\n(.*?)^\s*s_endpgm" % re.escape(sym), text, re.S | re.M)
        if m:
            out[sym] = (m.group(1).splitlines(), meta[sym])
    return out


def prologue(lines):
    seq = []
    for ln in lines:
        ln = ln.split(";")[0].strip()
        op = ln.split(" ")[0] if ln else ""
        key = None
        if op.startswith("global_load") or op.startswith("buffer_load"):
            key = op
        elif op.startswith("ds_write") or op.startswith("ds_store"):
            key = op
        elif op == "s_waitcnt" and "vmcnt" in ln:
            key = "s_waitcnt " + re.search(r"vmcnt\(\d+\)", ln).group(0)
        elif op == "s_barrier":
            seq.append([op, 1])
            break
        elif op.startswith("s_cbranch"):
            key = op
        if key is None:
            continue
        if seq and seq[-1][0] == key and not key.startswith("s_"):
            seq[-1][1] += 1
        else:
            seq.append([key, 1])
    return seq


def main():
    path, wanted = sys.argv[1], sys.argv[2:]
    ks = kernels(open(path).read())
    for sym, (lines, meta) in sorted(ks.items()):
        name = demangle(sym)
        if not any(w in name for w in wanted):
            continue
        print(name)
        print("  " + "  ".join(f"{k}={v}" for k, v in meta.items()))
        for key, n in prologue(lines):
            print(f"    {n:3d} x {key}" if n > 1 else f"          {key}")
        print()


if __name__ == "__main__":
    main()
