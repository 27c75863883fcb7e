#!/usr/bin/env python3
"""From hipcc -S listings: for every kernel whose demangled name contains one of the given substrings, the
order of global loads, vmcnt waits, LDS stores and barriers from the kernel's entry to its first s_barrier
(runs of the same instruction are counted), and its register / scratch / spill figures.

  hipcc -O3 -std=c++17 --offload-arch=gfx950 -Iinclude -Ipoint-cloud-audio_amd/csrc --cuda-device-only -S \
      point-cloud-audio_amd/csrc/mab0_bwd_bf16.hip -o mab0_bwd_bf16.s
  scripts/experiments/isa_prologue.py mab0_bwd_bf16.s 'k_mab0_bwd<64, true>' 'k_mab0_bwd_small<true>'

--to-mfma  for kernels whose loads lie behind more than one barrier (k_mab1_bwd: the weight images, the K / V images,
           then the tile): the sequence from the entry to the first MFMA, barriers included, and on through the
           MFMA phases - there only global loads, vmcnt waits, global stores, scratch traffic and the runs of
           MFMAs - to the first s_barrier behind them (k_mab1_bwd: through the head loop and the dX stage)
--counts   no sequence: one line per kernel with its global loads, vmcnt waits, vmcnt(0) waits, the vmcnt(0)
           waits that have a global load among the 8 instructions in front of them (a load waited for where it
           was issued: a serial round trip), the global loads and the global stores by width (4 / 8 / 12 / 16 bytes
           per lane; narrower ones count as 4), VGPRs and scratch bytes
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


def ops(lines):
    """(mnemonic, text without the comment) of every instruction line"""
    out = []
    for ln in lines:
        ln = ln.split(";")[0].strip()
        if not ln or ln.endswith(":") or ln.startswith("."):
            continue
        out.append((ln.split(" ")[0], ln))
    return out


def is_gload(op):
    return op.startswith("global_load") or op.startswith("buffer_load")


def to_mfma(lines):
    seq = []
    seen_mfma = False
    for op, ln in ops(lines):
        key = None
        if is_gload(op) or op.startswith("global_store") or op.startswith("scratch_"):
            key = op
        elif op.startswith("v_mfma"):
            key, seen_mfma = "v_mfma", True
        elif (op.startswith("ds_write") or op.startswith("ds_store")) and not seen_mfma:
            key = op
        elif op == "s_waitcnt" and "vmcnt" in ln:
            key = "s_waitcnt " + re.search(r"vmcnt\(\d+\)", ln).group(0)
        elif op == "s_barrier":
            seq.append([op, 1])
            if seen_mfma:
                break
            continue
        elif op.startswith("s_cbranch") and not seen_mfma:
            key = op
        if key is None:
            continue
        if seq and seq[-1][0] == key and not key.startswith("s_"):
            seq[-1][1] += 1
        else:
            seq.append([key, 1])
    return seq


def counts(lines):
    ins = ops(lines)
    loads = sum(is_gload(op) for op, _ in ins)
    waits = [i for i, (op, ln) in enumerate(ins) if op == "s_waitcnt" and "vmcnt" in ln]
    full = [i for i in waits if "vmcnt(0)" in ins[i][1]]
    behind = sum(any(is_gload(op) for op, _ in ins[max(0, i - 8):i]) for i in full)
    return loads, len(waits), len(full), behind


def by_width(lines, kind):
    """Global `kind` ("load" / "store") instructions by bytes per lane: "n4/n8/n12/n16"."""
    n = {4: 0, 8: 0, 12: 0, 16: 0}
    for op, _ in ops(lines):
        if not (op.startswith("global_" + kind) or op.startswith("buffer_" + kind)) or "lds" in op:
            continue
        w = re.search(r"dwordx(\d)", op)
        n[4 * int(w.group(1)) if w else 4] += 1
    return "/".join(str(n[k]) for k in (4, 8, 12, 16))


def main():
    flags = [a for a in sys.argv[1:] if a.startswith("--")]
    rest = [a for a in sys.argv[1:] if not a.startswith("--")]
    path, wanted = rest[0], rest[1:]
    ks = kernels(open(path).read())
    listing = to_mfma if "--to-mfma" in flags else prologue
    if "--counts" in flags:
        print(f"{'global loads':>12} {'vmcnt waits':>11} {'vmcnt(0)':>8} {'(0) <= 8 behind a load':>22} "
              f"{'loads 4/8/12/16 B':>17} {'stores 4/8/12/16 B':>18} {'VGPRs':>5} {'scratch B':>9}  kernel")
    for sym, (lines, meta) in sorted(ks.items(), key=lambda kv: demangle(kv[0])):
        name = demangle(sym)
        if wanted and not any(w in name for w in wanted):
            continue
        if "--counts" in flags:
            lo, wa, fu, be = counts(lines)
            short = re.sub(r"\(.*$", "", name.replace("(anonymous namespace)::", "").replace("void ", ""))
            print(f"{lo:12d} {wa:11d} {fu:8d} {be:22d} {by_width(lines, 'load'):>17} {by_width(lines, 'store'):>18} "
                  f"{meta.get('vgpr_count', -1):5d} "
                  f"{meta.get('private_segment_fixed_size', -1):9d}  {short}")
            continue
        print(name)
        print("  " + "  ".join(f"{k}={v}" for k, v in meta.items()))
        for key, n in listing(lines):
            print(f"    {n:3d} x {key}" if n > 1 else f"          {key}")
        print()


if __name__ == "__main__":
    main()
