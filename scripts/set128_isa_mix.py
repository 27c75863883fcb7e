#!/usr/bin/env python3
"""Static instruction mix of k_set128_fwd from hipcc's assembly listing (a record, not a test).

    hipcc -O3 -std=c++17 --offload-arch=gfx950 -S --cuda-device-only \
        -Iinclude -Ipoint-cloud-audio_amd/csrc point-cloud-audio_amd/csrc/set128_fwd.hip -o set128_fwd.s
    python scripts/set128_isa_mix.py set128_fwd.s [--inst 2,2,0 --inst 2,2,1]

Every instruction line of an instance is put into one class by its mnemonic's prefix; global accesses
are further split by their address form (a 64-bit VGPR pair with `off`, or a 32-bit VGPR offset with a
scalar base) and stores by width.  The register / scratch / spill figures of ALL instances come from the
code-object metadata at the end of the listing.
"""
import argparse
import collections
import re
import sys

INT_MOVE = (
    "v_mov_b", "v_add_u32", "v_add_co", "v_addc_co", "v_sub_u32", "v_subrev_u32", "v_sub_co", "v_subb_co",
    "v_add3_u32", "v_lshlrev_b", "v_lshrrev_b", "v_ashrrev_i", "v_lshl_add_u", "v_lshl_or_b32",
    "v_add_lshl_u32", "v_and_b32", "v_or_b32", "v_xor_b32", "v_and_or_b32", "v_or3_b32", "v_bfe_", "v_bfi_b32",
    "v_mul_lo_u32", "v_mul_hi_u32", "v_mul_u32_u24", "v_mul_i32_i24", "v_mad_u64_u32", "v_mad_i64_i32",
    "v_mad_u32_u24", "v_mad_i32_i24", "v_mbcnt", "v_accvgpr", "v_not_b32", "v_xad_u32", "v_add_i32",
    "v_sub_i32", "v_mad_u32_u16", "v_xnor_b32",
)


def instance_label(din, upq, length):
    return re.compile(r"^(_Z\w*k_set128_fwdILi%dELi%dELb%dEE\w*):" % (din, upq, length))


def body_of(lines, pat):
    start = None
    for i, ln in enumerate(lines):
        if start is None:
            if pat.match(ln):
                start = i + 1
        elif ln.startswith(".Lfunc_end"):
            return lines[start:i]
    raise SystemExit("instance not found in the listing")


def instructions(body):
    for ln in body:
        s = ln.split(";", 1)[0].strip()
        if not s or s.startswith(".") or s.endswith(":"):
            continue
        parts = s.split(None, 1)
        yield parts[0], parts[1] if len(parts) > 1 else ""


def mix(body):
    cls = collections.Counter()
    mnem = collections.Counter()
    glob = collections.Counter()
    pair_by = collections.Counter()
    for m, ops in instructions(body):
        cls["all"] += 1
        mnem[m] += 1
        if m.startswith("v_mfma") or m.startswith("v_smfmac"):
            cls["mfma"] += 1
        elif m.startswith("v_"):
            cls["valu"] += 1
            if m.startswith(INT_MOVE):
                cls["valu_int_move"] += 1
        elif m == "s_waitcnt":
            cls["s_waitcnt"] += 1
        elif m == "s_nop":
            cls["s_nop"] += 1
        elif m.startswith("ds_"):
            cls["lds"] += 1
        elif m.startswith("global_") or m.startswith("flat_"):
            cls["global"] += 1
            toks = [t.strip() for t in ops.replace(",", " ").split()]
            if "off" in toks or m.startswith("flat_"):
                cls["global_vgpr_pair"] += 1
                pair_by[m] += 1
            else:
                cls["global_saddr"] += 1
            glob[m] += 1
        elif m.startswith("scratch_") or m.startswith("buffer_"):
            cls["scratch_or_buffer"] += 1
        elif m.startswith("s_load") or m.startswith("s_buffer_load"):
            cls["s_load"] += 1
        elif m.startswith("s_"):
            cls["salu_other"] += 1
        else:
            cls["other"] += 1
    return cls, mnem, glob, pair_by


def report(name, body, out):
    cls, mnem, glob, pair_by = mix(body)
    w = out.write
    w("== %s\n" % name)
    w("  all instructions            %5d\n" % cls["all"])
    w("  v_mfma_*                    %5d\n" % cls["mfma"])
    w("  other VALU                  %5d\n" % cls["valu"])
    w("    integer / move only       %5d (%.0f %%)\n" % (cls["valu_int_move"], 100.0 * cls["valu_int_move"] / max(cls["valu"], 1)))
    top = sorted(((n, m) for m, n in mnem.items() if m.startswith(INT_MOVE)), reverse=True)[:12]
    w("      " + ", ".join("%s %d" % (m, n) for n, m in top) + "\n")
    w("  s_waitcnt / s_nop           %5d / %d\n" % (cls["s_waitcnt"], cls["s_nop"]))
    w("  s_load / other SALU         %5d / %d\n" % (cls["s_load"], cls["salu_other"]))
    w("  LDS                         %5d\n" % cls["lds"])
    w("  scratch / buffer            %5d\n" % cls["scratch_or_buffer"])
    w("  global accesses             %5d\n" % cls["global"])
    w("    64-bit VGPR address pair  %5d  (%s)\n" % (cls["global_vgpr_pair"], ", ".join("%s %d" % kv for kv in sorted(pair_by.items()))))
    w("    scalar base (saddr)       %5d\n" % cls["global_saddr"])
    w("    by mnemonic: " + ", ".join("%s %d" % kv for kv in sorted(glob.items())) + "\n")


def metadata(lines, out):
    """.vgpr_count / spills / scratch of every k_set128_fwd instance (amdhsa.kernels metadata)."""
    cur = {}
    rows = []
    for ln in lines:
        s = ln.strip()
        m = re.match(r"^-?\s*\.(\w+):\s*(.*)$", s)
        if not m:
            continue
        k, v = m.group(1), m.group(2).strip("'\" ")
        if k in ("agpr_count", "vgpr_count", "sgpr_count", "sgpr_spill_count", "vgpr_spill_count",
                 "private_segment_fixed_size", "group_segment_fixed_size"):
            cur[k] = v
        elif k == "name" and "k_set128_fwd" in v:
            cur["name"] = v
        elif k == "wavefront_size":             # the last key of a kernel's record
            if "name" in cur:
                rows.append(cur)
            cur = {}
    out.write("== code objects (DIN, UPQ, LEN): vgpr agpr sgpr | scratch bytes | vgpr spills | sgpr spills\n")
    for r in sorted(rows, key=lambda r: r.get("name", "")):
        t = re.search(r"ILi(\d)ELi(\d)ELb(\d)E", r.get("name", ""))
        tag = "<%s,%s,%s>" % t.groups() if t else r.get("name", "?")
        out.write("  %-9s %4s %3s %4s | %s | %s | %s\n" % (
            tag, r.get("vgpr_count", "?"), r.get("agpr_count", "?"), r.get("sgpr_count", "?"),
            r.get("private_segment_fixed_size", "?"), r.get("vgpr_spill_count", "?"), r.get("sgpr_spill_count", "?")))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("listing")
    ap.add_argument("--inst", action="append", default=None, help="DIN,UPQ,LEN (default: 2,2,0 and 2,2,1)")
    a = ap.parse_args()
    lines = open(a.listing).read().splitlines()
    for inst in a.inst or ["2,2,0", "2,2,1"]:
        din, upq, length = (int(x) for x in inst.split(","))
        report("k_set128_fwd<%d, %d, %s>" % (din, upq, "true" if length else "false"),
               body_of(lines, instance_label(din, upq, length)), sys.stdout)
    metadata(lines, sys.stdout)


if __name__ == "__main__":
    main()
