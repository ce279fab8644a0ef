#!/usr/bin/env python3
"""Memory instructions per function of a device assembly listing, and the resources of its kernels.

    hipcc <the build's flags> --cuda-device-only -S seqlib_amd/csrc/slx_align.hip -o align.s
    scripts/asm_mem_counts.py align.s dev_fin_regs dev_chain_read_coop k_regs_wave k_chain_coop

Every function or kernel whose demangled name contains one of the given words gets one row: how many flat / LDS / scratch / global
loads and stores it holds and how many full drains (a wait for both the vector-memory and the LDS counter at zero).  Kernels also get
their registers, private segment, LDS and the waves per CU these allow (gfx950: 512 VGPRs per lane and SIMD, 160 KB of LDS, 8 waves per
SIMD at the most; a 64-thread block is one wave).  (profiles/NOTES_lds_tables.md has the tables made with it.)"""
import re
import subprocess
import sys


def demangle(names):
    try:
        out = subprocess.run(["c++filt"], input="\n".join(names), capture_output=True, text=True, check=True).stdout.split("\n")
        return dict(zip(names, out))
    except Exception:
        return {n: n for n in names}


COLS = (("flat_ld", r"^\s*flat_load"), ("flat_st", r"^\s*flat_(store|atomic)"), ("ds_rd", r"^\s*ds_(read|load)"), ("ds_wr", r"^\s*ds_(write|store)"),
        ("scr_ld", r"^\s*scratch_load"), ("scr_st", r"^\s*scratch_store"), ("glb_ld", r"^\s*global_load"), ("glb_st", r"^\s*global_(store|atomic)"),
        ("drain", r"^\s*s_waitcnt vmcnt\(0\) lgkmcnt\(0\)"), ("vm0", r"^\s*s_waitcnt vmcnt\(0\)"))


def main():
    path, words = sys.argv[1], sys.argv[2:]
    funcs, cur, meta, kern = {}, None, {}, None
    for line in open(path, errors="replace"):
        m = re.match(r"^(_Z\w+|\w+):\s*(;.*)?$", line)
        if m and not line.startswith(".L"):
            cur = m.group(1)
            funcs.setdefault(cur, dict((c, 0) for c, _ in COLS))
            continue
        if re.match(r"^\s*\.amdhsa_kernel\s+(\S+)", line):
            kern = line.split()[1]
            meta[kern] = {}
            continue
        if kern:
            m = re.match(r"^\s*\.amdhsa_(next_free_vgpr|next_free_sgpr|accum_offset|private_segment_fixed_size|group_segment_fixed_size)\s+(\d+)", line)
            if m:
                meta[kern][m.group(1)] = int(m.group(2))
            if ".end_amdhsa_kernel" in line:
                kern = None
            continue
        if cur and re.match(r"^\s*s_endpgm|^\s*s_setpc_b64", line):
            pass
        if cur:
            for c, rx in COLS:
                if re.match(rx, line):
                    funcs[cur][c] += 1
    dm = demangle(list(funcs))
    print("%-78s " % "function" + " ".join("%7s" % c for c, _ in COLS) + "   vgpr  priv_B  lds_B  waves/CU")
    for f in funcs:
        name = dm.get(f, f)
        if words and not any(w in name for w in words):
            continue
        row = "%-78s " % re.sub(r"\(.*", "", name)[:78] + " ".join("%7d" % funcs[f][c] for c, _ in COLS)
        if f in meta:
            k = meta[f]
            v = k.get("next_free_vgpr", 0)
            lds = k.get("group_segment_fixed_size", 0)
            by_v = min(8, 512 // max(8, (v + 7) // 8 * 8))
            by_l = (160 * 1024) // lds if lds else 32
            row += "  %5d %7d %6d  %d" % (v, k.get("private_segment_fixed_size", 0), lds, min(4 * by_v, by_l))
        print(row)


if __name__ == "__main__":
    main()
