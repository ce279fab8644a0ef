#!/usr/bin/env python3
"""Rows per extension DP with and without the row exit (dev_lane_rows.h: ext_row_bound / ext_row_done), on a sample of a bench config's reads, on the CPU.
The jobs: for every kept chain of a read (the checker's chain stage) the extension of its top seed inside the chain's window, as mem_chain2aln
makes it -- exact for one-seed chains (nearly all chains of a read from a repeat) and for the light reads' top-seed jobs; the other seeds of a
chain of several are left out.  A side the diagonal answers (diag_extend's conditions) runs no DP and is dropped.  The row loop is the product's
own, compiled for the host (tests/cpp/ext_row_exit_test.cpp): exit off, strict, relaxed.
  scripts/ext_row_exit_rows.py <index prefix of the config's reference> [config=C3] [reads=100000] [first block=0]
Heavy = a read with at least 64 seed occurrences (the walk's in-place extensions); light = the others (their top-seed jobs)."""
import os
import subprocess
import sys
import tempfile

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from oracle import orc          # noqa: E402
from seqlib_amd import synth    # noqa: E402


def max_gap(opt, qlen):
    l_del = int((qlen * opt.a - opt.o_del) / opt.e_del + 1.)
    l_ins = int((qlen * opt.a - opt.o_ins) / opt.e_ins + 1.)
    return min(max(l_del, l_ins, 1), opt.w << 1)


def diagonal(q, t, h0, oe):
    """diag_extend: None, or the score it reports"""
    if len(t) < len(q) or not 1 <= len(q) <= 192:
        return None
    sc = np.where((q == 4) | (t[:len(q)] == 4), -1, np.where(q == t[:len(q)], 1, -4))
    loss = int((1 - sc).sum())
    if loss > oe - 1 or h0 <= loss:
        return None
    return max(h0, h0 + int(np.cumsum(sc).max()))


def main():
    prefix = sys.argv[1]
    cfg = synth.CONFIGS[sys.argv[2] if len(sys.argv) > 2 else "C3"]
    n = int(sys.argv[3]) if len(sys.argv) > 3 else 100000
    refs = synth.make_reference(cfg)
    g = np.concatenate([c for _, c in refs]).astype(np.uint8)
    assert len(refs) == 1, "one contig: the window's contig clip is the l_pac rule"
    l_pac = len(g)
    both = np.concatenate([g, (3 - g)[::-1]])
    reads = synth.make_config_reads(cfg, refs, n, int(sys.argv[4]) if len(sys.argv) > 4 else 0)
    oidx = orc.Index.load(prefix)
    opt = orc.default_opt()
    oe = min(opt.o_del + opt.e_del, opt.o_ins + opt.e_ins)
    code = np.full(256, 4, dtype=np.uint8)
    for i, ch in enumerate(b"ACGT"):
        code[ch] = i
    dig = lambda v: "".join(map(str, v.tolist())) if len(v) else "-"
    lines, n_heavy, n_jobs = [], 0, {"heavy": 0, "light": 0}
    for r in range(n):
        seq = reads[r].tobytes()
        iv = orc.stage_dump(opt, oidx, seq, 0).reshape(-1, 4)
        heavy = int(np.minimum(iv[:, 3], opt.max_occ).sum()) >= 64
        n_heavy += heavy
        d = orc.stage_dump(opt, oidx, seq, 1)
        c = code[reads[r]]
        lq, at = len(c), 1
        for _ in range(int(d[0])):
            k = int(d[at + 2])
            seeds = d[at + 3:at + 3 + 4 * k].reshape(k, 4)          # rbeg qbeg len score
            at += 3 + 4 * k
            if k == 0:
                continue
            rmax0, rmax1 = l_pac << 1, 0
            for rb, qb, ln, _ in seeds:
                rmax0 = min(rmax0, rb - (qb + max_gap(opt, qb)))
                rmax1 = max(rmax1, rb + ln + ((lq - qb - ln) + max_gap(opt, lq - qb - ln)))
            rmax0, rmax1 = max(rmax0, 0), min(rmax1, l_pac << 1)
            if rmax0 < l_pac < rmax1:
                if seeds[0][0] < l_pac:
                    rmax1 = l_pac
                else:
                    rmax0 = l_pac
            top = max(range(k), key=lambda i: (seeds[i][3], i))
            rb, qb, ln, _ = (int(x) for x in seeds[top])
            h0 = ln * opt.a
            left = (c[:qb][::-1], both[rmax0:rb][::-1]) if qb else None
            qe, re0 = qb + ln, rb + ln
            right = (c[qe:], both[re0:rmax1]) if qe != lq else None
            if left:
                s = diagonal(left[0], left[1], h0, oe)
                if s is not None:
                    left, h0 = None, s
            if right and not left and diagonal(right[0], right[1], h0, oe) is not None:          # (behind a left DP the right side's h0 is not known here: it stays)
                right = None
            if not left and not right:
                continue
            kind = "heavy" if heavy else "light"
            n_jobs[kind] += 1
            e = np.zeros(0, dtype=np.uint8)
            ql, tl = left or (e, e)
            qr, tr = right or (e, e)
            lines.append("%s %d %d %d %d %d %d %s %s %s %s" % (kind, max(len(ql), len(qr)) + 2, h0, opt.w, opt.zdrop, opt.pen_clip5, opt.pen_clip3, dig(ql), dig(tl), dig(qr), dig(tr)))
    print("%d reads, %d heavy; jobs with a DP: %r" % (n, n_heavy, n_jobs))
    with tempfile.TemporaryDirectory() as tmp:
        exe, cases = os.path.join(tmp, "t"), os.path.join(tmp, "cases.txt")
        subprocess.check_call(["g++", "-std=c++17", "-O2", "-o", exe, os.path.join(ROOT, "tests", "cpp", "ext_row_exit_test.cpp")])
        open(cases, "w").write("\n".join(lines) + "\n")
        base = {}
        for mode, name in ((0, "off"), (1, "strict"), (2, "relaxed")):
            out = subprocess.run([exe, "run", cases, str(mode)], stdout=subprocess.PIPE, text=True, check=True).stdout
            for ln in out.split("\n"):
                if ln.startswith("#"):
                    _, kind, ncase, trials, rows, exits = ln.split()
                    rows, trials = int(rows), int(trials)
                    base.setdefault(kind, rows)
                    print("%-8s %-6s %7s jobs %8d DPs %10d rows  %6.1f rows per DP  %6.2f %% of the rows without the exit  %7s DPs ended by the exit" %
                          (name, kind, ncase, trials, rows, rows / max(trials, 1), 100. * rows / max(base[kind], 1), exits))


if __name__ == "__main__":
    main()
