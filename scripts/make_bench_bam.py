#!/usr/bin/env python3
"""Writes the input of tools/bamread_bench.cpp: a BAM of synthetic 150 bp records with qualities, BGZF members of 0xff00 bytes deflated at level 6
(zlib, one process per slice of members).  The reads are windows of a reference FASTA (default tests/golden/tiny.fa) with 1 % substitutions, half of
them reverse-complemented, stored as unmapped records -- so the same file feeds BWAAligner::alignSequences(BamReader&) with that reference's index.
--sorted writes the coordinate-sorted variant tools/bamregion_bench.cpp takes: the same windows as mapped records (150M, 0x10 on half of them) at the
place they were cut from, in (reference, position) order; --shuffled writes the same mapped records in random order (SO:unsorted), the input of
tools/bamsort_bench.cpp; without either option the output is what it always was.  --pairs (with --shuffled) turns the first half of every slice of records
into read pairs -- two neighbours share a name, 0x1 | 0x40 | 0x20 forward and 200 bp upstream, 0x1 | 0x80 | 0x10 reverse -- and lets every tenth pair and
every tenth fragment take the place and strand of the one before it: the input of tools/bammarkdup_bench.cpp, about 10 % duplicates.

    python scripts/make_bench_bam.py out.bam [--records 2000000] [--ref tests/golden/tiny.fa] [--procs 8] [--seed 1] [--sorted | --shuffled [--pairs]]
"""
import argparse
import os
import struct
import sys
import zlib
from concurrent.futures import ProcessPoolExecutor

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EOF_BLOCK = bytes([0x1f, 0x8b, 8, 4, 0, 0, 0, 0, 0, 0xff, 6, 0, 0x42, 0x43, 2, 0, 0x1b, 0, 3, 0, 0, 0, 0, 0, 0, 0, 0, 0])
L = 150


def member(payload):
    c = zlib.compressobj(6, zlib.DEFLATED, -15)
    comp = c.compress(payload) + c.flush()
    return (bytes([0x1f, 0x8b, 8, 4, 0, 0, 0, 0, 0, 0xff, 6, 0, 0x42, 0x43, 2, 0]) + struct.pack("<H", 18 + len(comp) + 8 - 1) + comp +
            struct.pack("<II", zlib.crc32(payload) & 0xffffffff, len(payload)))


def members(data):
    return b"".join(member(data[i:i + 0xff00]) for i in range(0, len(data), 0xff00))


def records(n, first, ref, rng):
    """n fixed-size records as one uint8 array"""
    name_w = 10                                          # 'r' + 8 digits + NUL
    size = 4 + 32 + name_w + (L + 1) // 2 + L
    a = np.zeros((n, size), dtype=np.uint8)
    core = np.frombuffer(struct.pack("<IiiBBHHHiiii", size - 4, -1, -1, name_w, 0, 4680, 0, 4, L, -1, -1, 0), dtype=np.uint8)
    a[:, :36] = core
    ids = np.arange(first, first + n)
    a[:, 36] = ord("r")
    for d in range(8):
        a[:, 37 + d] = 48 + (ids // 10 ** (7 - d)) % 10
    start = rng.integers(0, len(ref) - L, size=n)
    codes = ref[start[:, None] + np.arange(L)[None, :]]                  # 0..3
    sub = rng.random((n, L)) < 0.01
    codes = np.where(sub, (codes + rng.integers(1, 4, size=(n, L))) & 3, codes)
    rev = rng.random(n) < 0.5
    codes = np.where(rev[:, None], 3 - codes[:, ::-1], codes)
    nib = (1 << codes).astype(np.uint8)                                  # A 1, C 2, G 4, T 8
    a[:, 36 + name_w:36 + name_w + L // 2] = (nib[:, 0::2] << 4) | nib[:, 1::2]
    q = np.clip(rng.normal(34, 5, size=(n, L)) - np.arange(L)[None, :] * 0.04, 2, 40).astype(np.uint8)       # high, drifting down along the read
    a[:, 36 + name_w + L // 2:] = q
    return a


def reg2bin(beg, end):
    """SAMv1 5.3 over arrays"""
    end = end - 1
    out = np.zeros(len(beg), dtype=np.int64)
    for sh, base in ((26, 1), (23, 9), (20, 73), (17, 585), (14, 4681)):          # coarse to fine: the finest level that holds the span wins
        out = np.where(beg >> sh == end >> sh, base + (beg >> sh), out)
    return out


def placed_records(first, ref, rng, tid, pos):
    """the records of the sorted variant: one per (tid, pos), mapped with CIGAR 150M, half of them flagged 0x10 (the stored bases are the forward strand's)"""
    n, name_w = len(pos), 10
    size = 4 + 32 + name_w + 4 + (L + 1) // 2 + L
    a = np.zeros((n, size), dtype=np.uint8)
    a[:, :36] = np.frombuffer(struct.pack("<IiiBBHHHiiii", size - 4, 0, 0, name_w, 60, 0, 1, 0, L, -1, -1, 0), dtype=np.uint8)
    a[:, 4:8] = tid.astype("<i4").view(np.uint8).reshape(n, 4)
    a[:, 8:12] = pos.astype("<i4").view(np.uint8).reshape(n, 4)
    a[:, 14:16] = reg2bin(pos.astype(np.int64), pos.astype(np.int64) + L).astype("<u2").view(np.uint8).reshape(n, 2)
    a[:, 18] = np.where(rng.random(n) < 0.5, 16, 0)
    ids = np.arange(first, first + n)
    a[:, 36] = ord("r")
    for d in range(8):
        a[:, 37 + d] = 48 + (ids // 10 ** (7 - d)) % 10
    a[:, 36 + name_w:40 + name_w] = np.frombuffer(struct.pack("<I", L << 4), dtype=np.uint8)
    return a, 40 + name_w


def pair_up(a, rng):
    """--pairs, in place: records 2k and 2k + 1 of the first half become a pair, and every tenth pair and fragment a duplicate of its predecessor"""
    n = len(a)
    k = n // 4
    first, second = np.arange(0, 2 * k, 2), np.arange(1, 2 * k, 2)
    pos = a[:, 8:12].copy().view("<i4").reshape(n)
    a[second, 4:8] = a[first, 4:8]
    a[second, 36:46] = a[first, 36:46]
    pos[second] = pos[first]
    pos[first] = np.maximum(pos[first] - 200, 0)
    a[first, 18] = 0x1 | 0x40 | 0x20
    a[second, 18] = 0x1 | 0x80 | 0x10
    for j in np.nonzero(rng.random(k) < 0.1)[0]:
        if j:
            a[2 * j, 4:8] = a[2 * j - 2, 4:8]; a[2 * j + 1, 4:8] = a[2 * j - 2, 4:8]
            pos[2 * j] = pos[2 * j - 2]; pos[2 * j + 1] = pos[2 * j - 1]
    for i in 2 * k + 1 + np.nonzero(rng.random(n - 2 * k - 1) < 0.1)[0]:
        a[i, 4:8] = a[i - 1, 4:8]; a[i, 18] = a[i - 1, 18]
        pos[i] = pos[i - 1]
    a[:, 8:12] = pos.astype("<i4").view(np.uint8).reshape(n, 4)
    a[:, 14:16] = reg2bin(pos.astype(np.int64), pos.astype(np.int64) + L).astype("<u2").view(np.uint8).reshape(n, 2)


def slice_job(args):
    if len(args) >= 6:
        n, first, ref, seed, tid, start = args[:6]
        rng = np.random.default_rng(seed)
        a, so = placed_records(first, ref, rng, tid, start[1])
        if len(args) == 7 and args[6]:
            pair_up(a, rng)
        codes = ref[start[0][:, None] + np.arange(L)[None, :]]
        codes = np.where(rng.random((n, L)) < 0.01, (codes + rng.integers(1, 4, size=(n, L))) & 3, codes)
        nib = (1 << codes).astype(np.uint8)
        a[:, so:so + L // 2] = (nib[:, 0::2] << 4) | nib[:, 1::2]
        a[:, so + L // 2:] = np.clip(rng.normal(34, 5, size=(n, L)), 2, 40).astype(np.uint8)
        return members(a.tobytes())
    n, first, ref, seed = args
    return members(records(n, first, ref, np.random.default_rng(seed)).tobytes())


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("out")
    ap.add_argument("--records", type=int, default=2000000)
    ap.add_argument("--ref", default=os.path.join(ROOT, "tests", "golden", "tiny.fa"))
    ap.add_argument("--procs", type=int, default=8)
    ap.add_argument("--seed", type=int, default=1)
    ap.add_argument("--sorted", action="store_true", help="mapped records in coordinate order (the input of tools/bamregion_bench.cpp)")
    ap.add_argument("--shuffled", action="store_true", help="the mapped records of --sorted in random order (the input of tools/bamsort_bench.cpp)")
    ap.add_argument("--pairs", action="store_true", help="with --shuffled: half of the records in pairs, about 10 %% duplicates (the input of tools/bammarkdup_bench.cpp)")
    o = ap.parse_args()
    if o.pairs and not o.shuffled:
        ap.error("--pairs goes with --shuffled")
    names, seqs = [], []
    for ln in open(o.ref):
        if ln.startswith(">"):
            names.append(ln[1:].split()[0]); seqs.append([])
        else:
            seqs[-1].append(ln.strip().upper())
    seqs = ["".join(s) for s in seqs]
    lut = np.zeros(256, dtype=np.uint8)
    for i, c in enumerate("ACGT"):
        lut[ord(c)] = i
    ref = lut[np.frombuffer("".join(seqs).encode(), dtype=np.uint8)]
    text = "@HD\tVN:1.6\tSO:%s\n" % ("coordinate" if o.sorted and not o.shuffled else "unsorted") + "".join("@SQ\tSN:%s\tLN:%d\n" % (n, len(s)) for n, s in zip(names, seqs))
    hdr = b"BAM\1" + struct.pack("<I", len(text)) + text.encode() + struct.pack("<I", len(names))
    for n, s in zip(names, seqs):
        hdr += struct.pack("<I", len(n) + 1) + n.encode() + b"\0" + struct.pack("<I", len(s))
    per = 200000                                         # records per job
    jobs = [(min(per, o.records - f), f, ref, o.seed * 100003 + f) for f in range(0, o.records, per)]
    if o.sorted or o.shuffled:
        # places in the concatenated reference, in order; a window that would cross into the next sequence is pulled back to end with its own
        ends = np.cumsum([len(s) for s in seqs])
        g = np.sort(np.random.default_rng(o.seed).integers(0, len(ref) - L, size=o.records))
        tid = np.searchsorted(ends, g, side="right")
        g = np.minimum(g, ends[tid] - L)
        order = np.lexsort((g, tid))
        if o.shuffled:
            order = order[np.random.default_rng(o.seed + 7).permutation(len(order))]
        g, tid = g[order], tid[order]
        pos = g - (ends[tid] - np.array([len(s) for s in seqs])[tid])
        jobs = [j + (tid[j[1]:j[1] + j[0]], (g[j[1]:j[1] + j[0]], pos[j[1]:j[1] + j[0]])) + ((True,) if o.pairs else ()) for j in jobs]
    with open(o.out, "wb") as f, ProcessPoolExecutor(o.procs) as ex:
        f.write(members(hdr))
        for part in ex.map(slice_job, jobs):
            f.write(part)
        f.write(EOF_BLOCK)
    print("%s: %d records, %d bytes" % (o.out, o.records, os.path.getsize(o.out)), file=sys.stderr)


if __name__ == "__main__":
    main()
