#!/usr/bin/env python3
"""Writes the input of tools/bamread_bench.cpp: a BAM of synthetic 150 bp records with qualities, BGZF members of 0xff00 bytes deflated at level 6
(zlib, one process per slice of members).  The reads are windows of a reference FASTA (default tests/golden/tiny.fa) with 1 % substitutions, half of
them reverse-complemented, stored as unmapped records -- so the same file feeds BWAAligner::alignSequences(BamReader&) with that reference's index.

    python scripts/make_bench_bam.py out.bam [--records 2000000] [--ref tests/golden/tiny.fa] [--procs 8] [--seed 1]
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


def slice_job(args):
    n, first, ref, seed = args
    return members(records(n, first, ref, np.random.default_rng(seed)).tobytes())


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("out")
    ap.add_argument("--records", type=int, default=2000000)
    ap.add_argument("--ref", default=os.path.join(ROOT, "tests", "golden", "tiny.fa"))
    ap.add_argument("--procs", type=int, default=8)
    ap.add_argument("--seed", type=int, default=1)
    o = ap.parse_args()
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
    text = "@HD\tVN:1.6\tSO:unsorted\n" + "".join("@SQ\tSN:%s\tLN:%d\n" % (n, len(s)) for n, s in zip(names, seqs))
    hdr = b"BAM\1" + struct.pack("<I", len(text)) + text.encode() + struct.pack("<I", len(names))
    for n, s in zip(names, seqs):
        hdr += struct.pack("<I", len(n) + 1) + n.encode() + b"\0" + struct.pack("<I", len(s))
    per = 200000                                         # records per job
    jobs = [(min(per, o.records - f), f, ref, o.seed * 100003 + f) for f in range(0, o.records, per)]
    with open(o.out, "wb") as f, ProcessPoolExecutor(o.procs) as ex:
        f.write(members(hdr))
        for part in ex.map(slice_job, jobs):
            f.write(part)
        f.write(EOF_BLOCK)
    print("%s: %d records, %d bytes" % (o.out, o.records, os.path.getsize(o.out)), file=sys.stderr)


if __name__ == "__main__":
    main()
