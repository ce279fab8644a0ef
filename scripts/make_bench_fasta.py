#!/usr/bin/env python3
"""Writes the input of tools/refgenome_bench.cpp: a synthetic multi-contig FASTA with 60-base lines, the layout of the human reference's files.  Contig i is named
chrI and followed by a description; lengths fall off from the first to the last as a genome's do; the bases are A, C, G, T with runs of N and stretches of
lower case, from a seed.  --bgzf writes the same text as BGZF members of 0xff00 bytes (what bgzip writes), --gzip as one gzip stream.

    python scripts/make_bench_fasta.py out.fa [--bases 500000000] [--contigs 24] [--seed 1] [--bgzf | --gzip]
"""
import argparse
import gzip
import struct
import zlib

import numpy as np

W = 60


def contig_text(name, n, rng):
    b = np.frombuffer(b"ACGT", dtype=np.uint8)[rng.integers(0, 4, n)]
    for _ in range(max(1, n // 2000000)):                 # a run of N and a stretch of lower case per 2 Mb
        a = int(rng.integers(0, max(1, n - 5000)))
        b[a:a + int(rng.integers(100, 5000))] = ord("N")
        a = int(rng.integers(0, max(1, n - 20000)))
        b[a:a + int(rng.integers(1000, 20000))] |= 0x20
    full = n // W
    body = np.empty((full, W + 1), dtype=np.uint8)
    body[:, :W] = b[:full * W].reshape(full, W)
    body[:, W] = 10
    tail = b[full * W:].tobytes()
    return b">" + name + b" synthetic contig, seed-generated\n" + body.tobytes() + (tail + b"\n" if tail else b"")


def member(payload):
    c = zlib.compressobj(6, zlib.DEFLATED, -15)
    comp = c.compress(payload) + c.flush()
    return (bytes([0x1f, 0x8b, 8, 4, 0, 0, 0, 0, 0, 0xff, 6, 0, 0x42, 0x43, 2, 0]) + struct.pack("<H", 18 + len(comp) + 8 - 1) + comp +
            struct.pack("<II", zlib.crc32(payload) & 0xffffffff, len(payload)))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("out")
    ap.add_argument("--bases", type=int, default=500000000)
    ap.add_argument("--contigs", type=int, default=24)
    ap.add_argument("--seed", type=int, default=1)
    ap.add_argument("--bgzf", action="store_true")
    ap.add_argument("--gzip", action="store_true")
    a = ap.parse_args()
    rng = np.random.default_rng(a.seed)
    w = np.array([1.0 / (1 + 0.15 * i) for i in range(a.contigs)])
    lens = np.maximum(1, (w / w.sum() * a.bases).astype(np.int64))
    eof = bytes([0x1f, 0x8b, 8, 4, 0, 0, 0, 0, 0, 0xff, 6, 0, 0x42, 0x43, 2, 0, 0x1b, 0, 3, 0, 0, 0, 0, 0, 0, 0, 0, 0])
    with (gzip.open(a.out, "wb", compresslevel=6) if a.gzip else open(a.out, "wb")) as f:
        carry = b""
        for i, n in enumerate(lens):
            t = contig_text(b"chr%d" % (i + 1), int(n), rng)
            if not a.bgzf:
                f.write(t)
                continue
            t = carry + t
            cut = len(t) - len(t) % 0xff00
            f.write(b"".join(member(t[k:k + 0xff00]) for k in range(0, cut, 0xff00)))
            carry = t[cut:]
        if a.bgzf:
            f.write((member(carry) if carry else b"") + eof)
    print("%s: %d contigs, %d bases" % (a.out, a.contigs, int(lens.sum())))


if __name__ == "__main__":
    main()
