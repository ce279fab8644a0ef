#!/usr/bin/env python3
"""Writes the input of tools/fastq_bench.cpp: synthetic 150 bp reads (seqlib_amd/synth.py: wgsim-like reads of a reference FASTA, default
tests/golden/tiny.fa, so the same file aligns against that reference's index) as strict 4-line FASTQ, 322 bytes a record:

    @r00000017 1:N:0        name, comment
    <150 bases>
    +
    <150 qualities>         high, drifting down along the read

in three forms of the same text: <out> plain, <out>.bgz as BGZF (members of 0xff00 bytes, level 6) and <out>.gz as one gzip stream (level 6).

    python scripts/make_bench_fastq.py out.fq [--reads 2000000] [--ref tests/golden/tiny.fa] [--procs 8] [--seed 1]
"""
import argparse
import os
import struct
import sys
import zlib
from concurrent.futures import ProcessPoolExecutor

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from seqlib_amd import synth  # noqa: E402

EOF_BLOCK = bytes([0x1f, 0x8b, 8, 4, 0, 0, 0, 0, 0, 0xff, 6, 0, 0x42, 0x43, 2, 0, 0x1b, 0, 3, 0, 0, 0, 0, 0, 0, 0, 0, 0])
L = 150


def member(payload):
    c = zlib.compressobj(6, zlib.DEFLATED, -15)
    comp = c.compress(payload) + c.flush()
    return (bytes([0x1f, 0x8b, 8, 4, 0, 0, 0, 0, 0, 0xff, 6, 0, 0x42, 0x43, 2, 0]) + struct.pack("<H", 18 + len(comp) + 8 - 1) + comp +
            struct.pack("<II", zlib.crc32(payload) & 0xffffffff, len(payload)))


def members(data):
    return b"".join(member(data[i:i + 0xff00]) for i in range(0, len(data), 0xff00))


def records(reads, first, seed):
    """reads: uint8 ASCII [n, L] -> the text of the n records"""
    n = len(reads)
    head = b"@r00000000 1:N:0\n"
    a = np.zeros((n, len(head) + L + 3 + L + 1), dtype=np.uint8)
    a[:, :len(head)] = np.frombuffer(head, dtype=np.uint8)
    ids = np.arange(first, first + n)
    for d in range(8):
        a[:, 2 + d] = 48 + (ids // 10 ** (7 - d)) % 10
    o = len(head)
    a[:, o:o + L] = reads
    a[:, o + L:o + L + 3] = np.frombuffer(b"\n+\n", dtype=np.uint8)
    rng = np.random.default_rng(seed)
    a[:, o + L + 3:o + 2 * L + 3] = 33 + np.clip(rng.normal(34, 5, size=(n, L)) - np.arange(L)[None, :] * 0.04, 2, 40).astype(np.uint8)
    a[:, -1] = 10
    return a.tobytes()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("out")
    ap.add_argument("--reads", type=int, default=2000000)
    ap.add_argument("--ref", default=os.path.join(ROOT, "tests", "golden", "tiny.fa"))
    ap.add_argument("--procs", type=int, default=8)
    ap.add_argument("--seed", type=int, default=1)
    o = ap.parse_args()
    seq = "".join(ln.strip().upper() for ln in open(o.ref) if not ln.startswith(">"))
    lut = np.zeros(256, dtype=np.uint8)
    for i, c in enumerate("ACGT"):
        lut[ord(c)] = i
    genome = lut[np.frombuffer(seq.encode(), dtype=np.uint8)]
    per = 200000
    gz = zlib.compressobj(6, zlib.DEFLATED, 31)
    size = 0
    with open(o.out, "wb") as f, open(o.out + ".bgz", "wb") as fb, open(o.out + ".gz", "wb") as fg, ProcessPoolExecutor(o.procs) as ex:
        carry = b""
        for first in range(0, o.reads, per):
            n = min(per, o.reads - first)
            reads = synth.make_reads(genome, n, L, o.seed * 100003 + first)
            text = records(reads, first, o.seed * 7 + first)
            f.write(text)
            fg.write(gz.compress(text))
            data = carry + text
            cut = len(data) - len(data) % 0xff00
            step = 0xff00 * 64
            for part in ex.map(members, [data[i:min(i + step, cut)] for i in range(0, cut, step)]):
                fb.write(part)
            carry = data[cut:]
            size += len(text)
        fb.write(members(carry) + EOF_BLOCK)
        fg.write(gz.flush())
    print("%s: %d reads, %d bytes of text; .bgz %d bytes, .gz %d bytes" % (o.out, o.reads, size, os.path.getsize(o.out + ".bgz"), os.path.getsize(o.out + ".gz")), file=sys.stderr)


if __name__ == "__main__":
    main()
