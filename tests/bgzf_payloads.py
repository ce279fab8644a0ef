"""The payloads that pin the DEFLATE encoder's corner cases, shared by tests/test_bgzf_writer.py (the host-compiled member body) and tests/test_gpu_bgzf.py
(the GPU writer).  Everything comes from seeds, tests/bam_util.py and the FASTQ fixture; nothing here touches the library."""
import functools
import os
import random

from tests import bam_util as bu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
M = bu.MEMBER_MAX
SIZES = [0, 1, 2, 3, 257, 258, 259, M - 1, M, M + 1, 2 * M + 5]


def rand_bytes(n, seed):
    return random.Random(seed).randbytes(n)


def corpus_bam():
    """the `bam` payload of tests/test_bam_reader.payloads()"""
    bam = bu.bam_header(bu.TEXT, bu.REFS) + b"".join(bu.sample_records(120))
    return bam[:M]


@functools.lru_cache(maxsize=None)
def p1():
    """{(kind, size): payload}: zeros, seeded random bytes, the corpus's bam payload repeated"""
    bam = corpus_bam()
    out = {}
    for n in SIZES:
        out["zeros", n] = bytes(n)
        out["random", n] = rand_bytes(n, 1000 + n)
        out["bam", n] = (bam * (n // len(bam) + 1))[:n]
    return out


@functools.lru_cache(maxsize=None)
def p2():
    """X + R + X in one member: the repeat at distance exactly 32768, and at 32769 where it must not be used"""
    x = rand_bytes(300, 21)
    return {"dist32768": x + rand_bytes(32468, 22) + x, "dist32769": x + rand_bytes(32469, 23) + x}


@functools.lru_cache(maxsize=None)
def p3():
    run = bytes([0x5a]) * (258 * 3 + 2)
    return {"abc": b"abc" * 20000, "run": rand_bytes(5000, 31) + run + rand_bytes(5000, 32), "zeros200k": bytes(200000)}


@functools.lru_cache(maxsize=None)
def p4():
    """byte value i occurs Fib(i) times, i = 1..22: 46 367 bytes, an unlimited Huffman tree over them is 21 deep"""
    a, b, data = 1, 1, bytearray()
    for i in range(1, 23):
        data += bytes([i]) * a
        a, b = b, a + b
    assert len(data) == 46367
    lst = list(data)
    random.Random(41).shuffle(lst)
    return bytes(lst)


@functools.lru_cache(maxsize=None)
def p5_sample():
    """header + 6000 sample records: 2.3 MB, 36 members"""
    return bu.bam_header(bu.TEXT, bu.REFS) + b"".join(bu.sample_records(6000))


@functools.lru_cache(maxsize=None)
def p5_fastq():
    """header + the FASTQ fixture's 3000 reads as mapped records, 150M, the file's qualities: 904 598 bytes"""
    lines = open(os.path.join(ROOT, "tests", "golden", "sim1_bcr.head3000.fq")).read().split("\n")
    recs = []
    for i in range(0, len(lines) - 3, 4):
        name, seq, qual = lines[i][1:], lines[i + 1], lines[i + 3]
        recs.append(bu.bam_record(name, 0, 0, 100 + 37 * (i // 4), 60, [("M", len(seq))], seq, bytes(ord(c) - 33 for c in qual)))
    p = bu.bam_header(bu.TEXT, bu.REFS) + b"".join(recs)
    assert len(p) == 904598
    return p


def everything():
    """[(name, payload)] of P1..P5"""
    out = [("p1/%s/%d" % k, v) for k, v in p1().items()]
    out += [("p2/" + k, v) for k, v in p2().items()] + [("p3/" + k, v) for k, v in p3().items()]
    out += [("p4/fib", p4()), ("p5/sample", p5_sample()), ("p5/fastq", p5_fastq())]
    return out


def blocks(payload):
    return [payload[i:i + M] for i in range(0, len(payload), M)]


def isize_list(payload):
    return [len(b) for b in blocks(payload)]


def check_round_trip(raw, payload):
    """inflate_all(file) == payload (ISIZE and CRC32 asserted per member), the EOF block, the ISIZE list [0xff00] * k + [rest]"""
    members, has_eof = bu.scan_members(raw)
    assert has_eof
    assert [m[3] for m in members[:-1]] == isize_list(payload)
    assert all(m[0] + m[1] + m[2] + 8 <= 0x10000 + m[0] for m in members)
    assert bu.inflate_all(raw) == payload
    return members[:-1]


def zlib_total(payload, **opts):
    """deflate bytes of the payload's 0xff00 blocks under a zlib setting"""
    return sum(len(bu.deflate_raw(b, **opts)) for b in blocks(payload))
