"""The rules of include/seqlib_amd_cov.h restated in Python and numpy, for tests/test_cov_host.py, tests/test_gpu_cov.py and tests/test_cpp_cov.py: record
builders (through tests/bam_util.py), the depth of every position by brute force in the three modes, region sums, bedGraph text and a named list of cases.
Written from the rules, not from csrc/cov_host.h: depth here is a slice increment per covered interval, never a difference array."""
import struct

import numpy as np

from tests import bam_util as bu

SPAN, FULL, ALIGNED = 0, 1, 2
REFS = [("one", 1), ("c70", 70), ("c5k", 5000), ("big", 10000001)]
TEXT = "@HD\tVN:1.6\tSO:coordinate\n" + "".join("@SQ\tSN:%s\tLN:%d\n" % r for r in REFS)
OPS = "MIDNSHP=X"
REF_OPS = (0, 2, 3, 7, 8)          # M D N = X consume reference; 9..15 do not
# (mode, buff, count_del): every setting the tests run
CONFIGS = [(SPAN, 0, 0), (SPAN, 3, 0), (SPAN, -2, 0), (FULL, 0, 0), (ALIGNED, 0, 0), (ALIGNED, 0, 1)]
CONFIG_IDS = ["span", "span_buff3", "span_buff-2", "full", "aligned", "aligned_del"]


def rec(tid, pos, ops, flag=0, mapq=60, name="r"):
    """ops: "10M3D5M", or [(op code 0..15, len)] for codes the text form cannot say"""
    if isinstance(ops, str):
        out, num = [], ""
        for ch in ops:
            if ch.isdigit():
                num += ch
            else:
                out.append((OPS.index(ch), int(num)))
                num = ""
        ops = out
    raw = bytearray(bu.bam_record(name, flag, tid, pos, mapq, [("M", 1)] * len(ops), "", b""))
    at = 36 + len(name) + 1
    for i, (op, ln) in enumerate(ops):
        struct.pack_into("<I", raw, at + 4 * i, ln << 4 | op)
    return bytes(raw)


def parse(r):
    tid, pos, l_name, mapq, _bin, n_cig, flag = struct.unpack_from("<iiBBHHH", r, 4)
    words = struct.unpack_from("<%dI" % n_cig, r, 36 + l_name)
    return tid, pos, mapq, flag, [(w & 15, w >> 4) for w in words]


def stream_of(recs):
    off = [0]
    for r in recs:
        off.append(off[-1] + len(r))
    return b"".join(recs), off


def eligible(r, n_ref, exclude_flags=0x704, min_mapq=0):
    tid, pos, mapq, flag, _ = parse(r)
    return 0 <= tid < n_ref and pos >= 0 and not (flag & exclude_flags) and mapq >= min_mapq


def intervals(r, mode, buff=0, count_del=0):
    """the half-open intervals the record covers, before clipping; flags and mapq are not looked at"""
    tid, pos, _mapq, flag, ops = parse(r)
    if tid < 0 or pos < 0:
        return []
    reflen = sum(ln for op, ln in ops if op in REF_OPS)
    end = pos + (1 if reflen == 0 or flag & 4 else reflen)
    if mode == ALIGNED:
        out, x = [], pos
        for op, ln in ops:
            if op in (0, 7, 8) or (op == 2 and count_del):
                out.append((x, x + ln))
            if op in REF_OPS:
                x += ln
        return out
    if mode == FULL:
        p = max(0, pos - ops[0][1]) if ops and ops[0][0] == 4 else pos
        e = end + ops[-1][1] if ops and ops[-1][0] == 4 else end
    else:
        p, e = pos + buff, end - buff
    if p < 0 or e < 0 or p > e:
        return []
    return [(p, e + 1)]          # inclusive of e: the reference's quirk


def clipped(iv, beg, end):
    return [(max(lo, beg), min(hi, end)) for lo, hi in iv if max(lo, beg) < min(hi, end)]


def depth(recs, mode, buff=0, count_del=0, exclude_flags=0x704, min_mapq=0, refs=REFS, window=None):
    """-> [numpy int32 per contig]: the depth of every position; with a window (tid, beg, end) only that contig has positions, the others are empty"""
    out = [np.zeros(ln, dtype=np.int32) for _, ln in refs]
    for r in recs:
        if not eligible(r, len(refs), exclude_flags, min_mapq):
            continue
        tid = parse(r)[0]
        beg, end = (0, refs[tid][1]) if window is None else ((window[1], window[2]) if window[0] == tid else (0, 0))
        for lo, hi in clipped(intervals(r, mode, buff, count_del), max(beg, 0), min(end, refs[tid][1])):
            out[tid][lo:hi] += 1
    return out


def region_sums(d, regs, min_depth):
    s, c = [], []
    for tid, beg, end in regs:
        v = d[tid][max(beg, 0):max(min(end, len(d[tid])), 0)] if beg < end else d[tid][:0]
        s.append(int(v.sum(dtype=np.int64)))
        c.append(int((v >= min_depth).sum()))
    return s, c


def bedgraph(d, include_zero, tids=None, refs=REFS, first=0):
    """name \t start \t end \t depth per maximal run of equal depth over positions first .. first + len(d[t]) of the contigs tids (None: all, in order)"""
    out = []
    for t in range(len(refs)) if tids is None else tids:
        v = d[t]
        if not len(v):
            continue
        heads = np.concatenate(([0], np.flatnonzero(v[1:] != v[:-1]) + 1, [len(v)]))
        for a, b in zip(heads[:-1].tolist(), heads[1:].tolist()):
            if v[a] or include_zero:
                out.append("%s\t%d\t%d\t%d\n" % (refs[t][0], a + first, b + first, v[a]))
    return "".join(out).encode()


def many_ops(n):
    """a CIGAR of n ops that uses every kind of block: M I M D M N = X ... with a leading and a trailing soft clip"""
    cyc = [(0, 3), (1, 2), (0, 4), (2, 1), (7, 2), (3, 5), (8, 1)]
    return [(4, 6)] + [cyc[i % len(cyc)] for i in range(n - 2)] + [(4, 9)]


# name, record: every shape include/seqlib_amd_cov.h has a rule for
CASES = [
    ("plain", rec(2, 100, "50M")),
    ("tid_-1", rec(-1, 100, "50M")),
    ("tid_n_ref", rec(len(REFS), 100, "50M")),
    ("pos_-1", rec(2, -1, "50M")),
    ("unmapped_placed", rec(2, 200, "50M", flag=4)),
    ("n_cigar_0", rec(2, 300, "")),
    ("5S10M", rec(2, 400, "5S10M")),
    ("10M5S", rec(2, 420, "10M5S")),
    ("2H5S10M", rec(2, 440, "2H5S10M")),
    ("7S", rec(2, 460, "7S")),
    ("5S10M_at_2", rec(2, 2, "5S10M")),
    ("10M100N10M", rec(2, 500, "10M100N10M")),
    ("10M3D10M2I5M", rec(2, 700, "10M3D10M2I5M")),
    ("0M", rec(2, 760, [(0, 0)])),
    ("ends_at_end", rec(2, 4990, "10M")),
    ("ends_beyond", rec(2, 4995, "10M")),
    ("last_base", rec(2, 4999, "1M")),
    ("last_base_long", rec(2, 4999, "30M")),
    ("starts_at_0", rec(2, 0, "20M")),
    ("len_1_contig", rec(0, 0, "1M")),
    ("len_1_contig_long", rec(0, 0, "5S10M5S")),
    ("c70_whole", rec(1, 0, "70M")),
    ("c70_over", rec(1, 60, "20M")),
    ("low_mapq", rec(2, 800, "50M", mapq=3)),
    ("dup", rec(2, 810, "50M", flag=0x400)),
    ("secondary", rec(2, 820, "50M", flag=0x100)),
    ("qcfail", rec(2, 830, "50M", flag=0x200)),
    ("supplementary", rec(2, 840, "50M", flag=0x800)),
    ("big_near_end", rec(3, 10000001 - 40, "8S30M2D20M")),
    ("big_8_digits", rec(3, 9999000, "100M")),
    ("ops_64", rec(2, 1000, many_ops(64))),
    ("ops_65", rec(2, 1500, many_ops(65))),
    ("ops_200", rec(2, 2000, many_ops(200))),
    ("ops_200_over_end", rec(2, 4800, many_ops(200))),
] + [("op_code_%d" % k, rec(2, 900 + 4 * k, [(k, 7)])) for k in range(16)]


def random_records(n, seed=1, refs=REFS, span=None):
    """n records on the contigs below the big one, coordinate-sorted: mostly short reads of a few ops, some unmapped, filtered or with long CIGARs; span: keep every
    start below it (None: anywhere on the contig)"""
    import random
    rng = random.Random(seed)
    shapes = ["%dM", "5S%dM", "%dM4S", "20M2I%dM", "20M3D%dM", "10M50N%dM", "3H%dM", "%d=2X"]
    out = []
    for i in range(n):
        tid = rng.choice((1, 2, 2, 2, 2, 0))
        pos = rng.randrange(min(refs[tid][1], span or refs[tid][1]))
        k = rng.randrange(40)
        if k == 0:
            out.append(rec(-1, -1, "", flag=4))
        elif k == 1:
            out.append(rec(tid, pos, "30M", flag=rng.choice((0x100, 0x200, 0x400, 4))))
        elif k == 2:
            out.append(rec(tid, pos, many_ops(rng.choice((65, 90, 130)))))
        else:
            out.append(rec(tid, pos, rng.choice(shapes) % rng.randrange(1, 150), mapq=rng.randrange(61)))
    return sorted(out, key=lambda r: (parse(r)[0] & 0xffffffff, parse(r)[1]))
