"""The rules of include/seqlib_amd_pile.h restated in plain Python, for tests/test_pile_host.py, tests/test_gpu_pile.py and tests/test_cpp_pile.py: record builders
(through tests/bam_util.py), the events of one record by a sequential walk, the 15 planes of a window by one increment per event, the candidate sites and their
TSV text, and a named list of cases.  Written from the rules, not from csrc/pile_host.h: there is no prefix sum and no lane here."""
import struct

import numpy as np

from tests import bam_util as bu

REFS = [("one", 1), ("c70", 70), ("c5k", 5000), ("big", 10000001)]
TEXT = "@HD\tVN:1.6\tSO:coordinate\n" + "".join("@SQ\tSN:%s\tLN:%d\n" % r for r in REFS)
OPS = "MIDNSHP=X"
PLANES = 15
A, C, G, T, N, DEL, INS, REV, LOWQ = 0, 1, 2, 3, 4, 5, 6, 7, 14
WHOLE = (2, 0, 5000)
WINDOWS = [WHOLE, (2, 100, 300), (2, 4900, 6000), (2, 0, 1)]
CLIPS = [(0, 1 << 40), (0, 5000), (100, 300), (4990, 5000), (0, 1)]


def parse_ops(ops):
    if not isinstance(ops, str):
        return list(ops)
    out, num = [], ""
    for ch in ops:
        if ch.isdigit():
            num += ch
        else:
            out.append((OPS.index(ch), int(num)))
            num = ""
    return out


def query_len(ops):
    return sum(ln for op, ln in parse_ops(ops) if op in (0, 1, 4, 7, 8))


def rec(tid, pos, ops, seq=None, qual=None, flag=0, mapq=60, name="r"):
    """ops: "10M3D5M", or [(op code 0..15, len)] for codes the text form cannot say; seq: None makes ACGT... of the CIGAR's query length; qual: None is absent"""
    ops = parse_ops(ops)
    if seq is None:
        seq = "".join("ACGT"[(i * 7 + i // 5) % 4] for i in range(query_len(ops)))
    raw = bytearray(bu.bam_record(name, flag, tid, pos, mapq, [("M", 1)] * len(ops), seq, qual))
    at = 36 + len(name) + 1
    for i, (op, ln) in enumerate(ops):
        struct.pack_into("<I", raw, at + 4 * i, ln << 4 | op)
    return bytes(raw)


def parse(r):
    """-> tid, pos, mapq, flag, [(op, len)], [4-bit codes], quality bytes"""
    tid, pos, l_name, mapq, _bin, n_cig, flag, l_seq = struct.unpack_from("<iiBBHHHi", r, 4)
    at = 36 + l_name
    words = struct.unpack_from("<%dI" % n_cig, r, at)
    at += 4 * n_cig
    packed = r[at:at + (l_seq + 1) // 2]
    codes = [(packed[i >> 1] >> (4 if i % 2 == 0 else 0)) & 15 for i in range(l_seq)]
    at += (l_seq + 1) // 2
    return tid, pos, mapq, flag, [(w & 15, w >> 4) for w in words], codes, r[at:at + l_seq]


def stream_of(recs):
    off = [0]
    for r in recs:
        off.append(off[-1] + len(r))
    return b"".join(recs), off


def eligible(r, tid, exclude_flags=0x704, min_mapq=0):
    t, pos, mapq, flag, ops, codes, _ = parse(r)
    return t == tid and pos >= 0 and not (flag & exclude_flags) and mapq >= min_mapq and len(ops) > 0 and len(codes) > 0


def events(r, min_baseq=0):
    """the (plane, position) events of a record before clipping, in the walk's order; flags, mapq and tid are not looked at"""
    _tid, pos, _mapq, flag, ops, codes, qual = parse(r)
    if pos < 0 or not ops or not codes:
        return []
    has_q = qual[0] != 0xff
    s = REV if flag & 0x10 else 0
    out, x, y = [], pos, 0
    for op, ln in ops:
        if op in (0, 7, 8):
            for _ in range(ln):
                if y >= len(codes):
                    return out
                base = {1: A, 2: C, 4: G, 8: T}.get(codes[y], N)
                out.append((s + base, x) if (not has_q or qual[y] >= min_baseq) else (LOWQ, x))
                x += 1
                y += 1
        elif op == 2:
            out += [(s + DEL, x + i) for i in range(ln)]
            x += ln
        elif op == 1:
            out.append((s + INS, x - 1))
            y += ln
        elif op == 4:
            y += ln
        elif op == 3:
            x += ln
    return out


def clipped(ev, beg, end):
    return [(p, x) for p, x in ev if beg <= x < end]


def window_of(window, refs=REFS):
    tid, beg, end = window
    beg = min(max(beg, 0), refs[tid][1])
    return tid, beg, min(max(end, beg), refs[tid][1])


def planes(recs, window=WHOLE, refs=REFS, min_mapq=0, min_baseq=0, exclude_flags=0x704):
    """-> numpy int32 [15, L] of the window clipped to its contig: one increment per event"""
    tid, beg, end = window_of(window, refs)
    out = np.zeros((PLANES, end - beg), dtype=np.int32)
    for r in recs:
        if eligible(r, tid, exclude_flags, min_mapq):
            for p, x in clipped(events(r, min_baseq), beg, end):
                out[p, x - beg] += 1
    return out


def sites(pl, beg, contig, min_depth, min_alt, frac_num, frac_den):
    """pl: planes of a window that starts at beg; contig: the reference contig's bytes -> [(pos, ref byte in upper case, depth, alt, ins, [15 counts])]"""
    out = []
    for i in range(pl.shape[1]):
        c = [int(v) for v in pl[:, i]]
        depth = sum(c[k] + c[REV + k] for k in (A, C, G, T, N, DEL))
        ref = contig[beg + i]
        if 97 <= ref <= 122:
            ref -= 32
        r = {65: A, 67: C, 71: G, 84: T}.get(ref)
        alt = 0 if r is None else depth - c[r] - c[REV + r]
        ins = c[INS] + c[REV + INS]
        ok = lambda v: v >= min_alt and v * frac_den >= frac_num * depth
        if depth >= min_depth and (ok(alt) or ok(ins)):
            out.append((beg + i, ref, depth, alt, ins, c))
    return out


def tsv(site_list, name):
    lines = []
    for pos, ref, depth, _alt, _ins, c in site_list:
        lines.append("%s\t%d\t%s\t%d\t%s\t%d\n" % (name, pos + 1, chr(ref), depth, "\t".join("%d,%d" % (c[k], c[REV + k]) for k in range(REV)), c[LOWQ]))
    return "".join(lines).encode()


def many_ops(n):
    """a CIGAR of n ops that uses every kind of block: M I M D M N = X ... with a leading and a trailing soft clip"""
    cyc = [(0, 3), (1, 2), (0, 4), (2, 1), (7, 2), (3, 5), (8, 1)]
    return [(4, 6)] + [cyc[i % len(cyc)] for i in range(n - 2)] + [(4, 9)]


RAMP = bytes((i * 3) % 41 for i in range(64))          # qualities 0 .. 40, present
# name, record: every shape include/seqlib_amd_pile.h has a rule for
CASES = [
    ("plain", rec(2, 100, "50M")),
    ("plain_rev", rec(2, 110, "50M", flag=0x10)),
    ("with_quals", rec(2, 120, "50M", qual=RAMP[:50])),
    ("with_quals_rev", rec(2, 125, "40M2I8M", qual=RAMP[:50], flag=0x10)),
    ("quals_ff_then_zeros", rec(2, 130, "20M", qual=b"\xff" + bytes(19))),
    ("quals_ff_inside", rec(2, 135, "20M", qual=bytes(5) + b"\xff" + bytes(14))),
    ("all_codes", rec(2, 200, "16M", seq=bu.SEQ_CODES)),
    ("all_codes_rev_quals", rec(2, 210, "16M", seq=bu.SEQ_CODES, qual=RAMP[20:36], flag=0x10)),
    ("odd_length", rec(2, 230, "7M", seq="ACGTNAC")),
    ("one_base", rec(2, 250, "1M", seq="G")),
    ("leading_I", rec(2, 100, "3I10M")),
    ("leading_I_at_0", rec(2, 0, "3I10M")),
    ("trailing_I", rec(2, 290, "10M3I")),
    ("trailing_I_at_window_end", rec(2, 291, "9M3I")),
    ("leading_S", rec(2, 300, "4S10M")),
    ("trailing_S", rec(2, 310, "10M4S")),
    ("H_S_M_S_H", rec(2, 320, "2H3S10M3S2H")),
    ("S_then_I", rec(2, 330, "3S2I10M")),
    ("D_over_window_begin", rec(2, 90, "5M20D5M")),
    ("D_over_window_end", rec(2, 290, "5M20D5M")),
    ("N_over_window_begin", rec(2, 85, "5M30N5M")),
    ("N_over_window_end", rec(2, 285, "5M30N5M")),
    ("D_over_contig_end", rec(2, 4990, "5M20D5M")),
    ("N_over_contig_end", rec(2, 4985, "5M30N5M")),
    ("M_over_contig_end", rec(2, 4995, "10M")),
    ("ends_on_last_base", rec(2, 4990, "10M")),
    ("I_anchored_on_last_base", rec(2, 4995, "5M2I3M")),
    ("starts_at_0", rec(2, 0, "20M")),
    ("M_over_window_begin_and_end", rec(2, 95, "300M")),
    ("short_seq_in_M", rec(2, 400, "20M", seq="ACGTACGTACGT")),
    ("short_seq_second_M", rec(2, 420, "5M3D10M2I5M", seq="ACGTACGT")),
    ("short_seq_S_passes_it", rec(2, 440, "10S5M", seq="ACGTACGT")),
    ("short_seq_I_D_then_M", rec(2, 450, "5M10I2D5M", seq="ACGTACGT")),
    ("short_seq_ends_with_op", rec(2, 470, "8M4D", seq="ACGTACGT")),
    ("0M", rec(2, 480, [(0, 0)], seq="A")),
    ("0M_past_short_seq", rec(2, 485, [(0, 2), (0, 0), (2, 3)], seq="AC")),
    ("n_cigar_0", rec(2, 500, "", seq="ACGT")),
    ("l_seq_0", rec(2, 510, "10M", seq="")),
    ("tid_elsewhere", rec(1, 10, "20M")),
    ("tid_-1", rec(-1, 100, "20M")),
    ("pos_-1", rec(2, -1, "20M")),
    ("unmapped_placed", rec(2, 520, "20M", flag=4)),
    ("dup", rec(2, 530, "20M", flag=0x400)),
    ("secondary", rec(2, 540, "20M", flag=0x100)),
    ("qcfail", rec(2, 550, "20M", flag=0x200)),
    ("supplementary", rec(2, 560, "20M", flag=0x800)),
    ("low_mapq", rec(2, 570, "20M", mapq=3)),
    ("10M3D10M2I5M", rec(2, 700, "10M3D10M2I5M", qual=RAMP[:27])),
    ("10M100N10M_rev", rec(2, 750, "10M100N10M", flag=0x10)),
    ("=_and_X", rec(2, 900, "10=2X8=", qual=RAMP[10:30])),
    ("ops_64", rec(2, 1000, many_ops(64))),
    ("ops_65", rec(2, 1500, many_ops(65), qual=(RAMP * 4)[:query_len(many_ops(65))])),
    ("ops_200", rec(2, 2000, many_ops(200), flag=0x10)),
    ("ops_200_over_end", rec(2, 4800, many_ops(200))),
    ("ops_200_short_seq", rec(2, 2600, many_ops(200), seq="ACGT" * 40)),
    ("read_5000", rec(2, 0, "5000M", qual=(RAMP * 79)[:5000])),
    ("read_5000_over_end", rec(2, 3000, "2500M50D2450M", flag=0x10)),
    ("big_contig", rec(3, 100, "50M")),
] + [("op_code_%d" % k, rec(2, 3000 + 10 * k, [(k, 7)], seq="ACGTACG")) for k in range(16)]


def random_records(n, seed=1, span=5000, tid=2):
    """n records on contig tid, coordinate-sorted: mostly short reads of a few ops with and without qualities, on both strands, some filtered or with long CIGARs"""
    import random
    rng = random.Random(seed)
    shapes = ["%dM", "5S%dM", "%dM4S", "20M2I%dM", "20M3D%dM", "10M50N%dM", "3H%dM", "%d=2X", "2I%dM"]
    out = []
    for _ in range(n):
        pos = rng.randrange(span)
        k = rng.randrange(40)
        if k == 0:
            out.append(rec(-1, -1, "", seq="", flag=4))
        elif k == 1:
            out.append(rec(tid, pos, "30M", flag=rng.choice((0x100, 0x200, 0x400, 4))))
        elif k == 2:
            out.append(rec(tid, pos, many_ops(rng.choice((65, 90, 130)))))
        elif k == 3:
            out.append(rec(rng.choice((0, 1)), 0, "1M", seq="A"))
        else:
            ops = rng.choice(shapes) % rng.randrange(1, 150)
            ql = query_len(ops)
            seq = "".join(rng.choice("ACGTACGTACGTN") for _ in range(ql))
            qual = bytes(rng.randrange(42) for _ in range(ql)) if rng.random() < 0.6 else None
            out.append(rec(tid, pos, ops, seq=seq, qual=qual, mapq=rng.randrange(61), flag=rng.choice((0, 0x10, 0x63, 0x93))))
    return sorted(out, key=lambda r: (parse(r)[0] & 0xffffffff, parse(r)[1]))


# ---------------------------------------------------------------- reads against a reference text, for the candidate sites
def fasta_contigs(path):
    out = []
    for ln in open(path):
        if ln.startswith(">"):
            out.append([ln[1:].split()[0], []])
        else:
            out[-1][1].append(ln.strip())
    return [(n, "".join(s).encode()) for n, s in out]


def cut_reads(contig, tid, first, last, step, length, edits):
    """reads of `length` bases cut from the contig every `step` positions; edits: {pos: (kind, every, arg)} plants, in every `every`-th read that covers pos, a
    substitution ('X': the base after the reference's in ACGT), an insertion ('I', arg bases after pos) or a deletion ('D', arg bases from pos)"""
    recs = []
    for k, s in enumerate(range(first, last, step)):
        ops, seq, x = [], [], s
        run = 0
        while x < s + length:
            e = edits.get(x)
            base = chr(contig[x]).upper()
            base = base if base in "ACGT" else "A"
            if e and k % e[1] == 0 and s < x < s + length - 8:
                kind, _, arg = e
                if kind == "X":
                    seq.append("ACGT"[("ACGT".index(base) + 1) % 4]); run += 1; x += 1
                elif kind == "I":
                    seq.append(base); run += 1; x += 1
                    ops.append((0, run)); run = 0
                    ops.append((1, arg)); seq += ["G"] * arg
                else:
                    ops.append((0, run)); run = 0
                    ops.append((2, arg)); x += arg
                continue
            seq.append(base); run += 1; x += 1
        if run:
            ops.append((0, run))
        recs.append(rec(tid, s, ops, seq="".join(seq), flag=0x10 if k % 3 == 0 else 0, qual=bytes([30 + k % 10]) * len(seq) if k % 2 else None))
    return recs
