"""The rules of include/seqlib_amd_ref.h, stated in Python: the .fai text of a FASTA, the clipping of a region, the NM / MD walk of a BAM record; the FASTA and
record cases the host and the GPU tests share.

Where the documented .fai format and the calmd rules are silent, the library decides, and the decisions are these (the header states the same):
  - a CR in front of the LF belongs to the terminator, and so does a CR at the very end of a last line without a LF;
  - NAME ends at the first space or tab; a header line is recognised by its first byte alone;
  - OFFSET of a contig without bases is the byte behind its header line; its LINEBASES and LINEWIDTH are 0;
  - the contig's last sequence line may be shorter than LINEBASES, never longer, and its terminator is not compared;
  - a blank line may be followed only by blank lines, a header or the end: a sequence line behind one fails;
  - any byte outside 33..126 inside a sequence line fails like a space or a tab;
  - a text without any contig (an empty one) fails; the first error in file order is the one reported;
  - an M, = or X stops the walk where it would read a base at or behind l_seq (a CIGAR longer than its read);
  - a D emits the run and '^' even when the contig's end leaves it no base; '=' and U in the reference are code 15.
"""
import random
import struct

from tests import bam_util as bu

MAX_CONTIG = 2 ** 31 - 1
WHAT = {
    "byte": "a space, a tab or another byte outside 33..126 inside a sequence line",
    "ragged": "a ragged line in the middle of a contig",
    "after_blank": "a sequence line behind a blank line",
    "name_empty": "an empty contig name",
    "name_twice": "a contig name seen twice",
    "before": "bytes before the first '>'",
    "fastq": "a '@' record: this is FASTQ, not FASTA",
    "none": "no contig",
}


class FastaError(Exception):
    def __init__(self, what, contig, byte):
        super().__init__("%s (contig '%s', byte %d)" % (WHAT[what], contig.decode("latin-1"), byte))
        self.what = what


def lines_of(text):
    """[(start, content, width)]"""
    out, a = [], 0
    while a < len(text):
        b = text.find(b"\n", a)
        e = len(text) if b < 0 else b + 1
        content = text[a:e]
        if content.endswith(b"\n"):
            content = content[:-1]
        if content.endswith(b"\r"):
            content = content[:-1]
        out.append((a, content, e - a))
        a = e
    return out


def contigs_of(text):
    """[(name, length, offset, linebases, linewidth, bases)]; raises FastaError"""
    if not text:
        raise FastaError("none", b"", 0)
    if text[0:1] != b">":
        raise FastaError("fastq" if text[0:1] == b"@" else "before", b"", 0)
    L = lines_of(text)
    out, seen, prev_blank = [], set(), False
    for i, (a, c, w) in enumerate(L):
        if not c:
            prev_blank = True
            continue
        if c[0:1] == b">":
            name = c[1:].split(b" ")[0].split(b"\t")[0]
            if not name:
                raise FastaError("name_empty", name, a)
            if name in seen:
                raise FastaError("name_twice", name, a)
            seen.add(name)
            out.append([name, 0, a + w, 0, 0, bytearray()])
        else:
            cur = out[-1]
            if prev_blank:
                raise FastaError("after_blank", cur[0], a)
            if any(x < 33 or x > 126 for x in c):
                raise FastaError("byte", cur[0], a)
            if cur[1] == 0 and cur[3] == 0:
                cur[3], cur[4] = len(c), w
            nxt = L[i + 1][1] if i + 1 < len(L) else b""
            is_last = not nxt or nxt[0:1] == b">"
            if (len(c) > cur[3]) if is_last else (len(c) != cur[3] or w != cur[4]):
                raise FastaError("ragged", cur[0], a)
            cur[1] += len(c)
            cur[5] += c
        prev_blank = False
    return [tuple(c[:5]) + (bytes(c[5]),) for c in out]


def fai_text(text):
    return b"".join(b"%s\t%d\t%d\t%d\t%d\n" % c[:5] for c in contigs_of(text))


def fetch(contigs, regions, upper=0):
    """the clipping: (bytes, offsets) of [(tid, beg, end)]"""
    out, offs = bytearray(), [0]
    for tid, beg, end in regions:
        seq = contigs[tid][5]
        b, e = max(beg, 0), min(end, len(seq))
        if e > b:
            out += seq[b:e].upper() if upper else seq[b:e]
        offs.append(len(out))
    return bytes(out), offs


# ---------------------------------------------------------------- FASTA generator and cases
def fasta(contigs, width=60, eol=b"\n", last_eol=True):
    """contigs: [(header text behind '>', bases)]"""
    t = bytearray()
    for hdr, seq in contigs:
        t += b">" + hdr + eol
        for i in range(0, len(seq), width):
            t += seq[i:i + width] + eol
    if not last_eol and t.endswith(eol):
        del t[len(t) - len(eol):]
    return bytes(t)


def rand_bases(rng, n, alphabet=b"ACGT"):
    return bytes(rng.choice(alphabet) for _ in range(n))


def _cases():
    rng = random.Random(11)
    a, b, c = rand_bases(rng, 150), rand_bases(rng, 47), rand_bases(rng, 120)
    three = [(b"one", a), (b"two", b), (b"three", c)]
    good = {
        "lf": fasta(three, 60),
        "crlf": fasta(three, 60, b"\r\n"),
        "no_final_eol": fasta(three, 60, last_eol=False),
        "crlf_no_final_eol": fasta(three, 60, b"\r\n", last_eol=False),
        "one_line_contig": fasta([(b"solo", b)], 60),
        "last_line_full": fasta([(b"x", c), (b"y", a[:60])], 60),
        "zero_between": fasta([(b"one", a), (b"empty", b""), (b"three", c)], 60),
        "zero_last": fasta([(b"one", a), (b"empty", b"")], 60),
        "zero_last_no_eol": fasta([(b"one", a), (b"empty", b"")], 60, last_eol=False),
        "zero_only": b">nothing\n",
        "trailing_blank": fasta(three, 60) + b"\n\n\n",
        "blank_before_header": fasta([(b"one", a)], 60) + b"\n" + fasta([(b"two", b)], 60) + b"\r\n",
        "lower_and_iupac": fasta([(b"mix", b"acgtnACGTNRYKMSWBDHVryk" * 5)], 50),
        "description": fasta([(b"chr1 the first one", a), (b"chr2\twith a tab", b)], 70),
        "width_1": fasta([(b"w1", b[:9])], 1),
        "other_printables": fasta([(b"odd", b"AC*-.@GT>x" * 7)], 30),
        "cr_at_end_unterminated": b">x\nACGT\nAC\r",
        "last_line_other_terminator": b">x\r\nACGT\r\nAC\n>y\nGG\n",
    }
    bad = {
        "empty_name": (b">one\nACGT\n>\nAC\n", "name_empty", b"", 10),
        "empty_name_with_description": (b"> desc\nACGT\n", "name_empty", b"", 0),
        "name_twice": (b">one\nACGT\n>two\nAC\n>one x\nAC\n", "name_twice", b"one", 18),
        "bytes_before": (b"ACGT\n>one\nACGT\n", "before", b"", 0),
        "blank_before": (b"\n>one\nACGT\n", "before", b"", 0),
        "fastq": (b"@r1\nACGT\n+\nIIII\n", "fastq", b"", 0),
        "space_inside": (b">one\nACGT\nAC T\nAC\n", "byte", b"one", 10),
        "tab_inside": (b">one\nAC\tT\nACGT\n", "byte", b"one", 5),
        "control_inside": (b">one\nAC\x01T\n", "byte", b"one", 5),
        "ragged_short": (b">one\nACGT\nAC\nACGT\n", "ragged", b"one", 10),
        "ragged_long_last": (b">one\nACGT\nACGTA\n", "ragged", b"one", 10),
        "ragged_width": (b">one\nACGT\r\nACGT\nACGT\n", "ragged", b"one", 11),
        "ragged_second_contig": (b">one\nACGT\nAC\n>two\nAC\nACG\nA\n", "ragged", b"two", 21),
        "blank_inside": (b">one\nACGT\n\nACGT\n", "after_blank", b"one", 11),
        "blank_after_header": (b">one\n\nACGT\n", "after_blank", b"one", 6),
        "empty": (b"", "none", b"", 0),
    }
    return good, bad


GOOD, BAD = _cases()


def bad_message(name):
    text, what, contig, byte = BAD[name]
    return "%s (contig '%s', byte %d)" % (WHAT[what], contig.decode(), byte)


def edge_fasta(length, width, seed=3):
    """one contig of `length` bases between two others, lines of `width`"""
    rng = random.Random(seed * 1000003 + length * 131 + width)
    return fasta([(b"head", rand_bases(rng, 33)), (b"edge_%d_%d" % (length, width), rand_bases(rng, length, b"ACGTacgtN")), (b"tail", rand_bases(rng, 17))], width)


# ---------------------------------------------------------------- NM and MD
NT16 = {ch: i for i, ch in enumerate("=ACMGRSVTWYHKDBN") if i}


def nt16(byte):
    return NT16.get(chr(byte).upper(), 15)


def parse(rec):
    bs, tid, pos, l_name, mapq, _bin, n_cig, flag, l_seq = struct.unpack_from("<IiiBBHHHi", rec)
    at = 36 + l_name
    cig = [struct.unpack_from("<I", rec, at + 4 * k)[0] for k in range(n_cig)]
    at += 4 * n_cig
    codes = [(rec[at + (i >> 1)] >> (4 if i % 2 == 0 else 0)) & 15 for i in range(l_seq)]
    return dict(tid=tid, pos=pos, flag=flag, cig=[(w & 15, w >> 4) for w in cig], codes=codes, l_seq=l_seq)


def nm_md(rec, contigs, tid_map=None):
    """(nm, md bytes) of one block_size-prefixed record; contigs: [bytes]"""
    p = parse(rec)
    n_map = len(contigs) if tid_map is None else len(tid_map)
    if p["flag"] & 4 or p["tid"] < 0 or p["tid"] >= n_map or p["pos"] < 0 or not p["cig"] or p["l_seq"] == 0:
        return -1, b""
    c = p["tid"] if tid_map is None else tid_map[p["tid"]]
    if c < 0:
        return -1, b""
    ref, x, y, u, nm, md, stop = contigs[c], p["pos"], 0, 0, 0, bytearray(), False
    for op, ln in p["cig"]:
        if stop:
            break
        if op in (0, 7, 8):
            for _ in range(ln):
                if x >= len(ref) or y >= p["l_seq"]:
                    stop = True
                    break
                c1, c2 = p["codes"][y], nt16(ref[x])
                if (c1 == c2 and c1 != 15) or c1 == 0:
                    u += 1
                else:
                    md += b"%d" % u + bytes([ref[x]]).upper()
                    nm, u = nm + 1, 0
                x, y = x + 1, y + 1
        elif op == 2:
            md += b"%d^" % u
            for _ in range(ln):
                if x >= len(ref):
                    stop = True
                    break
                md += bytes([ref[x]]).upper()
                x, nm = x + 1, nm + 1
            u = 0
        elif op == 1:
            nm, y = nm + ln, y + ln
        elif op == 4:
            y += ln
        elif op == 3:
            x += ln
    md += b"%d" % u
    return nm, bytes(md)


def raw_record(name, flag, tid, pos, cig_words, seq, aux=b"", mapq=30):
    """a record whose CIGAR is given as (op code, len) pairs: every op code 0..15 can be written"""
    r = bytearray(bu.bam_record(name, flag=flag, refid=tid, pos=pos, mapq=mapq, cigar=[("M", 1)] * len(cig_words), seq=seq, aux=aux))
    at = 36 + len(name) + 1
    for k, (op, ln) in enumerate(cig_words):
        struct.pack_into("<I", r, at + 4 * k, ln << 4 | op)
    return bytes(r)


# the contigs the record cases are walked against: upper case, lower case with IUPAC and N, a short one
REC_CONTIGS = [b"ACGTACGTACGGTTCAAGCTTGACCATGGATCCNNACGTTGCAAGGCTTACGATCGATCGGATTACA", b"acgtnryacgtacgtkmswbdhvacgtacgtacgtacgt", b"ACGTACGT"]


def _read(contig, pos, n):
    return "".join(c if c in "ACGT" else "N" for c in contig[pos:pos + n].decode().upper())


def _record_cases():
    A, B, S = REC_CONTIGS
    M, I, D, N, Sc, H, P, EQ, X = range(9)
    out = []
    add = lambda name, *a, **k: out.append((name, raw_record(name, *a, **k)))
    add("perfect", 0, 0, 4, [(M, 20)], _read(A, 4, 20))
    add("one_mismatch", 0, 0, 4, [(M, 20)], _read(A, 4, 9) + "A" + _read(A, 14, 10))
    add("mismatch_first_and_last", 0, 0, 0, [(M, 12)], "C" + _read(A, 1, 10) + "A")
    add("all_mismatch", 0, 0, 0, [(M, 8)], "TTTTTTTT")
    add("every_op", 0, 0, 2, [(H, 3), (Sc, 2), (M, 5), (I, 2), (M, 4), (D, 3), (M, 4), (N, 6), (P, 1), (EQ, 5), (X, 2), (Sc, 1), (H, 2)] + [(op, 3) for op in range(9, 16)],
        "GG" + _read(A, 2, 5) + "TT" + _read(A, 7, 4) + _read(A, 14, 4) + _read(A, 24, 5) + "AA" + "C")
    add("ops_9_to_15_only", 0, 0, 2, [(op, 4) for op in range(9, 16)], "ACGT")
    add("lead_soft", 0, 0, 5, [(Sc, 4), (M, 10)], "TTTT" + _read(A, 5, 10))
    add("trail_soft", 0, 0, 5, [(M, 10), (Sc, 4)], _read(A, 5, 10) + "TTTT")
    add("lead_hard", 0, 0, 5, [(H, 4), (M, 10)], _read(A, 5, 10))
    add("trail_hard", 0, 0, 5, [(M, 10), (H, 4)], _read(A, 5, 10))
    add("hard_and_soft_both_ends", 0, 0, 5, [(H, 1), (Sc, 2), (M, 10), (Sc, 3), (H, 4)], "GG" + _read(A, 5, 10) + "CCC")
    add("ins_next_to_mismatch", 0, 0, 3, [(M, 5), (I, 2), (M, 5)], _read(A, 3, 4) + "A" + "GG" + "T" + _read(A, 9, 4))
    add("del_next_to_mismatch", 0, 0, 3, [(M, 5), (D, 2), (M, 5)], _read(A, 3, 4) + "A" + "A" + _read(A, 11, 4))
    add("del_at_start", 0, 0, 6, [(D, 3), (M, 8)], _read(A, 9, 8))
    add("del_after_del", 0, 0, 6, [(M, 2), (D, 1), (D, 2), (M, 4)], _read(A, 6, 2) + _read(A, 11, 4))
    add("n_in_read", 0, 0, 4, [(M, 10)], _read(A, 4, 4) + "N" + _read(A, 9, 5))
    add("n_in_reference", 0, 0, 28, [(M, 12)], _read(A, 28, 12))
    add("n_in_both", 0, 0, 30, [(M, 8)], "CCCNNACG")
    add("iupac_read", 0, 0, 0, [(M, 8)], "RCGTMCGW")
    add("eq_in_read", 0, 0, 4, [(M, 8)], "=C=T====")
    add("lower_case_reference", 0, 1, 0, [(M, 20)], "ACGTNRYACGTACGTKMSWB")
    add("lower_case_mismatch_and_del", 0, 1, 7, [(M, 4), (D, 4), (M, 6)], "ACTT" + "MSWBDT")
    add("off_end_in_m", 0, 2, 4, [(M, 10)], "ACGTACGTAC")
    add("off_end_in_m_with_mismatch", 0, 2, 5, [(M, 3), (M, 10)], "CGAACGTACGTAC")
    add("off_end_in_d", 0, 2, 2, [(M, 3), (D, 9), (M, 4)], "GTAACGT")
    add("d_at_the_end_exactly", 0, 2, 2, [(M, 3), (D, 3), (M, 4)], "GTAACGT")
    add("d_past_the_end", 0, 2, 6, [(M, 2), (N, 5), (D, 2), (M, 2)], "GTAC")
    add("pos_at_the_end", 0, 2, 8, [(M, 4)], "ACGT")
    add("n_skip_past_the_end", 0, 2, 2, [(M, 2), (N, 100), (M, 2)], "GTAC")
    add("cigar_longer_than_read", 0, 0, 0, [(M, 12)], "ACGTAC")
    add("insert_longer_than_read", 0, 0, 0, [(M, 2), (I, 9), (M, 4)], "ACGTAC")
    add("zero_length_ops", 0, 0, 3, [(M, 0), (D, 0), (M, 6), (I, 0)], _read(A, 3, 6))
    add("run_of_ten", 0, 0, 0, [(M, 11)], _read(A, 0, 10) + "A")
    add("unmapped_flag", 4, 0, 4, [(M, 4)], "ACGT")
    add("tid_minus_one", 0, -1, 4, [(M, 4)], "ACGT")
    add("tid_out_of_range", 0, 3, 4, [(M, 4)], "ACGT")
    add("pos_negative", 0, 0, -1, [(M, 4)], "ACGT")
    add("no_cigar", 0, 0, 4, [], "ACGT")
    add("l_seq_0", 0, 0, 4, [(M, 4)], "")
    add("with_aux", 16, 0, 4, [(M, 6)], _read(A, 4, 6), aux=b"NMC\x05MDZ6\x00")
    add("cigar_70_ops", 0, 0, 0, [(M, 1), (I, 1)] * 34 + [(M, 2)], "".join(_read(A, i, 1) + "T" for i in range(34)) + _read(A, 34, 2))
    return out


REC_CASES = _record_cases()


def truncated(rec):
    """damaged copies of a record: cut, cut inside the fixed part, n_cigar past block_size, l_seq past block_size"""
    return [rec[:-1], rec[:20], rec[:16] + b"\xff\xff" + rec[18:], rec[:20] + struct.pack("<i", 1 << 20) + rec[24:]]


def bulk_contigs(seed=17):
    rng = random.Random(seed)
    return [rand_bases(rng, 30000, b"ACGTACGTACGTACGTacgtN"), rand_bases(rng, 5000), rand_bases(rng, 300, b"ACGTRYKMSWN")]


def bulk_records(contigs, n=2000, seed=23):
    """generated records: read lengths 1..20 000, CIGARs of up to some 200 ops, mismatches, every op, walks off the contig's end, ineligible ones"""
    rng = random.Random(seed)
    lengths = [1, 2, 63, 64, 65, 127, 128, 129, 511, 512, 513, 20000, 12000, 4097] + [rng.choice((rng.randint(1, 40), rng.randint(41, 300), rng.randint(301, 2500))) for _ in range(n - 14)]
    out = []
    for i, ls in enumerate(lengths):
        tid = rng.choice((0, 0, 0, 1, 2)) if ls <= 250 else (0 if ls > 4000 else rng.choice((0, 1)))
        ref = contigs[tid]
        near_end = rng.random() < 0.08
        pos = max(0, len(ref) - rng.randint(1, max(1, ls))) if near_end else rng.randint(0, max(0, len(ref) - ls - 50))
        many = rng.random() < 0.15
        cig, seq, x, left = [], [], pos, ls
        if rng.random() < 0.2:
            cig.append((5, rng.randint(1, 9)))
        if left > 2 and rng.random() < 0.3:
            k = rng.randint(1, min(left - 1, 30))
            cig.append((4, k)); seq.append(_read(contigs[1], 0, k).ljust(k, "A")); left -= k
        tail = rng.randint(1, 6) if rng.random() < 0.2 and left > 6 else 0
        left -= tail
        while left > 0:
            r = rng.random()
            if r < 0.62 or not cig or cig[-1][0] not in (0, 7, 8):
                k = rng.randint(1, min(left, 4 if many else max(1, left // 2)))
                s = list(_read(ref, x, k).ljust(k, "G"))
                for j in range(k):
                    if rng.random() < 0.04:
                        s[j] = rng.choice("ACGTN=")
                cig.append((rng.choice((0, 0, 0, 7, 8)), k)); seq.append("".join(s)); x += k; left -= k
            elif r < 0.74:
                k = rng.randint(1, min(left, 12))
                cig.append((1, k)); seq.append("".join(rng.choice("ACGT") for _ in range(k))); left -= k
            elif r < 0.88:
                k = rng.randint(1, 15)
                cig.append((2, k)); x += k
            elif r < 0.94:
                k = rng.randint(1, 400)
                cig.append((3, k)); x += k
            else:
                cig.append((rng.choice((6, 9, 12, 15)), rng.randint(0, 5)))
        if tail:
            cig.append((4, tail)); seq.append("T" * tail)
        flag = rng.choice((0, 0, 0, 16, 16, 4, 256, 2048))
        if rng.random() < 0.03:
            tid = rng.choice((-1, 3, 7))
        out.append(raw_record("b%d" % i, flag, tid, -1 if rng.random() < 0.01 else pos, cig[:65535], "".join(seq), mapq=rng.choice((0, 10, 30, 60))))
    return out


def stream_of(recs):
    off = [0]
    for r in recs:
        off.append(off[-1] + len(r))
    return b"".join(recs), off
