"""The rules of include/seqlib_amd_win.h restated in Python, for tests/test_win_host.py, tests/test_gpu_win.py and tests/test_cpp_win.py: the loop
`for record: for window it overlaps: AddRead(record)` written record by record and base by base -- no offsets, no tiles, no sort.  The overlap test is
tests/grc_util.py's (the "records" rule of the interval unit).  It also holds the record cases both sides run."""
import random
import struct

from tests import bam_util as bu
from tests import grc_util as gu

SEQ_CODES = "=ACMGRSVTWYHKDBN"
KEEP, SKIP_FLAG, NO_SEQ, NO_NAME, TRIMMED = 0, 1, 2, 3, 4
# the edges of the nibble pair, the 16-byte store, the ballot, the "wave_len" knob and the tile
EDGE_LENGTHS = (1, 2, 15, 16, 17, 31, 32, 33, 63, 64, 65, 511, 512, 513, 2047, 2048, 2049, 4097)


class BadRecord(Exception):
    pass


class Rules:
    def __init__(self, skip_flags=0, qual_trim=-1, original_strand=0):
        self.skip_flags, self.qual_trim, self.original_strand = skip_flags, qual_trim, original_strand


def quality_trim(qual, t):
    """BamRecord::QualityTrimmedSequence (reference src/BamRecord.cpp:591-624) on the phred bytes -> (startpoint, endpoint)"""
    if len(qual) == 0 or qual[0] == 0xff:
        return 0, -1
    ok = [i for i, q in enumerate(qual) if q >= t]
    if not ok:
        return len(qual), -1
    return ok[0], ok[-1] + 1


def fields(rec):
    """the fixed part of one block_size-prefixed record whose block_size fills it -> (flag, l_name, l_seq, seq_at); BadRecord when fields pass the record or the
    name does not end in NUL"""
    if len(rec) < 36:
        raise BadRecord("short")
    l_name, n_cig, flag = rec[12], struct.unpack_from("<H", rec, 16)[0], struct.unpack_from("<H", rec, 18)[0]
    l_seq = struct.unpack_from("<i", rec, 20)[0]
    if l_seq < 0:
        raise BadRecord("l_seq")
    seq_at = 36 + l_name + 4 * n_cig
    if seq_at + (l_seq + 1) // 2 + l_seq > len(rec):
        raise BadRecord("fields pass block_size")
    if l_name >= 1 and rec[36 + l_name - 1] != 0:
        raise BadRecord("name without NUL")
    return flag, l_name, l_seq, seq_at


def read_of(rec, rules):
    """-> (status, bases, quals): what AddRead(record) adds, as bytes, or why it adds nothing"""
    flag, l_name, l_seq, seq_at = fields(rec)
    if flag & rules.skip_flags:
        return SKIP_FLAG, b"", b""
    if l_seq == 0:
        return NO_SEQ, b"", b""
    if l_name <= 1:
        return NO_NAME, b"", b""
    packed, qual = rec[seq_at:seq_at + (l_seq + 1) // 2], rec[seq_at + (l_seq + 1) // 2:seq_at + (l_seq + 1) // 2 + l_seq]
    seq = "".join(SEQ_CODES[(packed[i >> 1] >> (0 if i & 1 else 4)) & 15] for i in range(l_seq))
    a, b = 0, l_seq
    if rules.qual_trim >= 0:
        s, e = quality_trim(qual, rules.qual_trim)
        if e < 0 and s != 0:
            return TRIMMED, b"", b""
        if e >= 0:
            a, b = s, e
    seq, qual = seq[a:b], qual[a:b]
    if rules.original_strand and flag & 0x10:
        seq, qual = bu.revcomp(seq), qual[::-1]
    return KEEP, seq.encode(), bytes((q + 33) & 255 for q in qual)


def first_bad(stream, off):
    """the lowest record index the add names with SLX_EIO, or None: the editor's extent test, then fields()"""
    n, nb, base = len(off) - 1, len(stream), off[0] if off else 0
    ld = lambda at: struct.unpack_from("<I", stream, at)[0]
    ok = lambda a, b: b > a and b <= nb and b - a >= 36 and b - a <= 0xffffffff
    if n == 0:
        return 0 if nb else None
    for i in range(n):
        if off[i] < base or off[i + 1] < base:
            return i
        a, b = off[i] - base, off[i + 1] - base
        if i > 0:
            z = off[i - 1] - base
            if ok(z, a) and ld(z) + 4 != a - z:
                return i
        if not ok(a, b):
            return i
        own = ld(a) + 4 == b - a
        if i + 1 == n and (b != nb or not own):
            return i
        if own:
            try:
                fields(stream[a:b])
            except BadRecord:
                return i
    return None


def collect(windows, batches, rules=None):
    """windows: [(chr, pos1, pos2)]; batches: lists of records, in the order of the adds -> (bases, quals, offs, win_off, rec_of_read, statuses)"""
    rules = rules or Rules()
    per = [[] for _ in windows]
    ordinal, statuses = 0, []
    for recs in batches:
        for r in recs:
            st, b, q = read_of(r, rules)
            statuses.append(st)
            if st == KEEP:
                iv = gu.record_iv(r)
                for w, win in enumerate(windows):
                    if gu.is_hit(win, iv):
                        per[w].append((ordinal, b, q))
            ordinal += 1
    bases, quals, offs, win_off, ror = b"", b"", [0], [0], []
    for reads in per:
        for o, b, q in reads:
            bases += b
            quals += q
            offs.append(len(bases))
            ror.append(o)
        win_off.append(len(ror))
    return bases, quals, offs, win_off, ror, statuses


# ---- records
def rand_seq(rng, n, alphabet="ACGT"):
    return "".join(rng.choice(alphabet) for _ in range(n))


def record(name, tid, pos, seq, qual=None, flag=0, cigar=None):
    """a mapped record with one M over its sequence (or the cigar given) at its position"""
    if cigar is None:
        cigar = [("M", len(seq))] if seq and not flag & 4 else []
    return bu.bam_record(name, flag=flag, refid=tid, pos=pos, mapq=30, cigar=cigar, seq=seq, qual=qual)


def edge_records(seed=7, tid=0, pos0=1000, step=10):
    """one record per edge length, every code of the alphabet among them, qualities 0 .. 93 and a 0xff-filled one, every other one on the reverse strand"""
    rng = random.Random(seed)
    out = []
    for k, n in enumerate(EDGE_LENGTHS):
        seq = rand_seq(rng, n, SEQ_CODES if k % 3 == 0 else "ACGT")
        qual = None if k % 5 == 4 else bytes(rng.randrange(0, 94) for _ in range(n))
        out.append(record("e%d" % n, tid, pos0 + step * k, seq, qual, flag=0x10 if k % 2 else 0))
    return out


def profile_quals(n, t):
    """the quality profiles of the trim, for a read of n bases and a threshold t: name -> phred bytes"""
    lo, hi = max(t - 1, 0), min(max(t, 0), 93)
    p = {"all_below": bytes([lo]) * n, "all_above": bytes([hi]) * n}
    if n:
        p["first_only"] = bytes([hi]) + bytes([lo]) * (n - 1)
        p["last_only"] = bytes([lo]) * (n - 1) + bytes([hi])
        p["filler"] = b"\xff" + bytes([lo]) * (n - 1)
    return p


def sim_reads(genome, lo, hi, n, tid=0, length=150, err=0.01, seed=1, prefix="s"):
    """n records of `length` bases whose alignment starts in [lo, hi - length] of `genome` (bytes), one M over the read at its position, substitution errors
    with a low quality most of the time, half of them with 0x10 (the bases as stored: the reference strand) -> records by ascending position"""
    rng = random.Random(seed)
    out = []
    for k in range(n):
        pos = rng.randrange(lo, hi - length + 1)
        b, q = bytearray(genome[pos:pos + length]), bytearray([40]) * length
        for j in range(length):
            if rng.random() < err:
                b[j] = b"ACGT"[(b"ACGT".index(b[j]) + rng.randrange(1, 4)) % 4] if b[j] in b"ACGT" else b[j]
                q[j] = 2 if rng.random() < 0.8 else 40
            elif rng.random() < 0.05:
                q[j] = 2
        out.append((pos, record("%s%d" % (prefix, k), tid, pos, b.decode(), bytes(q), flag=0x10 if rng.random() < 0.5 else 0)))
    return [r for _, r in sorted(out, key=lambda x: x[0])]


# the end-to-end case: two overlapping windows of 4 000 bp on myc (tid 0 of its own header) at about 20-fold coverage, and a window with three reads
E2E_WINDOWS = [(0, 1000, 4999), (0, 3000, 6999), (0, 9000, 12999)]
E2E_SEED = 11


def e2e_records(myc):
    return sim_reads(myc, 1000, 7000, 800, seed=E2E_SEED) + sim_reads(myc, 9500, 10500, 3, seed=E2E_SEED + 1, prefix="t")
