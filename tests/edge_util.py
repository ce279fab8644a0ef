"""Helpers of tests/test_ref_edges_oracle.py (CPU) and tests/test_gpu_ref_edges.py (GPU): references whose contigs are there for their ENDS
(a one-base contig, a contig shorter than min_seed_len, a contig as long as a read, N holes, a copy on another contig, hundreds of tiny
contigs), the reads that sit on those ends, and a second, plain derivation of what an index over such a text must hold (glibc's lrand48
for the N fills, a suffix array by sorting Python strings)."""
import struct

import numpy as np

_RC = str.maketrans("ACGTN", "TGCAN")


def revcomp(s):
    return s[::-1].translate(_RC)


def rand_seq(rng, n):
    return "".join("ACGT"[int(x)] for x in rng.integers(0, 4, n))


# ---------------------------------------------------------------- the N fills
def lrand48_draws(state, n):
    """the next n values of `lrand48() & 3` of glibc's generator from the 48-bit state `state`: X = (X * 0x5DEECE66D + 0xB) mod 2^48, lrand48() = X >> 17.
    An index build draws one per N for the pac (first pass over all contigs) and then one per N again for the BWT text (second pass)."""
    x, out = int(state) & ((1 << 48) - 1), []
    for _ in range(n):
        x = (x * 0x5DEECE66D + 0xB) & ((1 << 48) - 1)
        out.append((x >> 17) & 3)
    return out


def n_positions(seqs):
    """positions of the N (any non-ACGT) bases in the concatenated reference, in reference order"""
    return [i for i, c in enumerate("".join(seqs)) if c not in "ACGTacgt"]


def both_fills(seqs, state):
    """(pac text, BWT text) of the forward strand as a build from RNG state `state` makes them"""
    fwd = list("".join(seqs).upper())
    at = n_positions(seqs)
    d = lrand48_draws(state, 2 * len(at))
    pac, bwt = list(fwd), list(fwd)
    for k, p in enumerate(at):
        pac[p] = "ACGT"[d[k]]
        bwt[p] = "ACGT"[d[len(at) + k]]
    return "".join(pac), "".join(bwt)


# ---------------------------------------------------------------- a second derivation of the index
def brute_sa(text):
    """suffix array of forward ++ reverse complement with the empty suffix first (a shorter suffix sorts before its extensions): n + 1 entries.
    Sorting Python strings: for texts up to 4 000 symbols."""
    t = text + revcomp(text)
    assert len(t) <= 4000
    return sorted(range(len(t) + 1), key=lambda i: t[i:])


def sa_file(prefix):
    """<prefix>.sa: primary at byte 0, sa_intv at 40, seq_len at 48, then the samples sa[intv], sa[2 intv], ... from byte 56"""
    b = open(prefix + ".sa", "rb").read()
    primary, = struct.unpack_from("<Q", b, 0)
    intv, seq_len = struct.unpack_from("<QQ", b, 40)
    samples = np.frombuffer(b, dtype="<u8", offset=56)
    assert len(samples) == (seq_len + intv) // intv - 1
    return dict(primary=int(primary), sa_intv=int(intv), seq_len=int(seq_len), samples=[int(x) for x in samples])


def pac_text(prefix, total):
    """the forward strand as <prefix>.pac holds it (N positions carry the first-pass draws)"""
    b = np.frombuffer(open(prefix + ".pac", "rb").read(), dtype=np.uint8)
    p = np.arange(total)
    codes = (b[p >> 2] >> ((~p & 3) << 1)) & 3
    return "".join("ACGT"[int(c)] for c in codes)


def check_against_brute_sa(prefix, bwt_text):
    """primary and every sample of <prefix>.sa against brute_sa of the BWT text"""
    sa = brute_sa(bwt_text)
    f = sa_file(prefix)
    n = 2 * len(bwt_text)
    assert f["seq_len"] == n and f["sa_intv"] == 32
    assert f["primary"] == sa.index(0), "primary %d, sorted suffixes say %d" % (f["primary"], sa.index(0))
    assert f["samples"] == [sa[i] for i in range(32, n + 1, 32)]


# ---------------------------------------------------------------- a property of every record
_REF_OPS = (0, 2, 3, 7, 8)          # M D N = X consume the reference


def inside_contig(out, lens):
    """every record of the SoA result `out` lies inside its contig: pos >= 0 and pos + (reference bases of its CIGAR) <= len(contig rid)"""
    for k in range(len(out["rid"])):
        c0, c1 = int(out["cig_off"][k]), int(out["cig_off"][k + 1])
        reflen = sum(int(w) >> 4 for w in out["cigar"][c0:c1] if (int(w) & 0xf) in _REF_OPS)
        rid, pos = int(out["rid"][k]), int(out["pos"][k])
        assert 0 <= rid < len(lens), "record %d: rid %d" % (k, rid)
        assert pos >= 0 and pos + reflen <= lens[rid], "record %d: [%d, %d) on contig %d of %d bases" % (k, pos, pos + reflen, rid, lens[rid])
    return True


def records(out):
    """the records of an SoA result as dicts, in order"""
    recs = []
    for k in range(len(out["rid"])):
        c0, c1 = int(out["cig_off"][k]), int(out["cig_off"][k + 1])
        recs.append(dict(rid=int(out["rid"][k]), pos=int(out["pos"][k]), flag=int(out["flag"][k]), mapq=int(out["mapq"][k]), AS=int(out["score"][k]),
                         NM=int(out["nm"][k]), cigar=[int(w) for w in out["cigar"][c0:c1]]))
    return recs


# ---------------------------------------------------------------- three forms of a read, both strands
def edge_forms(read, edge_at, rng):
    """the read as it is; with one substitution within 5 bases of edge_at and one in the interior; with a 2-base insertion and a 3-base deletion
    within 30 bases of edge_at (no diagonal answers that one: the DP runs into the clipped window) -- and the reverse complement of each"""
    L = len(read)
    e = min(max(int(edge_at), 0), L - 1)

    def other(c):
        return "ACGT"[("ACGT".find(c) + 1 + int(rng.integers(0, 3))) % 4] if c in "ACGT" else "A"

    sub = list(read)
    p = min(max(e + int(rng.integers(-5, 6)), 0), L - 1)
    sub[p] = other(sub[p])
    far = [q for q in range(10, L - 10) if abs(q - e) > 15] or [q for q in range(L) if q != p]
    q = far[int(rng.integers(0, len(far)))]
    sub[q] = other(sub[q])
    # the two indels 8 to 30 bases from the edge, one on each side of it where the read has room, otherwise both on the side that has
    lo, hi = 6, L - 9
    a = e - int(rng.integers(8, 31))
    b = e + int(rng.integers(8, 28))
    if a < lo:
        a = min(b + 12, hi)
    if b > hi:
        b = max(min(a, e) - 12, lo)
    a, b = min(max(a, lo), hi), min(max(b, lo), hi)
    ind = list(read)
    first, second = max(a, b), min(a, b)          # edit the later position first so the earlier one keeps its index
    del ind[first:first + 3]
    ind[second:second] = list(other(read[second]) + other(read[second - 1]))
    forms = [read, "".join(sub), "".join(ind)]
    return forms + [revcomp(f) for f in forms]


# ---------------------------------------------------------------- the references
def edge_ref(trim_last=0):
    """EDGE: 6 269 bp (total % 64 == 61); trim_last = 61 gives EDGE64 (2 * total a multiple of 128)"""
    rng = np.random.default_rng(20241)
    c0 = rand_seq(rng, 3000)
    short = rand_seq(rng, 18)
    hole = rand_seq(rng, 170) + "N" * 60 + rand_seq(rng, 120) + "N" + rand_seq(rng, 49)
    readlen = rand_seq(rng, 150)
    copy = c0[1000:1400] + rand_seq(rng, 300)
    last = rand_seq(rng, 2000)
    refs = [("c0", c0), ("one", "A"), ("short", short), ("hole", hole), ("readlen", readlen), ("copy", copy), ("last", last[:2000 - trim_last])]
    total = sum(len(s) for _, s in refs)
    assert (total == 6269 and total % 64 == 61) if trim_last == 0 else (2 * total) % 128 == 0
    return refs


def tiny300_ref():
    rng = np.random.default_rng(20242)
    return [("t%03d" % i, rand_seq(rng, int(rng.integers(20, 61)))) for i in range(300)]


def long3_ref():
    rng = np.random.default_rng(20243)
    return [("A", rand_seq(rng, 80000)), ("B", rand_seq(rng, 12000)), ("C", rand_seq(rng, 30000))]


def rep_ref(c_state):
    """the repeat filter's case: ... X N Y ... X c Y ... in one contig, c = the BWT text's draw for that N, so that the BWT text holds the 81-mer X c Y
    twice and the pac only when both draws agree.  Returns (refs, read, draws): the read is X c Y with 30 bases of the first copy's flanks on each side.
    (300 random bases before and after: the first copy needs a left flank, and the aligner builds its repeat filter for texts of 1 024 symbols and more.)"""
    rng = np.random.default_rng(20244)
    X, Y = rand_seq(rng, 40), rand_seq(rng, 40)
    left, mid, right = rand_seq(rng, 300), rand_seq(rng, 200), rand_seq(rng, 300)
    d = lrand48_draws(c_state, 2)
    c = "ACGT"[d[1]]
    ref = left + X + "N" + Y + mid + X + c + Y + right
    return [("rep", ref)], left[-30:] + X + c + Y + mid[:30], d


def offsets(refs):
    off, o = [], 0
    for _, s in refs:
        off.append(o)
        o += len(s)
    return off


# ---------------------------------------------------------------- the reads
def edge_reads(refs, F, seed=5):
    """(label, read, edge_at) for EDGE / EDGE64: reads over every junction, over the forward / reverse boundary, at the first and last bases of the
    reference, a whole contig, and the copy.  F: the forward strand as the pac has it."""
    rng = np.random.default_rng(seed)
    d = dict(refs)
    off = offsets(refs)
    c0, last, readlen = d["c0"], d["last"], d["readlen"]
    out = []
    for k in range(1, len(refs)):
        j = off[k]
        if j - 75 >= 0 and j + 75 <= len(F):
            out.append(("junction %s|%s" % (refs[k - 1][0], refs[k][0]), F[j - 75:j + 75], 75))
    o1 = off[[n for n, _ in refs].index("one")]
    out.append(("c0|one|short|hole", F[o1 - 100:o1 + 50], 100))
    out.append(("strand boundary 75+75", last[-75:] + revcomp(last[-75:]), 75))
    out.append(("strand boundary 100+50", last[-100:] + revcomp(last[-50:]), 100))
    out.append(("first 150", c0[:150], 0))
    out.append(("20 random + first 130", rand_seq(rng, 20) + c0[:130], 20))
    out.append(("last 150", last[-150:], 149))
    out.append(("last 130 + 20 random", last[-130:] + rand_seq(rng, 20), 130))
    out.append(("insertion 5 before the end", last[-140:-5] + "ACGTA" + last[-5:], 140))
    out.append(("deletion 5 after the start", c0[:5] + c0[12:157], 5))
    out.append(("whole contig", readlen, 0))
    out.append(("whole contig + 10 on each side", rand_seq(rng, 10) + readlen + rand_seq(rng, 10), 10))
    out.append(("the copy", c0[1100:1250], 75))
    return out


def n_junction_reads(refs):
    return len(refs) - 1


def tiny300_reads(F):
    return [F[p:p + 150] for p in range(0, len(F) - 150, 53)]


def with_forms(reads, seed=9):
    """every (label, read, edge_at) through edge_forms -> flat list of reads"""
    rng = np.random.default_rng(seed)
    out = []
    for _, r, e in reads:
        out += edge_forms(r, e, rng)
    return out


def mut_long(rng, t, n_sub, indel=True):
    """substitutions plus one insertion and one deletion (as the long-read tests mutate their contigs)"""
    t = list(t)
    for _ in range(n_sub):
        t[int(rng.integers(0, len(t)))] = "ACGT"[int(rng.integers(0, 4))]
    if indel:
        q = len(t) // 3
        t[q:q] = list("ACGTTGCAACGT")
        del t[2 * q:2 * q + 9]
    return "".join(t)


def long3_reads(refs, seed=31):
    """(label, read, contigs it touches in reference order) for LONG3, then the same reads mutated"""
    rng = np.random.default_rng(seed)
    A, B, C = (s for _, s in refs)
    base = [("A|B 600+600", A[-600:] + B[:600], (0, 1)),
            ("revcomp B|C 1500+1500", revcomp(B[-1500:] + C[:1500]), (1, 2)),
            ("A|B 4500+4500", A[-4500:] + B[:4500], (0, 1)),
            ("A|B|C", A[-4000:] + B + C[:4000], (0, 1, 2)),
            ("A|B 66000+4000", A[-66000:] + B[:4000], (0, 1)),
            ("strand boundary 5000+5000", C[-5000:] + revcomp(C[-5000:]), (2, 2)),
            ("500 random + A's start", rand_seq(rng, 500) + A[:8500], (0,)),
            ("C's end + 700 random", C[-9000:] + rand_seq(rng, 700), (2,)),
            ("revcomp B", revcomp(B), (1,))]
    muts = [(lab + ", mutated", mut_long(rng, r, max(3, len(r) // 2000)), t) for lab, r, t in base]
    return base, muts


def hole_reads(refs, F_pac, F_bwt, seed=13):
    """Part D: (label, pac form, bwt form) of the reads over the holes of EDGE's `hole` contig"""
    rng = np.random.default_rng(seed)
    names = [n for n, _ in refs]
    oh = offsets(refs)[names.index("hole")]
    hole = dict(refs)["hole"]
    h0, s1 = oh + 170, oh + 170 + 60 + 120
    out = []
    for lab, a, b in (("45 + hole + 45", h0 - 45, h0 + 105), ("ends 10 bases inside the hole", h0 - 140, h0 + 10), ("the single N, 70 on each side", s1 - 70, s1 + 71)):
        out.append((lab, F_pac[a:b], F_bwt[a:b]))
    out.append(("the hole as given", hole[120:270], hole[120:270]))
    filled = F_pac[h0 - 45:h0] + rand_seq(rng, 60) + F_pac[h0 + 60:h0 + 105]
    out.append(("random bases for the hole", filled, filled))
    return out
