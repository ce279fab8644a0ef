"""The rules of include/seqlib_amd_grc.h restated in Python by brute force, for tests/test_grc_host.py, tests/test_gpu_grc.py and tests/test_cpp_grc.py: every
(query, subject) pair is tested, the hits are sorted as the header orders them, merge is a plain sweep over a sorted copy, a width is the union of the clipped hits
by another sweep, and a record's interval comes from tests/cov_util.py's parser.  Written from the rules, not from csrc/grc_host.h: no binary search, no running
maximum, no end-sorted array on the query side.  It also holds the named list of cases both sides run."""
import random

from tests import cov_util as cu

INT32_MAX, INT32_MIN = 2 ** 31 - 1, -2 ** 31


def norm(iv):
    """(chr, pos1, pos2) or (chr, pos1, pos2, strand) -> the four"""
    return (iv[0], iv[1], iv[2], iv[3] if len(iv) > 3 else "*")


def is_hit(s, q, ignore_strand=True, contained=False):
    s, q = norm(s), norm(q)
    if s[0] != q[0] or s[2] < q[1] or s[1] > q[2]:
        return False
    if not ignore_strand and s[3] != q[3]:
        return False
    return not contained or (s[1] >= q[1] and s[2] <= q[2])


def hits(subjects, q, ignore_strand=True, contained=False):
    """-> [(subject id, clipped pos1, clipped pos2)] by ascending (pos1, pos2, subject id) of the subject"""
    found = sorted((s[1], s[2], i) for i, s in enumerate(subjects) if is_hit(s, q, ignore_strand, contained))
    return [(i, max(p1, q[1]), min(p2, q[2])) for p1, p2, i in found]


def width(clipped):
    """positions covered by the closed intervals [(pos1, pos2)]"""
    total, reach = 0, None
    for a, b in sorted(clipped):
        if reach is None or a > reach:
            total += b - a + 1
            reach = b
        elif b > reach:
            total += b - reach
            reach = b
    return total


def join(subjects, queries, ignore_strand=True):
    """-> (pairs [(query id, subject id, clipped pos1, clipped pos2)], counts, widths)"""
    pairs, counts, widths = [], [], []
    for qi, q in enumerate(queries):
        h = hits(subjects, q, ignore_strand)
        pairs += [(qi,) + x for x in h]
        counts.append(len(h))
        widths.append(width([(a, b) for _, a, b in h]))
    return pairs, counts, widths


def sorted_index(subjects):
    """-> (sorted intervals, perm, run_p2, ends): the arrays slx_grc_sorted gives"""
    perm = sorted(range(len(subjects)), key=lambda i: (subjects[i][0], subjects[i][1], subjects[i][2], i))
    srt = [norm(subjects[i]) for i in perm]
    run, ends = [], []
    for i, s in enumerate(srt):
        run.append(max(x[2] for x in srt[:i + 1] if x[0] == s[0]))
    for c in sorted(set(s[0] for s in srt)):
        ends += sorted(s[2] for s in srt if s[0] == c)
    return srt, perm, run, ends


def merge(subjects):
    """GenomicRegionCollection.cpp:267-306: touching intervals merge, adjacent ones do not; the first member's pos1 and strand, the run's largest pos2"""
    out = []
    for s in sorted_index(subjects)[0]:
        if out and out[-1][0] == s[0] and out[-1][2] >= s[1]:
            out[-1] = (out[-1][0], out[-1][1], max(out[-1][2], s[2]), out[-1][3])
        else:
            out.append(s)
    return out


def record_iv(r):
    """(tid, pos, end) of a block_size-prefixed record: end = pos + reference length, pos + 1 when that is 0 or the record is unmapped"""
    tid, pos, _mapq, flag, ops = cu.parse(r)
    reflen = sum(ln for op, ln in ops if op in cu.REF_OPS)
    return (tid, pos, pos + (1 if reflen == 0 or flag & 4 else reflen))


def subject_counts(subjects, recs):
    return [sum(1 for r in recs if is_hit(s, record_iv(r))) for s in subjects]


# ---- the cases
CHRS = (0, 1, 2)


def random_subjects(n, seed):
    """exon-like intervals over three chr values, one on a negative chr and one on a chr no query uses (from the third on)"""
    rng = random.Random(seed)
    out = []
    for i in range(n):
        chr_ = -3 if i == 2 else 7 if i == 3 else rng.choice(CHRS)
        p1 = rng.randrange(0, 3000)
        out.append((chr_, p1, p1 + rng.choice((0, 1, 5, 40, 150, 900)), rng.choice("+-*")))
    return out


def random_queries(n, seed):
    rng = random.Random(seed)
    out = []
    for _ in range(n):
        p1 = rng.randrange(-50, 3300)
        out.append((rng.choice(CHRS + (-3, 5)), p1, p1 + rng.choice((0, 3, 60, 400, 4000)), rng.choice("+-*")))
    return out


def _container():
    s = [(1, 0, 100000, "+")] + [(1, 10 * i + 5, 10 * i + 12, "-") for i in range(200)] + [(1, 90000, 90001, "*")]
    q = [(1, 0, 100000, "-"), (1, 0, 700, "*"), (1, 5, 1300, "+"), (1, 50000, 50010, "-"), (1, 50000, 50010, "+"), (1, 2008, 2008, "-"), (0, 5, 10, "*"), (1, 100001, 100002, "*")]
    return s, q


# (name, subjects, queries)
CASES = [
    ("equal_starts", [(0, 10, 20), (0, 10, 15), (0, 10, 30), (0, 10, 10), (0, 10, 15)], [(0, 10, 10), (0, 12, 18), (0, 25, 40), (0, 0, 9), (0, 0, 10)]),
    ("strands", [(0, 5, 9, "+"), (0, 5, 9, "-"), (0, 5, 9, "*"), (0, 5, 9, "+")], [(0, 5, 9, "+"), (0, 5, 9, "-"), (0, 5, 9, "*"), (0, 9, 12, "+")]),
    ("touching_adjacent", [(0, 100, 200), (0, 300, 400, "-")], [(0, 50, 100), (0, 200, 250), (0, 50, 99), (0, 201, 250), (0, 201, 299), (0, 200, 300)]),
    ("points", [(0, 7, 7), (0, 8, 8), (0, 0, 100)], [(0, 7, 7), (0, 8, 8), (0, 9, 9), (0, 6, 8), (0, 101, 101)]),
    ("container_200",) + _container(),
    ("extremes", [(0, INT32_MIN, INT32_MIN), (0, INT32_MIN, INT32_MAX), (0, 0, 0), (0, INT32_MAX, INT32_MAX), (0, 0, INT32_MAX), (-5, INT32_MIN, 0), (INT32_MAX, 1, 2), (INT32_MIN, 1, 2)],
     [(0, INT32_MIN, INT32_MAX), (0, 0, 0), (0, INT32_MAX, INT32_MAX), (0, INT32_MIN, INT32_MIN), (-5, -1, 1), (0, -1, 1), (INT32_MAX, 2, 2), (INT32_MIN, 0, 1), (-4, 0, 1)]),
    ("absent_chr", [(0, 1, 5), (2, 1, 5)], [(1, 1, 5), (99, 1, 5), (-1, 1, 5), (2, 5, 5)]),
    ("merge_shape", [(23, 10, 100), (23, 20, 110), (2, 10, 100), (2, 20, 110), (2, 200, 310)], [(23, 10, 100), (2, 105, 205)]),
    ("touch_merge", [(0, 4, 6, "-"), (0, 6, 8, "+"), (1, 4, 5), (1, 6, 7), (0, 1, 50), (0, 51, 60), (0, 60, 61)], [(0, 6, 6), (1, 5, 6)]),
] + [("subjects_%d" % n, random_subjects(n, 100 + n), random_queries(65, 200 + n)) for n in (0, 1, 63, 64, 65, 300)] \
  + [("queries_%d" % n, random_subjects(300, 7), random_queries(n, 300 + n)) for n in (0, 1, 63, 64, 65, 1000)]
CASE_IDS = [c[0] for c in CASES]


def case(name):
    return CASES[CASE_IDS.index(name)]


# ---- records: tests/cov_util.py's case records (contigs 0 .. 3 and a few outside) and regions around them
REC_SUBJECTS = [(0, 0, 0), (0, 0, 1), (1, 0, 69), (1, 10, 20), (2, 100, 150), (2, 151, 160), (2, 390, 470), (2, 500, 620), (2, 700, 727), (2, 728, 800), (2, 899, 1000), (2, 4990, 5000),
                (3, 0, 10000000), (3, 9999990, 10000001), (2, 0, 99), (2, 150, 150), (5, 0, 100), (2, 300, 301), (2, 200, 202)]


def case_records():
    return [r for _, r in cu.CASES]
