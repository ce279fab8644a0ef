"""GPU tests of the pileup unit at the C-ABI (include/seqlib_amd_pile.h through seqlib_amd/pileio.py) against the Python statement of the rules in
tests/pile_util.py: every record shape through both kernels, batch shapes with every form of the LDS window and every group width, constructed window cases with
exact event counts, contended adds, the quality and mapq floors, accumulation, the window object, candidate sites against a reference in HBM, and batches that
come from the BAM reader (whole file, filtered, regions), the SAM reader and the record builder.  Equality is exact everywhere.  The C++ class is driven in
tests/test_cpp_pile.py."""
import os
import random

import numpy as np
import pytest

from tests import bam_util as bu
from tests import pile_util as pu

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")
ALL = [r for _, r in pu.CASES]
LDS_DEFAULT = None          # the knob is left alone


@pytest.fixture(scope="module")
def io(sl):
    from seqlib_amd import _ffi, bamio, filterio, pileio, recio, refio, samio
    pileio.lib()

    class F:
        pass
    f = F()
    f.ffi, f.bamio, f.pileio, f.filterio, f.recio, f.refio, f.samio = _ffi, bamio, pileio, filterio, recio, refio, samio
    return f


def make(io, recs, window=pu.WHOLE, refs=pu.REFS, knobs=None, pieces=1):
    """a pileup object over the window with the records added through slx_pile_add_host in `pieces` batches"""
    p = io.pileio.Pile(refs, window)
    for k, v in (knobs or {}).items():
        if v is not None:
            p.set(k, v)
    step = max(1, -(-len(recs) // pieces))
    for i in range(0, max(len(recs), 1), step):
        p.add_host(*pu.stream_of(recs[i:i + step]))
    return p


def same(p, want):
    got = p.planes()
    assert got.shape == want.shape
    bad = np.argwhere(got != want)
    assert not len(bad), (bad[:5].tolist(), [int(got[tuple(b)]) for b in bad[:5]], [int(want[tuple(b)]) for b in bad[:5]])


def is_long(r, long_cigar=64, long_read=1024):
    return len(pu.parse(r)[4]) > long_cigar or len(pu.parse(r)[5]) > long_read


def split(recs, window=pu.WHOLE, refs=pu.REFS, slice_records=1024, lds_window=0, long_cigar=64, long_read=1024, **elig):
    """(events_lds, events_global) by the header's description of the kernels: a block of slice_records records keeps lds_window positions from its first eligible
    record's start (clipped to the window) in LDS; long records go to HBM only"""
    tid, beg, end = pu.window_of(window, refs)
    lds = glob = 0
    for s in range(0, len(recs), slice_records):
        block = [r for r in recs[s:s + slice_records] if pu.eligible(r, tid, **elig)]
        if not block:
            continue
        a = min(max(pu.parse(block[0])[1], beg), end)
        for r in block:
            ev = pu.clipped(pu.events(r, 0), beg, end)
            inside = 0 if is_long(r, long_cigar, long_read) else sum(a <= x < a + lds_window for _, x in ev)
            lds += inside
            glob += len(ev) - inside
    return lds, glob


@pytest.mark.parametrize("long_read", [8, 1024])
@pytest.mark.parametrize("long_cigar", [64, 1, 1 << 20])
def test_every_record_shape_through_both_kernels(io, long_cigar, long_read):
    want = pu.planes(ALL)
    n_elig = sum(pu.eligible(r, 2) for r in ALL)
    n_long = sum(pu.eligible(r, 2) and is_long(r, long_cigar, long_read) for r in ALL)
    for group in (16, 32, 64):
        p = make(io, ALL, knobs={"long_cigar": long_cigar, "long_read": long_read, "group_lanes": group})
        same(p, want)
        assert (p.counter("records_seen"), p.counter("records_counted"), p.counter("long_records")) == (len(ALL), n_elig, n_long)
        assert p.counter("events_lds") + p.counter("events_global") == int(want.sum()) and p.counter("nonsense") == -1
        p.close()
    assert sum(pu.eligible(r, 2) and is_long(r) for r in ALL) == 6 and sum(pu.eligible(r, 2) and is_long(r, 1, 8) for r in ALL) > 40
    for window in pu.WINDOWS[1:]:
        p = make(io, ALL, window, knobs={"long_cigar": long_cigar, "long_read": long_read})
        same(p, pu.planes(ALL, window))
        p.close()
    # the other eligibility knobs: no flag excluded, and a mapq floor
    p = make(io, ALL, knobs={"long_cigar": long_cigar, "long_read": long_read, "exclude_flags": 0, "min_mapq": 4})
    same(p, pu.planes(ALL, exclude_flags=0, min_mapq=4))
    assert p.counter("records_counted") == sum(pu.eligible(r, 2, 0, 4) for r in ALL) != n_elig
    p.close()


@pytest.mark.parametrize("n", [0, 1, 63, 64, 65, 1000, 3000])
def test_batch_shapes_and_every_form_of_the_window(io, n):
    recs = pu.random_records(n, seed=n + 1)
    shuffled = list(recs)
    random.Random(5).shuffle(shuffled)
    want = pu.planes(recs)
    default = None
    k = 0
    for order in (recs, shuffled):
        for lds_window in (0, 64, LDS_DEFAULT):
            for slice_records in (64, 1024):
                group = (16, 32, 64)[k % 3]
                k += 1
                p = make(io, order, knobs={"lds_window": lds_window, "slice_records": slice_records, "group_lanes": group})
                same(p, want)
                assert p.counter("records_seen") == n and p.counter("records_counted") == sum(pu.eligible(r, 2) for r in recs)
                if lds_window is not None:
                    assert (p.counter("events_lds"), p.counter("events_global")) == split(order, slice_records=slice_records, lds_window=lds_window)
                else:          # whatever the default is, it is one window for both slices of this order
                    default = default or p.counter("events_lds") + p.counter("events_global")
                    assert p.counter("events_lds") + p.counter("events_global") == default == int(want.sum())
                p.close()


def test_constructed_window_cases(io):
    def counts(recs, window=pu.WHOLE, **knobs):
        p = make(io, recs, window, knobs=knobs)
        same(p, pu.planes(recs, window))
        got = (p.counter("events_lds"), p.counter("events_global"))
        assert got == split(recs, window, lds_window=knobs.get("lds_window", 0), slice_records=knobs.get("slice_records", 1024))
        p.close()
        return got
    # a record straddling the LDS window's end: 1050 .. 1063 inside, 1064 .. 1149 outside
    assert counts([pu.rec(2, 1000, "10M"), pu.rec(2, 1050, "100M")], lds_window=64) == (24, 86)
    # one wholly outside it, and one in front of the anchor (the input is not sorted)
    assert counts([pu.rec(2, 1000, "10M"), pu.rec(2, 2000, "20M"), pu.rec(2, 900, "20M")], lds_window=64) == (10, 40)
    # a deletion and an insertion's anchor on the window's last position and one past it
    assert counts([pu.rec(2, 1000, "10M"), pu.rec(2, 1060, "4M2I4D"), pu.rec(2, 1060, "5M2I4D", flag=0x10)], lds_window=64) == (10 + 4 + 1 + 0 + 4 + 0 + 0, 4 + 1 + 1 + 4)
    # one ending on the contig's last base, one running over it, with the window anchored 20 positions in front of the contig's end
    assert counts([pu.rec(2, 4980, "20M"), pu.rec(2, 4990, "20M")], lds_window=64) == (30, 0)
    assert counts([pu.rec(2, 4999, "1M")], lds_window=64) == (1, 0)
    # a window object: the anchor is clipped to the window's begin, events in front of it are dropped
    assert counts([pu.rec(2, 90, "20M"), pu.rec(2, 150, "20M"), pu.rec(2, 290, "20M")], (2, 100, 300), lds_window=64) == (10 + 14, 6 + 10)
    # a slice whose first records are not eligible: the anchor is the first eligible one
    recs = [pu.rec(-1, -1, "", seq="", flag=4), pu.rec(2, 50, "10M", flag=0x400), pu.rec(1, 3, "10M"), pu.rec(2, 3000, "10M"), pu.rec(2, 3005, "10M")]
    assert counts(recs, lds_window=64) == (20, 0)
    # no eligible record at all
    assert counts(recs[:3], lds_window=64) == (0, 0)
    # the anchor of every slice is its own
    recs = [pu.rec(2, 40 * i, "30M") for i in range(100)]
    assert counts(recs, lds_window=64, slice_records=64) == (30 + 24 + 30 + 24, 30 * 100 - 108)
    assert counts(recs, lds_window=0) == (0, 3000)


def test_1025_records_on_one_position(io):
    recs = [pu.rec(2, 1234, "10M", seq="ACGTACGTAC")] * 1025 + [pu.rec(2, 1234, "10M", seq="ACGTTCGTAC", flag=0x10)]
    want = pu.planes(recs)
    for lds_window in (0, 64, LDS_DEFAULT):
        for group in (16, 64):
            p = make(io, recs, knobs={"lds_window": lds_window, "group_lanes": group})
            same(p, want)
            at = p.at(1238)
            assert at[pu.A] == 1025 and at[pu.REV + pu.T] == 1 and sum(at) == 1026 and p.at(1233) == [0] * 15 and p.at(5000) == [0] * 15 and p.at(-1) == [0] * 15
            assert int(p.counts(pu.A, 1234, 1235)[0]) == 1025 and p.counts_device(pu.A)[1] == 5000
            p.close()


def test_quality_and_mapq_floors_move_bases(io):
    recs = [r for r in ALL + pu.random_records(400, seed=9)]
    seen = set()
    for min_baseq in (0, 20, 41):
        for min_mapq in (0, 30):
            want = pu.planes(recs, min_baseq=min_baseq, min_mapq=min_mapq)
            p = make(io, recs, knobs={"min_baseq": min_baseq, "min_mapq": min_mapq})
            same(p, want)
            p.close()
            seen.add((int(want[pu.LOWQ].sum()), int(want.sum())))
    assert len(seen) == 6 and min(s[0] for s in seen) == 0          # a base moves between its plane, LOWQ and nothing


def test_accumulation_and_clear(io):
    recs = ALL + pu.random_records(600, seed=3)
    want = pu.planes(recs)
    one = make(io, recs)
    same(one, want)
    three = make(io, recs, pieces=3)
    same(three, want)
    p = make(io, recs[:200])
    same(p, pu.planes(recs[:200]))
    p.add_host(*pu.stream_of(recs[200:450]))
    assert p.at(104) == [int(v) for v in pu.planes(recs[:450])[:, 104]]
    p.add_host(*pu.stream_of(recs[450:]))
    p.add_host(b"", [0])
    same(p, want)
    p.clear()
    same(p, pu.planes([]))
    p.add_host(*pu.stream_of(recs))          # and it is usable afterwards
    same(p, want)
    assert p.counter("records_seen") == 2 * len(recs)
    for x in (one, three, p):
        x.close()


def test_a_broken_record_fails_the_call(io):
    good = [r for r in ALL if pu.eligible(r, 2)][:10]
    bad = bytearray(good[3])
    bad[16:18] = b"\xff\xff"          # n_cigar passes block_size
    p = io.pileio.Pile(pu.REFS, pu.WHOLE)
    with pytest.raises(io.ffi.SlxError, match="record 3 of the batch") as e:
        p.add_host(*pu.stream_of(good[:3] + [bytes(bad)] + good[3:]))
    assert e.value.code == io.ffi.SLX_EIO
    bad = bytearray(good[5])
    bad[20:24] = b"\xff\xff\xff\x7f"          # l_seq passes block_size
    with pytest.raises(io.ffi.SlxError, match="record 5 of the batch") as e:
        p.add_host(*pu.stream_of(good[:5] + [bytes(bad)] + good[5:3:-1] + [bytes(bad)]))
    assert e.value.code == io.ffi.SLX_EIO
    stream, off = pu.stream_of(good)
    for bad_off in (off[:-1] + [off[-1] + 4], [0, off[2], off[1]] + off[3:]):          # an offset past the stream; offsets that run backwards
        with pytest.raises(io.ffi.SlxError, match="of the batch") as e:
            p.add_host(stream, bad_off)
        assert e.value.code == io.ffi.SLX_EIO
    p.clear()
    p.add_host(stream, off)
    same(p, pu.planes(good))
    p.close()


@pytest.mark.parametrize("window", pu.WINDOWS[1:] + [(2, 1000, 1003), (2, 700, 700), (2, 6000, 7000), (3, 0, 200)], ids=str)
def test_window_object_equals_the_slice(io, window):
    recs = ALL + [pu.rec(2, 90, "20M"), pu.rec(2, 290, "20M"), pu.rec(2, 95, "300M"), pu.rec(2, 299, "1M"), pu.rec(2, 300, "5M"), pu.rec(2, 94, "5M"), pu.rec(2, 94, "6M")] + pu.random_records(300, seed=4, span=600)
    tid, beg, end = pu.window_of(window)
    whole = make(io, recs, (tid, 0, pu.REFS[tid][1])) if tid == 2 else None
    w = make(io, recs, window)
    want = pu.planes(recs, window)
    same(w, want)
    assert w.counts_device(0)[1] == end - beg == want.shape[1]
    if whole is not None:
        assert np.array_equal(w.planes(), whole.planes(beg, end)) and (beg == end or want.any())
        wide = w.counts(pu.A, beg - 7, end + 9)
        assert not wide[:7].any() and not wide[len(wide) - 9:].any() and np.array_equal(wide[7:len(wide) - 9], want[pu.A])
        whole.close()
    assert w.at(beg - 1) == [0] * 15 and w.at(end) == [0] * 15 and (beg == end or w.at(beg) == [int(v) for v in want[:, 0]])
    w.close()


# ---------------------------------------------------------------- candidate sites
PARAMS = [(10, 3, 1, 5), (1, 1, 0, 1), (10000, 1, 0, 1)]


def test_sites_against_tiny_fa(io, tmp_path):
    contigs = pu.fasta_contigs(os.path.join(GOLDEN, "tiny.fa"))
    refs = [(n, len(s)) for n, s in contigs]
    assert sum(l for _, l in refs) == 354751
    tid = 2
    contig = contigs[tid][1]
    edits = {1500: ("X", 1, 0), 1600: ("X", 3, 0), 1700: ("I", 2, 3), 1800: ("D", 2, 3), 1900: ("X", 7, 0), 2000: ("I", 9, 1)}
    recs = pu.cut_reads(contig, tid, 1000, 3000, 7, 120, edits)
    window = (tid, 900, 3200)
    want = pu.planes(recs, window, refs)
    ref = io.refio.Ref(os.path.join(GOLDEN, "tiny.fa"))
    p = make(io, recs, window, refs)
    same(p, want)
    n_by_param = []
    for q in PARAMS:
        exp = pu.sites(want, 900, contig, *q)
        got = p.sites(ref, tid, *q)
        assert got == exp
        assert p.counter("sites") == len(exp)
        p.sites_tsv(tmp_path / "s.tsv")
        assert (tmp_path / "s.tsv").read_bytes() == pu.tsv(exp, refs[tid][0])
        n_by_param.append(len(exp))
    pos = [s[0] for s in pu.sites(want, 900, contig, *PARAMS[0])]
    assert 1500 in pos and 1600 in pos and 1700 in pos and 1800 in pos and 1801 in pos and 1802 in pos and 1900 not in pos and 2000 not in pos
    assert n_by_param[1] > n_by_param[0] == 6 and n_by_param[2] == 0 and (tmp_path / "s.tsv").read_bytes() == b""
    pos1 = [s[0] for s in pu.sites(want, 900, contig, *PARAMS[1])]
    assert 1900 in pos1 and 2000 in pos1
    # what is refused: a contig of another length, parameters outside their ranges
    for args in ((ref, 1, 10, 3, 1, 5), (ref, 9, 10, 3, 1, 5), (ref, -1, 10, 3, 1, 5), (ref, tid, 0, 3, 1, 5), (ref, tid, 10, 0, 1, 5), (ref, tid, 10, 3, 6, 5), (ref, tid, 10, 3, -1, 5), (ref, tid, 10, 3, 0, 0)):
        with pytest.raises(io.ffi.SlxError) as e:
            p.sites(*args)
        assert e.value.code == io.ffi.SLX_EINVAL
    p.close()
    # a whole-contig object whose length is no multiple of 4, sites on its last positions
    tid = 0
    contig = contigs[tid][1]
    L = len(contig)
    recs = pu.cut_reads(contig, tid, L - 400, L - 100, 5, 100, {L - 150: ("X", 1, 0)}) + [pu.rec(tid, L - 3, "3M", seq="NNN")] * 4
    p = make(io, recs, (tid, 0, L), refs)
    want = pu.planes(recs, (tid, 0, L), refs)
    exp = pu.sites(want, 0, contig, 1, 2, 1, 2)
    assert p.sites(ref, tid, 1, 2, 1, 2) == exp and [s[0] for s in exp][-3:] == [L - 3, L - 2, L - 1] and L % 4 != 0 and (L - 150) in [s[0] for s in exp]
    p.close()
    ref.close()


def test_sites_with_lower_case_and_n_reference_bytes(io, tmp_path):
    rng = random.Random(3)
    seq = [rng.choice("ACGT") for _ in range(401)]
    for i in range(100, 160):
        seq[i] = seq[i].lower()
    for i in range(200, 210):
        seq[i] = "N"
    seq[220], seq[221] = "n", "R"
    text = "".join(seq)
    fa = tmp_path / "small.fa"
    fa.write_text(">x some words\n" + "\n".join(text[i:i + 60] for i in range(0, len(text), 60)) + "\n")
    contig = text.encode()
    refs = [("x", 401)]
    recs = pu.cut_reads(contig, 0, 0, 330, 3, 70, {120: ("X", 1, 0), 130: ("I", 1, 2), 205: ("X", 1, 0), 300: ("D", 1, 2)})
    ref = io.refio.Ref(fa)
    for window in ((0, 0, 401), (0, 97, 303)):
        want = pu.planes(recs, window, refs)
        p = make(io, recs, window, refs)
        same(p, want)
        for q in PARAMS[:2] + [(5, 5, 1, 1), (3, 1, 1, 2)]:
            exp = pu.sites(want, pu.window_of(window, refs)[1], contig, *q)
            assert p.sites(ref, 0, *q) == exp
            p.sites_tsv(tmp_path / "x.tsv")
            assert (tmp_path / "x.tsv").read_bytes() == pu.tsv(exp, "x")
        exp = pu.sites(want, pu.window_of(window, refs)[1], contig, *PARAMS[0])
        by = {s[0]: s for s in exp}
        assert by[120][1] == ord(text[120].upper()) and 110 not in by and 130 in by and 300 in by and 301 in by          # lower case is compared without its case, printed in upper case
        assert not any(200 <= x < 210 or x in (220, 221) for x in by)                                                     # no alt where the reference says N or R
        p.close()
    ref.close()


# ---------------------------------------------------------------- batches that come from the readers
def drain(io, rd, p, max_bytes):
    n_batches = n = 0
    while True:
        recs, b = rd.next(max_bytes)
        if not b.n_records:
            return n_batches, n
        p.add_device(b.d_stream, b.n_bytes, b.d_rec_off, b.n_records)
        n_batches += 1
        n += b.n_records


@pytest.fixture(scope="module")
def sorted_bam(io, tmp_path_factory):
    key = lambda r: (pu.parse(r)[0] & 0xffffffff, pu.parse(r)[1])
    placed = lambda r: 0 <= pu.parse(r)[0] < 4 and 0 <= pu.parse(r)[1] < pu.REFS[pu.parse(r)[0]][1]
    recs = sorted((r for r in ALL + pu.random_records(2500, seed=8) if placed(r) or pu.parse(r)[0] < 0), key=key)          # the unplaced ones sort last
    p = tmp_path_factory.mktemp("pilebam") / "sorted.bam"
    p.write_bytes(bu.bam_bytes(pu.TEXT, pu.REFS, recs, member_size=4000))
    io.bamio.index_build(p)
    return p, recs


def test_through_the_bam_reader(io, sorted_bam):
    path, recs = sorted_bam
    rd = io.bamio.Reader(path)
    p = io.pileio.Pile(pu.REFS, pu.WHOLE)
    n_batches, n = drain(io, rd, p, 8000)
    assert n_batches >= 3 and n == len(recs)
    same(p, pu.planes(recs))
    p.close()
    # a mapq filter attached to the reader: the batches hold the kept records only
    flt = io.filterio.Filter([dict(rules=[dict(mapq=(30, 255, False))])])
    flt.attach(rd)
    rd.rewind()
    p = io.pileio.Pile(pu.REFS, pu.WHOLE)
    n_batches, n = drain(io, rd, p, 8000)
    kept = [r for r in recs if pu.parse(r)[2] >= 30]
    assert n_batches >= 3 and n == len(kept) < len(recs)
    same(p, pu.planes(kept))
    p.close()
    io.filterio.Filter.detach(rd)
    # two regions: a record is served, and counted, once per region it overlaps
    rd.index_load()
    regions = [(2, 1000, 2000), (2, 1990, 2600)]
    rd.set_regions(regions)
    p = io.pileio.Pile(pu.REFS, pu.WHOLE)
    p.set("exclude_flags", 0)
    n_batches, n = drain(io, rd, p, 8000)

    def served(r, reg):
        tid, pos, _, flag, ops = pu.parse(r)[:5]
        reflen = sum(ln for op, ln in ops if op in (0, 2, 3, 7, 8))
        return tid == reg[0] and pos < reg[2] and pos + (1 if reflen == 0 or flag & 4 else reflen) > reg[1]
    per = [[r for r in recs if served(r, reg)] for reg in regions]
    both = [r for r in per[0] if r in per[1]]
    assert n == len(per[0]) + len(per[1]) and len(both) > 3
    same(p, pu.planes(per[0] + per[1], exclude_flags=0))
    p.close()
    rd.close()


def test_through_the_sam_reader(io, tmp_path):
    from tests import sam_util as su
    recs = [r for r in bu.sample_records(400) if len(r) < 2000]
    path = tmp_path / "in.sam"
    path.write_bytes(su.sam_text(bu.TEXT, [su.record_to_line(r, bu.REFS) for r in recs]))
    rd = io.samio.Reader(path)
    window = (0, 0, bu.REFS[0][1])
    p = io.pileio.Pile(bu.REFS, window)
    p.set("min_baseq", 20)
    n_batches, n = drain(io, rd, p, 64 << 20)
    assert n == len(recs)
    want = pu.planes(recs, window, bu.REFS, min_baseq=20)
    same(p, want)
    assert want.sum() > 100
    rd.close()
    p.close()


def test_a_record_batch_of_the_builder(io, sl):
    idx = sl.BWAIndex()
    idx.LoadIndex(os.path.join(GOLDEN, "tiny.fa"))
    al = sl.BWAAligner(idx)
    L = open(os.path.join(GOLDEN, "sim1_bcr.head3000.fq")).read().split("\n")[:4 * 500]
    names, seqs = [L[i][1:].split()[0].encode() for i in range(0, len(L), 4)], [L[i + 1].encode() for i in range(0, len(L), 4)]
    rb = io.recio.Builder(al._handle())
    d_bases, d_offs, d_names, d_name_offs = rb.upload(seqs, names)
    hits = al.align_device(d_bases, d_offs, len(seqs), 0, False, 0.9, 10)
    b = rb.build(hits, d_bases, d_offs, d_names, d_name_offs, False)
    refs = [(n, len(s)) for n, s in pu.fasta_contigs(os.path.join(GOLDEN, "tiny.fa"))]
    window = (0, 0, refs[0][1])
    p = io.pileio.Pile(refs, window)
    p.set("min_baseq", 30)          # the builder writes no qualities (0xff then zeros): every base passes
    p.add_device(b.d_stream, b.n_bytes, b.d_rec_off, b.n_records)
    stream, off = rb.to_host(b)
    recs = [stream[off[i]:off[i + 1]] for i in range(b.n_records)]
    want = pu.planes(recs, window, refs, min_baseq=30)
    same(p, want)
    # (the reads of this file that land on the window's contig: two thirds of them)
    assert b.n_records >= 500 and p.counter("records_counted") == sum(pu.eligible(r, 0) for r in recs) > 300 and want.sum() > 30000 and not want[pu.LOWQ].any()
    p.close()
    rb.close()
