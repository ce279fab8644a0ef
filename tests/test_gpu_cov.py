"""GPU tests of the coverage unit at the C-ABI (include/seqlib_amd_cov.h through seqlib_amd/covio.py) against the Python statement of the rules in
tests/cov_util.py: every record shape under every mode, both CIGAR kernels, batch shapes with every form of the LDS window, constructed window cases,
accumulation, the window object, region sums, bedGraph text, and batches that come from the BAM reader (whole file, filtered, regions), the SAM reader and the
record builder.  Equality is exact everywhere.  The C++ class is driven in tests/test_cpp_cov.py."""
import os
import random

import numpy as np
import pytest

from tests import bam_util as bu
from tests import cov_util as cu

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")
SMALL = cu.REFS[:3]          # without the 10 Mbp contig: records on it are then outside the header
ALL = [r for _, r in cu.CASES]


@pytest.fixture(scope="module")
def io(sl):
    from seqlib_amd import _ffi, bamio, covio, filterio, recio, samio
    covio.lib()

    class F:
        pass
    f = F()
    f.ffi, f.bamio, f.covio, f.filterio, f.recio, f.samio = _ffi, bamio, covio, filterio, recio, samio
    return f


def make(io, recs, cfg=(cu.ALIGNED, 0, 0), refs=cu.REFS, window=None, knobs=None, pieces=1):
    """a coverage object over refs with the records added through slx_cov_add_host in `pieces` batches"""
    c = io.covio.Coverage(refs, window)
    c.set("mode", cfg[0]); c.set("buff", cfg[1]); c.set("count_del", cfg[2])
    for k, v in (knobs or {}).items():
        c.set(k, v)
    step = max(1, -(-len(recs) // pieces))
    for i in range(0, max(len(recs), 1), step):
        c.add_host(*cu.stream_of(recs[i:i + step]))
    return c


def same(c, want, refs=cu.REFS):
    for t in range(len(refs)):
        got = c.depth(t)
        bad = np.flatnonzero(got != want[t])
        assert not len(bad), (refs[t][0], bad[:5].tolist(), got[bad[:5]].tolist(), want[t][bad[:5]].tolist())


def n_long(recs, refs, threshold, **elig):
    return sum(cu.eligible(r, len(refs), **elig) and len(cu.parse(r)[4]) > threshold for r in recs)


@pytest.mark.parametrize("long_cigar", [64, 1, 1 << 20])
@pytest.mark.parametrize("cfg", cu.CONFIGS, ids=cu.CONFIG_IDS)
def test_every_record_shape_in_every_mode_through_both_kernels(io, cfg, long_cigar):
    c = make(io, ALL, cfg, knobs={"long_cigar": long_cigar})
    same(c, cu.depth(ALL, *cfg))
    n_elig = sum(cu.eligible(r, 4) for r in ALL)
    assert (c.counter("records_seen"), c.counter("records_counted"), c.counter("long_records")) == (len(ALL), n_elig, n_long(ALL, cu.REFS, long_cigar))
    assert n_long(ALL, cu.REFS, 64) == 3 and n_long(ALL, cu.REFS, 1) > 10 and c.counter("nonsense") == -1
    c.close()
    # the other eligibility knobs: no flag excluded, and a mapq floor
    c = make(io, ALL, cfg, knobs={"long_cigar": long_cigar, "exclude_flags": 0, "min_mapq": 4})
    want = cu.depth(ALL, *cfg, exclude_flags=0, min_mapq=4)
    same(c, want)
    assert c.counter("records_counted") == sum(cu.eligible(r, 4, 0, 4) for r in ALL) != n_elig
    assert c.max() == max(int(v.max()) for v in want) and c.max(2) == int(want[2].max()) and c.max(1) == int(want[1].max())
    assert [c.at(2, p) for p in (0, 104, 4999, 5000, -1)] == [int(want[2][0]), int(want[2][104]), int(want[2][4999]), 0, 0] and c.at(9, 0) == 0 and c.at(-1, 0) == 0
    assert c.at(3, 10000000) == int(want[3][-1]) == 1
    p, n = c.depth_device(2)
    assert p and n == 5000
    c.close()


@pytest.mark.parametrize("n", [0, 1, 63, 64, 65, 1024, 1025, 3000])
def test_batch_shapes_and_every_form_of_the_window(io, n):
    recs = cu.random_records(n, seed=n + 1)
    shuffled = list(recs)
    random.Random(5).shuffle(shuffled)
    for cfg in ((cu.ALIGNED, 0, 0), (cu.SPAN, 0, 0)):
        want = cu.depth(recs, *cfg, refs=SMALL)
        for order in (recs, shuffled):
            for lds_window in (0, 64, 8192):
                for slice_records in (64, 1024):
                    c = make(io, order, cfg, refs=SMALL, knobs={"lds_window": lds_window, "slice_records": slice_records})
                    same(c, want, SMALL)
                    ev = c.counter("events_lds") + c.counter("events_global")
                    assert c.counter("records_seen") == n and (lds_window or c.counter("events_lds") == 0)
                    if cfg[0] == cu.SPAN:          # one interval a record, two adds an interval (records that are clipped away give none)
                        assert ev == 2 * sum(cu.eligible(r, 3) and bool(cu.clipped(cu.intervals(r, *cfg), 0, SMALL[cu.parse(r)[0]][1])) for r in recs)
                    c.close()


def test_sorted_input_lands_in_the_lds_window(io):
    recs = [cu.rec(2, 2 * i, "100M") for i in range(2000)]          # 2000 reads over 4 kbp, coordinate-sorted
    c = make(io, recs, refs=SMALL)
    same(c, cu.depth(recs, cu.ALIGNED, refs=SMALL), SMALL)
    assert c.counter("events_lds") == 4000 and c.counter("events_global") == 0
    c.close()


def test_constructed_window_cases(io):
    # +1 inside the window, -1 outside
    recs = [cu.rec(2, 1000, "10M"), cu.rec(2, 1050, "100M")]
    c = make(io, recs, knobs={"lds_window": 64})
    same(c, cu.depth(recs, cu.ALIGNED))
    assert (c.counter("events_lds"), c.counter("events_global")) == (3, 1)
    c.close()
    # an interval that starts in front of the anchor (FULL reaches back over its soft clip)
    recs = [cu.rec(2, 1000, "10M"), cu.rec(2, 1002, "30S10M")]
    c = make(io, recs, (cu.FULL, 0, 0), knobs={"lds_window": 64})
    same(c, cu.depth(recs, cu.FULL))
    assert (c.counter("events_lds"), c.counter("events_global")) == (3, 1)
    c.close()
    # a tid change inside a slice: the window runs on over the next contig's entries
    recs = [cu.rec(0, 0, "1M"), cu.rec(1, 5, "60M"), cu.rec(1, 60, "30M"), cu.rec(2, 0, "10M"), cu.rec(2, 4000, "100M"), cu.rec(3, 7, "5M")]
    c = make(io, recs)
    same(c, cu.depth(recs, cu.ALIGNED))
    assert c.counter("events_lds") == 12 and c.counter("events_global") == 0          # 4 + 72 + 5004 entries in front of contig 3: all inside 8192
    c.close()
    c = make(io, recs, knobs={"lds_window": 128})
    same(c, cu.depth(recs, cu.ALIGNED))
    assert c.counter("events_lds") == 8 and c.counter("events_global") == 4
    c.close()
    # a slice whose first records are not eligible: the anchor is the first eligible one
    recs = [cu.rec(-1, -1, "", flag=4), cu.rec(2, 50, "10M", flag=0x400), cu.rec(2, 3000, "10M"), cu.rec(2, 3005, "10M")]
    c = make(io, recs, knobs={"lds_window": 64})
    same(c, cu.depth(recs, cu.ALIGNED))
    assert (c.counter("events_lds"), c.counter("events_global"), c.counter("records_counted")) == (4, 0, 2)
    c.close()
    # no eligible record at all
    c = make(io, recs[:2])
    same(c, cu.depth([], cu.ALIGNED))
    assert c.counter("records_counted") == 0 and c.max() == 0
    c.close()


def test_1025_records_on_one_position(io, tmp_path):
    recs = [cu.rec(2, 1234, "10M")] * 1025 + [cu.rec(2, 1240, "2M")]
    for lds_window in (0, 8192):
        c = make(io, recs, knobs={"lds_window": lds_window})
        want = cu.depth(recs, cu.ALIGNED)
        same(c, want)
        assert c.max() == c.at(2, 1240) == 1026 and c.at(2, 1234) == 1025
        c.bedgraph(tmp_path / "a.bg")
        assert (tmp_path / "a.bg").read_bytes() == b"c5k\t1234\t1240\t1025\nc5k\t1240\t1242\t1026\nc5k\t1242\t1244\t1025\n" == cu.bedgraph(want, 0)
        assert c.regions([(2, 0, 5000), (2, 1239, 1243)], 1025) == ([1025 * 10 + 2, 1025 * 4 + 2], [10, 4]) == cu.region_sums(want, [(2, 0, 5000), (2, 1239, 1243)], 1025)
        assert c.regions([(2, 0, 5000)], 1026) == ([1025 * 10 + 2], [2])
        c.close()


@pytest.mark.parametrize("cfg", [cu.CONFIGS[0], cu.CONFIGS[4]], ids=["span", "aligned"])
def test_accumulation(io, cfg):
    recs = ALL + cu.random_records(600, seed=3)
    want = cu.depth(recs, *cfg)
    one = make(io, recs, cfg)
    same(one, want)
    three = make(io, recs, cfg, pieces=3)
    same(three, want)
    # add, read, add again, read again: the settled array is turned back into differences
    c = make(io, recs[:200], cfg)
    same(c, cu.depth(recs[:200], *cfg))
    c.add_host(*cu.stream_of(recs[200:450]))
    assert c.at(2, 104) == int(cu.depth(recs[:450], *cfg)[2][104])
    c.add_host(*cu.stream_of(recs[450:]))
    c.add_host(b"", [0])
    same(c, want)
    c.clear()
    same(c, cu.depth([], *cfg))
    assert c.max() == 0
    c.add_host(*cu.stream_of(recs))          # and it is usable afterwards
    same(c, want)
    # the scan in chunks of 64 entries: the carry crosses every chunk and every contig border
    s = make(io, recs, cfg, refs=SMALL, knobs={"scan_chunk": 64})
    same(s, cu.depth(recs, *cfg, refs=SMALL), SMALL)
    s.add_host(*cu.stream_of(recs[:10]))
    same(s, cu.depth(recs + recs[:10], *cfg, refs=SMALL), SMALL)
    assert s.max() == max(int(v.max()) for v in cu.depth(recs + recs[:10], *cfg, refs=SMALL))
    for x in (one, three, c, s):
        x.close()
    with pytest.raises(io.ffi.SlxError) as e:
        make(io, [], knobs={"scan_chunk": 66})
    assert e.value.code == io.ffi.SLX_EINVAL


def test_a_broken_record_fails_the_call(io):
    good = ALL[:10]
    bad = bytearray(good[3])
    bad[16:18] = b"\xff\xff"          # n_cigar passes block_size
    c = io.covio.Coverage(cu.REFS)
    with pytest.raises(io.ffi.SlxError, match="record 3 of the batch") as e:
        c.add_host(*cu.stream_of(good[:3] + [bytes(bad)] + good[3:]))
    assert e.value.code == io.ffi.SLX_EIO
    stream, off = cu.stream_of(good)
    for bad_off in (off[:-1] + [off[-1] + 4], [0, off[2], off[1]] + off[3:]):          # an offset past the stream; offsets that run backwards
        with pytest.raises(io.ffi.SlxError, match="of the batch") as e:
            c.add_host(stream, bad_off)
        assert e.value.code == io.ffi.SLX_EIO
    c.clear()
    c.add_host(stream, off)
    same(c, cu.depth(good, cu.ALIGNED))
    c.close()


@pytest.mark.parametrize("cfg", cu.CONFIGS, ids=cu.CONFIG_IDS)
def test_window_object_equals_the_slice(io, cfg):
    recs = ALL + [cu.rec(2, 90, "20M"), cu.rec(2, 290, "20M"), cu.rec(2, 95, "300M"), cu.rec(2, 299, "1M"), cu.rec(2, 300, "5M"), cu.rec(2, 94, "5M")] + cu.random_records(300, seed=4, span=600)
    whole = make(io, recs, cfg)
    w = make(io, recs, cfg, window=(2, 100, 300))
    want = cu.depth(recs, *cfg)
    same(whole, want)
    assert np.array_equal(w.depth(2, 100, 300), want[2][100:300]) and np.array_equal(w.depth(2, 100, 300), whole.depth(2, 100, 300))
    got = w.depth(2)
    assert not got[:100].any() and not got[300:].any() and np.array_equal(got[100:300], want[2][100:300]) and got[100:300].any()
    assert not w.depth(1).any() and not w.depth(3, 9999000, 10000001).any() and w.max() == int(want[2][100:300].max()) == w.max(2) and w.max(1) == 0
    assert w.depth_device(2)[1] == 200 and w.depth_device(1)[1] == 0
    assert w.regions([(2, 0, 5000), (2, 150, 160), (1, 0, 70)], 1) == cu.region_sums([want[0][:0], want[1][:0], want[2][100:300]], [(2, 0, 200), (2, 50, 60), (1, 0, 70)], 1)
    ww = cu.depth(recs, *cfg, window=(2, 100, 300))
    assert np.array_equal(ww[2], got)
    for x in (whole, w):
        x.close()
    # a window clipped to its contig
    w = make(io, recs, cfg, window=(2, 4900, 6000))
    assert np.array_equal(w.depth(2, 4900, 5000), want[2][4900:]) and w.depth_device(2)[1] == 100
    w.close()


def test_regions(io):
    recs = ALL + cu.random_records(1500, seed=6) + [cu.rec(2, 1234, "10M")] * 1025 + [cu.rec(3, 100 + 7 * i, "150M") for i in range(2000)] + [cu.rec(3, 5000000, "2000000M")]
    c = make(io, recs)
    want = cu.depth(recs, cu.ALIGNED)
    regs = [(2, 100, 101), (2, 100, 163), (2, 101, 165), (2, 3, 68), (2, 7, 4104), (3, 1, 4098), (2, 0, 5000), (1, 0, 70), (0, 0, 1), (3, 0, 10000001), (2, -50, 6000), (3, 9999990, 1 << 40),
            (2, 700, 700), (2, 5000, 5000), (2, 6000, 7000), (3, 4999999, 7000003), (1, 69, 70)]
    for min_depth in (1, 2, 1025):
        assert c.regions(regs, min_depth) == cu.region_sums(want, regs, min_depth)
    s, n = c.regions(regs, 1025)
    assert s[12] == n[12] == 0 and n[6] == 10 and s[9] > 2000000 and c.regions([], 1) == ([], [])
    with pytest.raises(io.ffi.SlxError) as e:
        c.regions([(4, 0, 5)])
    assert e.value.code == io.ffi.SLX_EINVAL
    c.close()


@pytest.mark.parametrize("scan_chunk", [1 << 30, 64])
def test_bedgraph(io, tmp_path, scan_chunk):
    """scan_chunk 64 (on the contigs below the big one): the text is made 64 entries at a time, runs cross the pieces"""
    refs = cu.REFS if scan_chunk == 1 << 30 else SMALL
    recs = [r for r in ALL if cu.parse(r)[0] != 1]          # contig c70 stays all zero; c5k has a run that ends at the contig's end; big has 8-digit positions
    for cfg in (cu.CONFIGS[0], cu.CONFIGS[4]):
        c = make(io, recs, cfg, refs=refs, knobs={"scan_chunk": scan_chunk})
        want = cu.depth(recs, *cfg, refs=refs)
        assert not want[1].any() and want[2][-1] > 0 and (len(refs) == 3 or want[3][-1] > 0)
        for iz in (0, 1):
            c.bedgraph(tmp_path / "all.bg", include_zero=iz)
            text = (tmp_path / "all.bg").read_bytes()
            assert text == cu.bedgraph(want, iz, refs=refs)
            assert c.counter("runs") == text.count(b"\n") > 20
            assert (b"c70\t0\t70\t0\n" in text) == bool(iz) and (len(refs) == 3 or b"\t10000001\t" in text) and b"c5k\t4999\t5000\t" in text
            for tid in range(len(refs)):
                c.bedgraph(tmp_path / "one.bg", tid=tid, include_zero=iz)
                assert (tmp_path / "one.bg").read_bytes() == cu.bedgraph(want, iz, [tid], refs=refs)
        c.close()
    # a window object prints absolute positions
    w = make(io, recs, refs=refs, window=(2, 100, 300), knobs={"scan_chunk": scan_chunk})
    w.bedgraph(tmp_path / "w.bg", include_zero=1)
    d = cu.depth(recs, cu.ALIGNED, refs=refs)
    assert (tmp_path / "w.bg").read_bytes() == cu.bedgraph([d[t][100:300] if t == 2 else d[t][:0] for t in range(len(refs))], 1, refs=refs, first=100)
    w.close()
    with pytest.raises(io.ffi.SlxError) as e:
        make(io, recs).bedgraph(tmp_path / "no_such_dir" / "x.bg")
    assert e.value.code == io.ffi.SLX_EIO


# ---------------------------------------------------------------- batches that come from the readers
def drain(io, rd, c, max_bytes):
    n_batches = n = 0
    while True:
        recs, b = rd.next(max_bytes)
        if not b.n_records:
            return n_batches, n
        c.add_device(b.d_stream, b.n_bytes, b.d_rec_off, b.n_records)
        n_batches += 1
        n += b.n_records


@pytest.fixture(scope="module")
def sorted_bam(io, tmp_path_factory):
    key = lambda r: (cu.parse(r)[0] & 0xffffffff, cu.parse(r)[1])
    placed = lambda r: 0 <= cu.parse(r)[0] < 4 and 0 <= cu.parse(r)[1] < cu.REFS[cu.parse(r)[0]][1]
    recs = sorted((r for r in ALL + cu.random_records(2500, seed=8) if placed(r) or cu.parse(r)[0] < 0), key=key)          # the unplaced ones sort last
    p = tmp_path_factory.mktemp("covbam") / "sorted.bam"
    p.write_bytes(bu.bam_bytes(cu.TEXT, cu.REFS, recs, member_size=4000))
    io.bamio.index_build(p)
    return p, recs


def test_through_the_bam_reader(io, sorted_bam):
    p, recs = sorted_bam
    for cfg in (cu.CONFIGS[4], cu.CONFIGS[0]):
        rd = io.bamio.Reader(p)
        c = make(io, [], cfg)
        n_batches, n = drain(io, rd, c, 8000)
        assert n_batches >= 3 and n == len(recs)
        same(c, cu.depth(recs, *cfg))
        c.close()
        # a mapq filter attached to the reader: the batches hold the kept records only
        flt = io.filterio.Filter([dict(rules=[dict(mapq=(30, 255, False))])])
        flt.attach(rd)
        rd.rewind()
        c = make(io, [], cfg)
        n_batches, n = drain(io, rd, c, 8000)
        kept = [r for r in recs if flt.test_record(r)]
        assert kept == [r for r in recs if cu.parse(r)[2] >= 30]
        assert n_batches >= 3 and n == len(kept) < len(recs)
        same(c, cu.depth(kept, *cfg))
        c.close()
        io.filterio.Filter.detach(rd)
        # two regions: a record is served, and counted, once per region it overlaps
        rd.index_load()
        regions = [(2, 1000, 2000), (2, 1990, 2600)]
        rd.set_regions(regions)
        c = make(io, [], cfg, knobs={"exclude_flags": 0})
        n_batches, n = drain(io, rd, c, 8000)

        def served(r, reg):
            tid, pos, _, flag, ops = cu.parse(r)
            reflen = sum(ln for op, ln in ops if op in cu.REF_OPS)
            return tid == reg[0] and pos < reg[2] and pos + (1 if reflen == 0 or flag & 4 else reflen) > reg[1]
        per = [[r for r in recs if served(r, reg)] for reg in regions]
        both = [r for r in per[0] if r in per[1]]
        assert n == len(per[0]) + len(per[1]) and len(both) > 3
        same(c, cu.depth(per[0] + per[1], *cfg, exclude_flags=0))
        c.close()
        rd.close()


def test_through_the_sam_reader(io, tmp_path):
    from tests import sam_util as su
    recs = [r for r in bu.sample_records(400) if len(r) < 2000]
    p = tmp_path / "in.sam"
    p.write_bytes(su.sam_text(bu.TEXT, [su.record_to_line(r, bu.REFS) for r in recs]))
    rd = io.samio.Reader(p)
    c = io.covio.Coverage(bu.REFS)
    n_batches, n = drain(io, rd, c, 64 << 20)
    assert n == len(recs)
    same(c, cu.depth(recs, cu.ALIGNED, refs=bu.REFS), bu.REFS)
    assert c.max() > 1
    rd.close()
    c.close()


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
    refs = []
    for ln in open(os.path.join(GOLDEN, "tiny.fa")):
        if ln.startswith(">"):
            refs.append([ln[1:].split()[0], 0])
        else:
            refs[-1][1] += len(ln.strip())
    refs = [tuple(r) for r in refs]
    for cfg in (cu.CONFIGS[4], cu.CONFIGS[3]):
        c = io.covio.Coverage(refs)
        c.set("mode", cfg[0])
        c.add_device(b.d_stream, b.n_bytes, b.d_rec_off, b.n_records)
        stream, off = rb.to_host(b)
        recs = [stream[off[i]:off[i + 1]] for i in range(b.n_records)]
        want = cu.depth(recs, *cfg, refs=refs)
        same(c, want, refs)
        assert b.n_records >= 500 and c.counter("records_counted") > 400 and c.max() > 5
        c.close()
    rb.close()
