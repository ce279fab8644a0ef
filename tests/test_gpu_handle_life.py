"""What a handle of every unit built on the shared device context (csrc/slx_hip.h SlxGpu) takes, its free gives back: slx_hip_live_bytes, the process-wide tally of the
bytes of HBM and of pinned memory held through the grow-only buffers, is read before a create and after the free, around the smallest batch that makes every buffer of
the unit grow -- and around a second life of the same handle type, which catches state left behind.  A create on a device that is not there (index 99) is SLX_EINVAL
and leaves the tallies alone: the free-on-failure path.  Results are the business of each unit's own tests; here only a plausibility check says the path ran."""
import gc
import os

import pytest

from tests import bam_util as bu
from tests import cov_util as cu
from tests import fastq_util as fu
from tests import grc_util as gu
from tests import sam_util as su
from tests import samw_util as wu

pytestmark = pytest.mark.gpu
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
TINY = os.path.join(GOLDEN, "tiny.fa")
REFS = [("a", 1000), ("b", 1000)]
TEXT = "@HD\tVN:1.6\tSO:unsorted\n" + "".join("@SQ\tSN:%s\tLN:%d\n" % r for r in REFS)


def records():
    """eight records on two 1000-base contigs and two read groups; the third has three CIGAR operations and the last is larger than 64 bytes"""
    out = []
    for i in range(8):
        cigar, seq = ([("M", 4), ("D", 2), ("M", 4)], "ACGTACGT") if i == 2 else ([("M", 60)], "ACGT" * 15) if i == 7 else ([("M", 8)], "ACGTACGT")
        out.append(bu.bam_record("r%d" % i, 0, i % 2, 100 + 50 * i, 60, cigar, seq, bytes([30]) * len(seq), b"NMC\0RGZg%d\0" % (i % 2)))
    return out


RECS = records()
STREAM, OFF = cu.stream_of(RECS)


@pytest.fixture(scope="module")
def io(sl):
    from seqlib_amd import _ffi, bamio, covio, fastqio, grcio, recio, refio, samio, samwio, sortio, statsio
    for m in (bamio, covio, fastqio, grcio, recio, refio, samio, samwio, sortio, statsio):
        m.lib()

    class F:
        pass
    f = F()
    f.ffi, f.bamio, f.covio, f.fastqio, f.grcio, f.recio, f.refio, f.samio, f.samwio, f.sortio, f.statsio = _ffi, bamio, covio, fastqio, grcio, recio, refio, samio, samwio, sortio, statsio
    return f


def tallies(io):
    gc.collect()          # a handle another test dropped goes now, not in the middle of a life
    L = io.ffi.lib()
    return L.slx_hip_live_bytes(0), L.slx_hip_live_bytes(1)


def two_lives(io, life, warm=False):
    """life() creates a handle, uses it and frees it; it returns the tallies it read while the handle lived"""
    if warm:
        life()
    for _ in range(2):
        before = tallies(io)
        held = life()
        assert tallies(io) == before
        assert held[0] > before[0] and held[1] >= before[1], (before, held)          # the handle held HBM while it lived: the tally sees this unit's buffers


def refused(io, create):
    before = tallies(io)
    with pytest.raises(io.ffi.SlxError) as e:
        create()
    assert e.value.code == io.ffi.SLX_EINVAL and "device 99 is not one of the" in str(e.value)
    assert tallies(io) == before


def test_cov(io, tmp_path):
    def life():
        c = io.covio.Coverage(REFS)
        c.set("long_cigar", 2)
        c.add_host(STREAM, OFF)
        assert c.counter("long_records") == 1 and c.depth(0)[100:108].tolist() == [1] * 8
        assert c.regions([(0, 0, 1000)])[0][0] == 8 + 8 + 8 + 8          # records 0, 2, 4, 6 on contig a, the deletion not counted
        c.bedgraph(tmp_path / "a.bedgraph")
        assert (tmp_path / "a.bedgraph").read_bytes().startswith(b"a\t100\t108\t1\n")
        held = tallies(io)
        c.close()
        return held
    two_lives(io, life)
    refused(io, lambda: io.covio.Coverage(REFS, device=99))


def test_stats(io):
    def life():
        s = io.statsio.Stats(long_record=64)
        s.add_host(STREAM, OFF)
        assert s.n_groups() == 2 and s.counter("long_records") >= 1 and s.counter("group_misses") >= 2
        held = tallies(io)
        s.close()
        return held
    two_lives(io, life)
    refused(io, lambda: io.statsio.Stats(device=99))


def test_grc(io):
    subjects = [(0, 90, 120), (0, 100, 400), (0, 395, 500), (1, 0, 1000), (1, 150, 160)]
    queries = [(0, 100, 110), (0, 0, 50), (1, 155, 156), (0, 399, 401)]

    def life():
        g = io.grcio.Collection(subjects)
        assert g.counter("device") >= 0
        assert g.overlaps(queries)["count"] == [len(gu.hits(subjects, q)) for q in queries] and g.counter("pairs") > 0
        g.overlaps_host(STREAM, OFF)
        assert sum(g.subject_counts()) > 0 and len(g.merged()) == 2
        held = tallies(io)
        g.close()
        return held
    two_lives(io, life)
    refused(io, lambda: io.grcio.Collection(subjects, device=99))


def test_samw(io, tmp_path):
    good = [r for _, r, ok in wu.CASES if ok][:24]
    stream, off = wu.stream_of(good)

    def life():
        p = tmp_path / "a.sam"
        w = io.samwio.Writer(p)
        w.header(bu.TEXT, [n for n, _ in bu.REFS])
        w.write_host(stream, off)
        w.set("fast_fail", 1)          # every record through the host formatter: the slow buffers
        w.write_host(stream, off)
        assert w.counter("records") == 48 and w.counter("slow_records") >= 24
        held = tallies(io)
        w.close()
        assert p.read_bytes().count(b"\n") >= 48
        return held
    two_lives(io, life)
    refused(io, lambda: io.samwio.Writer(tmp_path / "b.sam", device=99))
    assert not (tmp_path / "b.sam").exists()


def test_sort(io):
    def life():
        s = io.sortio.Sorter()
        s.add_host(RECS[:5])
        s.add_host(RECS[5:])
        held = tallies(io)
        got, off, perm = s.to_host()
        assert len(got) == len(STREAM) and sorted(perm) == list(range(8))
        s.close()
        return held
    two_lives(io, life)
    refused(io, lambda: io.sortio.Sorter(device=99))


def test_bgzf_and_bam(io, tmp_path):
    raw = bu.bam_header(TEXT, REFS) + STREAM
    p = tmp_path / "a.bam"

    def write():
        w = io.bamio.Writer(p)
        w.write(raw)
        w.flush()
        held = tallies(io)
        w.close()
        return held

    def read():
        rd = io.bamio.Reader(p)
        recs, _ = rd.next()
        assert recs == RECS
        assert rd.reads_device()[2] == 8
        held = tallies(io)
        rd.close()
        return held
    two_lives(io, write)
    two_lives(io, read)
    refused(io, lambda: io.bamio.Writer(tmp_path / "b.bam", device=99))
    refused(io, lambda: io.bamio.Reader(p, device=99))
    assert not (tmp_path / "b.bam").exists()


def test_sam(io, tmp_path):
    p = tmp_path / "a.sam"
    p.write_bytes(su.sam_text(bu.TEXT, su.canonical(8)[0]))

    def life():
        rd = io.samio.Reader(p)
        assert len(rd.next()[0]) == 8
        held = tallies(io)
        rd.close()
        return held
    two_lives(io, life)
    refused(io, lambda: io.samio.Reader(p, device=99))


@pytest.mark.parametrize("source", ["plain", "bgzf"])
def test_fastq(io, tmp_path, source):
    text = b"".join(b"@r%d c\n%s\n+\n%s\n" % (i, b"ACGT" * (2 + i), b"I" * (8 + 4 * i)) for i in range(8))
    p = tmp_path / "a.fq"
    p.write_bytes(fu.bgzf(text) if source == "bgzf" else text)

    def life():
        with io.fastqio.Reader(p) as r:
            b = r.next()
            assert b.n_reads == 8
            return tallies(io)
    two_lives(io, life)
    refused(io, lambda: io.fastqio.Reader(p, device=99))


def test_ref(io):
    def life():
        r = io.refio.Ref(TINY)
        loaded = tallies(io)
        assert r.nseq() == 4 and len(r.fetch_host([(0, 0, 50), (3, 10, 20)])[0]) == 60
        nm, md = r.nm_md_host(STREAM, OFF)
        assert len(nm) == len(md) == 8
        held = tallies(io)
        assert held[0] > loaded[0]
        r.close()
        return held
    two_lives(io, life)
    refused(io, lambda: io.refio.Ref(TINY, device=99))


def test_rec(io, sl, tiny_gpu):
    L = open(os.path.join(GOLDEN, "sim1_bcr.head3000.fq")).read().split("\n")
    names, seqs = [L[i][1:].split()[0].encode() for i in range(0, 32, 4)], [L[i + 1].encode() for i in range(0, 32, 4)]
    aligner = sl.BWAAligner(tiny_gpu)

    def life():
        rb = io.recio.Builder(aligner._handle())
        d_bases, d_offs, d_names, d_name_offs = rb.upload(seqs, names)
        hits = aligner.align_device(d_bases, d_offs, len(seqs), 0)
        b = rb.build(hits, d_bases, d_offs, d_names, d_name_offs)
        assert b.n_records >= 8 and len(rb.to_host(b)[0]) == b.n_bytes
        held = tallies(io)
        rb.close()
        return held
    two_lives(io, life, warm=True)          # (the aligner's own work areas grow in its first call and stay)
