"""The interval unit on the GPU, exact equality everywhere against the brute-force rules of tests/grc_util.py: the device build against the host build, the batch
joins under every knob (pairs, clipped intervals, counts, widths, the two fill forms asserted by their counters), counts-only, merge, records as queries (per-record
counts and pairs, the read filter's region verdict, per-subject counts for any batch split, a broken record, batches from BamReader with and without regions and
from the record builder), and the C++ class's collection join against its single-query host path."""
import ctypes as C
import os
import subprocess

import pytest

from tests import bam_util as bu
from tests import cov_util as cu
from tests import grc_util as gu

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")
WAVE_RANGES = (64, 0, 1 << 20)


class Hip:
    """the HIP runtime the library runs on, for device buffers of the tests' own"""

    def __init__(self):
        paths = sorted({ln.split()[-1] for ln in open("/proc/self/maps") if "libamdhip64" in ln}, key=lambda x: "torch" in x)
        assert paths, "no HIP runtime mapped"
        self.l = C.CDLL(paths[0])
        self.l.hipMalloc.argtypes = [C.POINTER(C.c_void_p), C.c_size_t]
        self.l.hipMemcpy.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int]
        self.l.hipFree.argtypes = [C.c_void_p]

    def up(self, data):
        p = C.c_void_p()
        assert self.l.hipMalloc(C.byref(p), max(len(data), 1)) == 0
        assert self.l.hipMemcpy(p, bytes(data), len(data), 1) == 0
        return p.value

    def down(self, p, n):
        buf = C.create_string_buffer(max(n, 1))
        assert self.l.hipMemcpy(buf, p, n, 2) == 0
        return buf.raw[:n]

    def free(self, p):
        self.l.hipFree(p)


@pytest.fixture(scope="module")
def io(sl):
    from seqlib_amd import _ffi, bamio, filterio, grcio, recio
    grcio.lib()

    class F:
        pass
    f = F()
    f.ffi, f.bamio, f.filterio, f.grcio, f.recio = _ffi, bamio, filterio, grcio, recio
    return f


@pytest.fixture(scope="module")
def want():
    """the brute-force join of every case in both strand modes, computed once"""
    return {(name, ig): gu.join(s, q, ig) for name, s, q in gu.CASES for ig in (True, False)}


@pytest.mark.parametrize("name,subjects,queries", gu.CASES, ids=gu.CASE_IDS)
def test_device_build_equals_host_build_and_python(io, name, subjects, queries):
    c, h = io.grcio.Collection(subjects), io.grcio.Collection(subjects, device=io.grcio.SLX_GRC_HOST)
    assert c.counter("device") >= 0 and h.counter("device") == -1
    assert c.sorted() == h.sorted() == gu.sorted_index(subjects)          # the mirror of the arrays made in HBM and the host build's, array by array
    assert h.merged() == c.merged()
    h.close()
    m = gu.merge(subjects)
    assert c.merged() == m and c.counter("merged") == len(m)
    c.close()
    c = io.grcio.Collection(m)
    assert c.merged() == m          # merging a merged collection changes nothing
    c.close()


@pytest.mark.parametrize("name,subjects,queries", gu.CASES, ids=gu.CASE_IDS)
def test_join_under_every_knob(io, want, name, subjects, queries):
    c = io.grcio.Collection(subjects)
    idx = c.sorted()
    for ignore_strand in (True, False):
        pairs, counts, widths = want[(name, ignore_strand)]
        n_hit = sum(1 for k in counts if k)
        for wave_range in WAVE_RANGES:
            for slice_queries in (1 << 20, 64):
                c.set("wave_range", wave_range); c.set("slice_queries", slice_queries)
                r = c.overlaps(queries, ignore_strand)
                key = (ignore_strand, wave_range, slice_queries)
                assert r["pairs"] == pairs, key
                assert r["count"] == counts and r["width"] == widths and r["n_pairs"] == len(pairs), key
                assert r["offset"] == [sum(counts[:i]) for i in range(len(counts) + 1)], key
                lane, wave = c.counter("queries_lane"), c.counter("queries_wave")
                assert lane + wave == n_hit and c.counter("pairs") == len(pairs), key
                if wave_range == 0:
                    assert lane == 0
                if wave_range == 1 << 20:
                    assert wave == 0
                if wave_range == 64:          # the wave takes exactly the queries with a hit whose candidate range is longer than 64
                    assert wave == sum(1 for q, k in zip(queries, counts) if k and cand_len(idx, q) > 64), key
        for contained in (False, True):
            assert c.count(queries, ignore_strand, contained) == ([len(gu.hits(subjects, q, ignore_strand, True)) for q in queries] if contained else counts)
    c.close()


def cand_len(idx, q):
    """the candidate range by its definition: from the first entry of the chr whose running maximum reaches q.pos1 to the last with pos1 <= q.pos2"""
    srt, _perm, run, _ends = idx
    on = [i for i, s in enumerate(srt) if s[0] == q[0]]
    hi = [i for i in on if srt[i][1] <= q[2]]
    lo = [i for i in on if run[i] >= q[1]]
    return max(0, (hi[-1] + 1 if hi else 0) - lo[0]) if lo else 0


def test_both_fill_forms_run_and_two_ballot_steps(io, want):
    _, s, q = gu.case("container_200")
    c = io.grcio.Collection(s)
    r = c.overlaps(q, True)
    assert c.counter("queries_wave") >= 4 and c.counter("queries_lane") == 0 and max(r["count"]) == 202          # every candidate range starts at the container
    assert r["pairs"] == want[("container_200", True)][0]
    c.close()
    _, s, q = gu.case("queries_1000")
    c = io.grcio.Collection(s)
    c.overlaps(q, True)
    assert c.counter("queries_lane") > 100 and c.counter("queries_wave") > 20
    c.close()


def test_errors(io):
    c = io.grcio.Collection([(0, 1, 5)])
    with pytest.raises(io.ffi.SlxError) as e:
        c.overlaps([(0, 1, 2), (0, 3, 2)])
    assert e.value.code == io.ffi.SLX_EINVAL
    with pytest.raises(io.ffi.SlxError) as e:
        c.count([(0, 3, 2)])
    assert e.value.code == io.ffi.SLX_EINVAL
    assert c.overlaps([(0, 5, 9)])["pairs"] == [(0, 0, 5, 5)]
    c.close()


# ---------------------------------------------------------------- records
RECS = gu.case_records() + cu.random_records(300, seed=11)


def want_records(subjects, recs):
    q = [gu.record_iv(r) for r in recs]
    return gu.join(subjects, q, True)


def test_records_equal_python_and_the_read_filter(io):
    subjects = gu.REC_SUBJECTS
    pairs, counts, widths = want_records(subjects, RECS)
    assert sum(1 for k in counts if k) > 50 and sum(1 for k in counts if not k) > 20
    stream, off = cu.stream_of(RECS)
    hip = Hip()
    d_stream, d_off, d_keep = hip.up(stream), hip.up(b"".join(x.to_bytes(8, "little") for x in off)), hip.up(bytes(len(RECS)))
    flt = io.filterio.Filter([dict(regions=subjects)])
    flt.apply_device(d_stream, d_off, len(RECS), d_keep)
    keep = list(hip.down(d_keep, len(RECS)))
    for long_cigar in (64, 1, 1 << 20):
        for wave_range in WAVE_RANGES:
            c = io.grcio.Collection(subjects)
            c.set("long_cigar", long_cigar); c.set("wave_range", wave_range)
            r = c.overlaps_host(stream, off)
            assert r["pairs"] == pairs and r["count"] == counts and r["width"] == widths
            assert c.counter("long_records") == sum(1 for x in RECS if len(cu.parse(x)[4]) > long_cigar) and c.counter("records") == len(RECS)
            r = c.overlaps_device(d_stream, len(stream), d_off, len(RECS), want_pairs=False)
            assert r["count"] == counts and r["n_pairs"] == len(pairs)
            assert [1 if k else 0 for k in r["count"]] == keep          # the read filter's region test, record by record
            assert c.subject_counts() == [2 * x for x in gu.subject_counts(subjects, RECS)]
            c.close()
    for p in (d_stream, d_off, d_keep):
        hip.free(p)


@pytest.mark.parametrize("pieces", [1, 2, 7])
def test_subject_counts_for_any_batch_split(io, pieces):
    subjects = gu.REC_SUBJECTS + gu.random_subjects(65, 5)
    c = io.grcio.Collection(subjects)
    step = -(-len(RECS) // pieces)
    for i in range(0, len(RECS), step):
        c.overlaps_host(*cu.stream_of(RECS[i:i + step]), want_result=False)
    want = gu.subject_counts(subjects, RECS)
    assert c.subject_counts() == want and sum(want) > 100
    c.clear_counts()
    assert c.subject_counts() == [0] * len(subjects)
    c.overlaps_host(*cu.stream_of(RECS[:50]), want_pairs=False)
    assert c.subject_counts() == gu.subject_counts(subjects, RECS[:50])
    c.close()


def test_a_broken_record_fails_the_call(io):
    good = RECS[:10]
    bad = bytearray(good[3])
    bad[16:18] = b"\xff\xff"          # n_cigar passes block_size
    c = io.grcio.Collection(gu.REC_SUBJECTS)
    with pytest.raises(io.ffi.SlxError, match="record 3 of the batch") as e:
        c.overlaps_host(*cu.stream_of(good[:3] + [bytes(bad)] + good[3:]))
    assert e.value.code == io.ffi.SLX_EIO
    stream, off = cu.stream_of(good)
    for bad_off in (off[:-1] + [off[-1] + 4], [0, off[2], off[1]] + off[3:]):          # an offset past the stream; offsets that run backwards
        with pytest.raises(io.ffi.SlxError, match="of the batch") as e:
            c.overlaps_host(stream, bad_off)
        assert e.value.code == io.ffi.SLX_EIO
    assert c.overlaps_host(stream, off)["count"] == want_records(gu.REC_SUBJECTS, good)[1]
    c.close()


def test_batches_straight_from_the_bam_reader(io, tmp_path):
    key = lambda r: (cu.parse(r)[0] & 0xffffffff, cu.parse(r)[1])
    placed = lambda r: 0 <= cu.parse(r)[0] < 4 and 0 <= cu.parse(r)[1] < cu.REFS[cu.parse(r)[0]][1]
    recs = sorted((r for r in RECS + cu.random_records(1500, seed=8) if placed(r) or cu.parse(r)[0] < 0), key=key)
    p = tmp_path / "sorted.bam"
    p.write_bytes(bu.bam_bytes(cu.TEXT, cu.REFS, recs, member_size=4000))
    io.bamio.index_build(p)
    subjects = gu.REC_SUBJECTS + [(2, 1000, 2000), (2, 1990, 2600), (3, 5000, 900000)]
    rd = io.bamio.Reader(p)
    for regions in (None, [(2, 1000, 2000), (2, 1990, 2600)]):
        if regions:
            rd.index_load()
            rd.set_regions(regions)
        c = io.grcio.Collection(subjects)
        got, served, n_batches = [], [], 0
        while True:
            raws, b = rd.next(8000)
            if not b.n_records:
                break
            r = c.overlaps_device(b.d_stream, b.n_bytes, b.d_rec_off, b.n_records)
            got += [(q + len(served), s, a, e) for q, s, a, e in r["pairs"]]
            served += raws
            n_batches += 1
        assert n_batches >= 3 and (len(served) == len(recs) if not regions else 0 < len(served) < len(recs))
        assert got == want_records(subjects, served)[0] and len(got) > 100
        assert c.subject_counts() == gu.subject_counts(subjects, served)
        c.close()
    rd.close()


def test_a_record_batch_of_the_builder(io, sl):
    idx = sl.BWAIndex()
    idx.LoadIndex(os.path.join(GOLDEN, "tiny.fa"))
    al = sl.BWAAligner(idx)
    L = open(os.path.join(GOLDEN, "sim1_bcr.head3000.fq")).read().split("\n")[:4 * 300]
    names, seqs = [L[i][1:].split()[0].encode() for i in range(0, len(L), 4)], [L[i + 1].encode() for i in range(0, len(L), 4)]
    rb = io.recio.Builder(al._handle())
    d_bases, d_offs, d_names, d_name_offs = rb.upload(seqs, names)
    hits = al.align_device(d_bases, d_offs, len(seqs), 0, False, 0.9, 10)
    b = rb.build(hits, d_bases, d_offs, d_names, d_name_offs, False)
    stream, off = rb.to_host(b)
    recs = [stream[off[i]:off[i + 1]] for i in range(b.n_records)]
    ivs = [gu.record_iv(r) for r in recs if cu.parse(r)[0] >= 0]
    subjects = [(t, p - p % 5000, p - p % 5000 + 4999) for t, p, _ in ivs[::7]] + [(t, p + 20, p + 30) for t, p, _ in ivs[::11]]
    c = io.grcio.Collection(subjects)
    r = c.overlaps_device(b.d_stream, b.n_bytes, b.d_rec_off, b.n_records)
    pairs, counts, widths = want_records(subjects, recs)
    assert r["pairs"] == pairs and r["count"] == counts and r["width"] == widths and len(pairs) > 300
    assert c.subject_counts() == gu.subject_counts(subjects, recs)
    c.close()
    rb.close()


# ---------------------------------------------------------------- the C++ class
def test_cpp_class_join_equals_its_single_query_path(tmp_path):
    """tests/cpp/grc_api_test.cpp gpu: FindOverlaps(subject, query_id, subject_id) and Intersection against FindOverlaps(gr) looped over the same queries -- two
    routes through the same rules --, the reference's interval_queries shape (a merged collection's self-join returns size() hits of equal TotalWidth), and
    OverlapReads / CountReads over a reader's batches"""
    from seqlib_amd import build
    exe = str(tmp_path / "grc_api_test")
    here = os.path.dirname(build.SO)
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-Werror", "-DSEQLIB_GRC_QUERIES", "-I" + os.path.join(ROOT, "include"), os.path.join(ROOT, "tests", "cpp", "grc_api_test.cpp"), "-o", exe,
                           "-L" + here, "-lseqlib_amd", "-Wl,-rpath," + here, "-Wl,-rpath,/opt/rocm/lib", "-lz", "-lpthread"])
    recs = sorted((r for r in RECS if 0 <= cu.parse(r)[0] < 4 and 0 <= cu.parse(r)[1] < cu.REFS[cu.parse(r)[0]][1]), key=lambda r: (cu.parse(r)[0], cu.parse(r)[1]))
    p = tmp_path / "reads.bam"
    p.write_bytes(bu.bam_bytes(cu.TEXT, cu.REFS, recs, member_size=4000))
    want = gu.subject_counts(gu.REC_SUBJECTS, recs)
    subjects = tmp_path / "subjects.txt"
    subjects.write_text("".join("%d %d %d\n" % s[:3] for s in gu.REC_SUBJECTS))
    assert sum(want) > 100
    r = subprocess.run([exe, "gpu", str(p), str(len(recs)), str(subjects), str(sum(want))], capture_output=True, text=True, cwd=str(tmp_path))
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    assert "grc_api_test gpu OK" in r.stdout
