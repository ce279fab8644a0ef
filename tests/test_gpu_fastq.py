"""The FASTQ reader on the GPU (include/seqlib_amd_fastq.h through seqlib_amd/fastqio.py): for every case of the list all eight arrays of every batch, copied
down, equal the Python statement of the grammar (tests/fastq_util.py) byte for byte -- whatever the batch size, the source of the bytes and the knobs -- and
the counters show that the strict files went through the kernels, not through the serial parser."""
import os

import numpy as np
import pytest

from tests import fastq_util

pytestmark = pytest.mark.gpu

TILE = 64
CASES = fastq_util.cases(TILE)
BY = {n: (t, s) for n, t, s in CASES}
SWEEP = (64, 300, 4096, 0)          # smaller than a record (the batch grows), a few records, some tiles, the default


@pytest.fixture(scope="module")
def fq(sl):
    from seqlib_amd import fastqio
    fastqio.lib()
    return fastqio


@pytest.fixture(scope="module")
def expected():
    return {n: fastq_util.parse(t) for n, t, _ in CASES}          # computed once, shared, never changed


def flat(recs):
    """the eight arrays of records as one batch would hold them"""
    cat = lambda i: b"".join(r[i] for r in recs)
    offs = lambda i: np.cumsum([0] + [len(r[i]) for r in recs]).astype(np.uint64)
    return dict(bases=cat(2), quals=cat(3), names=cat(0), coms=cat(1), offs=offs(2), name_offs=offs(0), com_offs=offs(1), flags=bytes(r[4] for r in recs))


def run(fq, path, max_bytes=0, knobs=(), small_tiles=True):
    """-> (reads of all batches, infos, counters); every batch's arrays are also checked against each other"""
    with fq.Reader(path) as r:
        if small_tiles:
            r.set("tile_bytes", TILE)
        for k, v in knobs:
            r.set(k, v)
        reads, info = r.read_all(max_bytes)
        assert r.next(max_bytes) is None          # the end stays the end
        return reads, info, {c: r.counter(c) for c in fq.COUNTERS}


def check_batches(info, recs):
    """all eight arrays of every batch, byte for byte"""
    at = 0
    for b in info:
        e, h = flat(recs[at:at + b["n_reads"]]), b["host"]
        for k in ("bases", "quals", "names", "coms", "flags"):
            assert h[k].tobytes() == e[k], k
        for k in ("offs", "name_offs", "com_offs"):
            assert np.array_equal(h[k], e[k]), k
        at += b["n_reads"]
    assert at == len(recs)


@pytest.mark.parametrize("name", [n for n, _, _ in CASES])
def test_case_matches_the_grammar_for_every_batch_size(fq, expected, tmp_path, name):
    text, strict = BY[name]
    recs, bad = expected[name]
    p = tmp_path / "in.fq"
    p.write_bytes(text)
    for mb in SWEEP:
        reads, info, c = run(fq, p, mb)
        assert reads == recs, "max_bytes %d" % mb
        check_batches(info, recs)
        assert c["reads"] == len(recs) and c["fast_reads"] + c["slow_reads"] == len(recs) and c["source"] == 0
        assert c["bad_tail"] == (1 if bad else 0)
        assert sum(b["n_slow_reads"] for b in info) == c["slow_reads"]
        if not bad:
            assert sum(b["n_text_bytes"] for b in info) <= len(text)
        if strict:          # the kernels did it: the serial parser must not be what makes a broken fast path pass
            assert c["slow_reads"] == 0 and c["fast_reads"] == len(recs), "max_bytes %d" % mb
    if mb == 0 and recs:
        assert len(info) == 1


def test_golden_file_is_parsed_by_the_kernels_alone(fq, golden_dir):
    path = os.path.join(golden_dir, "sim1_bcr.head3000.fq")
    recs, bad = fastq_util.parse(open(path, "rb").read())
    for mb, tiles in ((0, False), (100000, True)):
        reads, info, c = run(fq, path, mb, small_tiles=tiles)
        assert reads == recs and not bad
        check_batches(info, recs)
        assert c["slow_reads"] == 0 and c["fast_reads"] == 3000 and c["reads"] == 3000
        assert c["batches"] == len(info) and (mb == 0) == (len(info) == 1)


@pytest.mark.parametrize("name", ["one_multiline_mid", "one_multiline_mid_crlf"])
def test_fast_path_runs_up_to_the_first_record_that_fails(fq, expected, tmp_path, name):
    p = tmp_path / "in.fq"
    p.write_bytes(BY[name][0])
    reads, info, c = run(fq, p)
    assert reads == expected[name][0]
    assert c["fast_reads"] == fastq_util.ONE_MULTILINE_MID_BEFORE and c["slow_reads"] == len(reads) - c["fast_reads"]


@pytest.mark.parametrize("name", ["strict", "lengths", "names_crlf", "blank_and_junk", "fasta_multi", "long_qual_mid"])
def test_sources_give_identical_batches(fq, expected, tmp_path, name):
    """plain, BGZF (members of 0x1800 bytes: records straddle members) and gzip forms of one text"""
    text, strict = BY[name]
    recs, bad = expected[name]
    forms = {0: text, 1: fastq_util.bgzf(text, 0x1800), 2: fastq_util.gzip_(text)}
    got = {}
    for src, data in forms.items():
        p = tmp_path / ("in%d.fq.gz" % src)
        p.write_bytes(data)
        for mb in (300, 0x1800 + 100, 0):
            reads, info, c = run(fq, p, mb)
            assert c["source"] == src
            assert reads == recs and c["bad_tail"] == (1 if bad else 0)
            check_batches(info, recs)
            if strict:
                assert c["slow_reads"] == 0
            if src != 1:          # BGZF grows a batch by whole members, the others by bytes: the cuts agree for those two
                got.setdefault(mb, []).append([b["n_reads"] for b in info])
    for mb, cuts in got.items():
        assert cuts[0] == cuts[1], mb


def test_empty_bgzf_and_gzip(fq, tmp_path):
    for i, data in enumerate((fastq_util.bgzf(b""), fastq_util.gzip_(b""))):
        p = tmp_path / ("e%d.gz" % i)
        p.write_bytes(data)
        reads, info, c = run(fq, p)
        assert reads == [] and c["source"] == i + 1 and c["reads"] == 0


@pytest.mark.parametrize("name", ["strict", "lengths_crlf", "one_multiline_mid", "truncated_qual"])
def test_fast_fail_knob_gives_the_same_bytes(fq, expected, tmp_path, name):
    p = tmp_path / "in.fq"
    p.write_bytes(BY[name][0])
    for mb in (300, 0):
        reads, info, c = run(fq, p, mb, knobs=(("fast_fail", 1),))
        assert reads == expected[name][0]
        check_batches(info, expected[name][0])
        assert c["fast_reads"] == 0 and c["slow_reads"] == len(reads)


@pytest.mark.parametrize("gather_tile", [16, 48, 4096])
def test_gather_tile_sizes(fq, expected, tmp_path, gather_tile):
    p = tmp_path / "in.fq"
    p.write_bytes(BY["lengths"][0])
    reads, info, c = run(fq, p, knobs=(("gather_tile_bytes", gather_tile),))
    assert reads == expected["lengths"][0] and c["slow_reads"] == 0


def test_rewind_and_knob_ranges(fq, expected, tmp_path):
    from seqlib_amd import _ffi
    p = tmp_path / "in.fq"
    p.write_bytes(BY["truncated_qual"][0])
    with fq.Reader(p) as r:
        for k, v in (("tile_bytes", 24), ("tile_bytes", 0), ("gather_tile_bytes", 8192), ("fast_fail", 2), ("no_such_key", 1)):
            with pytest.raises(_ffi.SlxError):
                r.set(k, v)
        assert r.counter("no_such_counter") == -1
        a, _ = r.read_all(100)
        assert r.counter("bad_tail") == 1 and r.next() is None
        r.rewind()
        assert r.counter("reads") == 0 and r.counter("bad_tail") == 0
        b, _ = r.read_all(0)
        assert a == b == expected["truncated_qual"][0] and r.counter("bad_tail") == 1
    p.write_bytes(BY["strict"][0])
    with fq.Reader(p) as r:
        first = r.next(2000)
        assert first is not None and first.n_reads < 50
        r.rewind()          # in the middle of a pass
        assert r.read_all(0)[0] == expected["strict"][0]
