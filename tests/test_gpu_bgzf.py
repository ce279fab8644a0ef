"""GPU tests of the BGZF writer at the C-ABI (slx_bgzf_* of include/seqlib_amd_bam.h through seqlib_amd/bamio.Writer).  The independent statement is Python's
zlib through tests/bam_util.scan_members / inflate_all (ISIZE and CRC32 asserted per member); the payloads are tests/bgzf_payloads.py's.  The C++ class is
driven in tests/test_cpp_bamwriter_gpu.py.  A write to a closed handle is not tested: slx_bgzf_close frees the handle, there is nothing left to write to."""
import random

import pytest

from tests import bai_util as ba
from tests import bam_util as bu
from tests import bgzf_payloads as bp

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def bamio(sl):
    from seqlib_amd import bamio as b
    b.lib()
    return b


@pytest.fixture(scope="module")
def ffi(sl):
    from seqlib_amd import _ffi
    return _ffi


def write(bamio, path, pieces, batch_bytes=None, counters=()):
    """pieces: bytes, or the string "flush"; -> (file bytes, {counter: value} read before close)"""
    w = bamio.Writer(path)
    if batch_bytes is not None:
        w.set("batch_bytes", batch_bytes)
    for p in pieces:
        if isinstance(p, str):
            w.flush()
        else:
            w.write(p)
    if counters:
        w.flush()
    got = {c: w.counter(c) for c in counters}
    w.close()
    return open(path, "rb").read(), got


def btype(raw, member):
    return (raw[member[0] + member[1]] >> 1) & 3


@pytest.mark.parametrize("kind", ["zeros", "random", "bam"])
def test_p1_sizes(bamio, tmp_path, kind):
    for n in bp.SIZES:
        payload = bp.p1()[kind, n]
        raw, c = write(bamio, tmp_path / "a.bgzf", [payload], counters=("members", "stored_members", "bytes_in", "bytes_out"))
        members = bp.check_round_trip(raw, payload)
        assert c["members"] == len(members) and c["bytes_in"] == n and c["bytes_out"] == len(raw) - 28, (n, c)
        if n == 0:
            assert raw == bu.EOF_BLOCK
        if kind == "random":                         # random blocks come out stored
            assert all(btype(raw, m) == 0 for m in members) and c["stored_members"] == len(members), (n, c)
        else:
            assert c["stored_members"] == sum(btype(raw, m) == 0 for m in members)
        if kind == "zeros" and n >= 257:
            # a member of 257 or more zeros is far smaller coded than stored, so it is a dynamic block; the 1- and 5-byte tails of the two largest sizes
            # are not held to that: a dynamic block's header alone is longer than the 5 bytes a stored one adds
            assert all(btype(raw, m) == 2 for m in members if m[3] >= 257) and sum(m[2] for m in members) <= 60 + n // 100


def test_p2_distance_cap(bamio, tmp_path):
    for name, payload in bp.p2().items():
        raw, _ = write(bamio, tmp_path / "a.bgzf", [payload])
        assert len(bp.check_round_trip(raw, payload)) == 1, name


def test_p3_overlapping_and_maximal_matches(bamio, tmp_path):
    for name, payload in bp.p3().items():
        raw, _ = write(bamio, tmp_path / "a.bgzf", [payload])
        members = bp.check_round_trip(raw, payload)
        if name == "abc":
            assert btype(raw, members[0]) == 2 and members[0][2] < 600
        if name == "zeros200k":
            assert sum(m[2] for m in members) < 200000 // 100


def test_p4_length_limiter(bamio, tmp_path):
    raw, _ = write(bamio, tmp_path / "a.bgzf", [bp.p4()])
    members = bp.check_round_trip(raw, bp.p4())
    assert len(members) == 1 and btype(raw, members[0]) == 2 and members[0][2] < 46367 // 2


@pytest.fixture(scope="module")
def p5_file(bamio, tmp_path_factory):
    """the P5 sample stream written in one call at the default batch size: the file the other ways of writing it are held against"""
    d = tmp_path_factory.mktemp("p5")
    raw, _ = write(bamio, d / "one.bam", [bp.p5_sample()])
    return d / "one.bam", raw


def test_p5_bam_round_trip_and_size(bamio, tmp_path, p5_file):
    members = bp.check_round_trip(p5_file[1], bp.p5_sample())
    assert len(members) == 36
    fq = bp.p5_fastq()
    raw, _ = write(bamio, tmp_path / "fq.bam", [fq])
    gpu = sum(m[2] for m in bp.check_round_trip(raw, fq))
    fixed, huff = bp.zlib_total(fq, level=6, strategy=bu.zlib.Z_FIXED), bp.zlib_total(fq, level=6, strategy=bu.zlib.Z_HUFFMAN_ONLY)
    print("p5/fastq deflate bytes: gpu %d, zlib fixed %d, huffman-only %d, level 1 %d, level 6 %d" % (gpu, fixed, huff, bp.zlib_total(fq, level=1), bp.zlib_total(fq, level=6)))
    assert gpu < fixed and gpu < huff


def test_splitting_does_not_matter(bamio, tmp_path, p5_file):
    """one call, seeded pieces of 1..700 bytes, batch_bytes of one member, of 3 members + 17, the default: byte-identical files; and again: the same bytes"""
    payload, want = bp.p5_sample(), p5_file[1]
    rng, pieces, o = random.Random(77), [], 0
    while o < len(payload):
        k = rng.randrange(1, 701)
        pieces.append(payload[o:o + k])
        o += k
    assert write(bamio, tmp_path / "pieces.bam", pieces)[0] == want
    assert write(bamio, tmp_path / "b1.bam", [payload], batch_bytes=0xff00)[0] == want
    assert write(bamio, tmp_path / "b3.bam", [payload], batch_bytes=3 * 0xff00 + 17)[0] == want
    assert write(bamio, tmp_path / "b3p.bam", pieces, batch_bytes=3 * 0xff00 + 17)[0] == want
    assert write(bamio, tmp_path / "again.bam", [payload])[0] == want


def test_flush_ends_the_member(bamio, tmp_path):
    a, b = bp.p5_sample()[:2 * 0xff00 + 100], bp.p5_sample()[300000:300000 + 0xff00 + 7]
    raw, c = write(bamio, tmp_path / "f.bgzf", [a, "flush", "flush", b, "flush", "flush"], counters=("members",))
    members, eof = bu.scan_members(raw)
    assert eof and [m[3] for m in members[:-1]] == bp.isize_list(a) + bp.isize_list(b) and c["members"] == 5
    assert bu.inflate_all(raw) == a + b
    # the same with a batch of one member: the flush points are the stream's, not the batches'
    assert write(bamio, tmp_path / "g.bgzf", [a[:11], a[11:], "flush", b], batch_bytes=0xff00)[0] == raw


def copy_through_device(bamio, src, dst, regions=None, max_bytes=1 << 20):
    """header from the host, then every batch of the reader from its device stream"""
    rd = bamio.Reader(src)
    text, refs = rd.header()
    if regions is not None:
        rd.set_regions(regions)
    w = bamio.Writer(dst)
    w.write(bu.bam_header(text, refs))
    w.flush()
    n = 0
    while True:
        recs, b = rd.next(max_bytes)
        if not recs:
            break
        w.write_device(b.d_stream, b.n_bytes)
        n += len(recs)
    w.close()
    rd.close()
    return n


def test_device_input(bamio, tmp_path):
    recs = bu.sample_records(3000)
    src = tmp_path / "src.bam"
    src.write_bytes(bu.bam_bytes(bu.TEXT, bu.REFS, recs))
    assert copy_through_device(bamio, src, tmp_path / "dst.bam", max_bytes=300000) == len(recs)
    text, refs, got = bu.parse_bam((tmp_path / "dst.bam").read_bytes())
    assert text == bu.TEXT and refs == bu.REFS and [r["raw"] for r in got] == recs
    # the same stream from the host gives the same file
    host, _ = write(bamio, tmp_path / "host.bam", [bu.bam_header(bu.TEXT, bu.REFS), "flush", b"".join(recs)])
    assert host == (tmp_path / "dst.bam").read_bytes()


def test_device_input_after_set_regions(bamio, tmp_path):
    raw = ba.sorted_bam()
    src = tmp_path / "s.bam"
    src.write_bytes(raw)
    (tmp_path / "s.bam.bai").write_bytes(ba.build_bai(raw))
    all_recs = bu.parse_bam(raw)[2]
    regs = [(0, 15000, 42000), (1, 0, 20000), (3, 99000, 100001)]
    want = [r for reg in regs for r in ba.region_filter(all_recs, *reg)]
    assert copy_through_device(bamio, src, tmp_path / "reg.bam", regions=regs) == len(want) > 100
    assert [r["raw"] for r in bu.parse_bam((tmp_path / "reg.bam").read_bytes())[2]] == want


def test_own_reader_and_index(bamio, tmp_path, p5_file):
    """the GPU-written BAM through bamio.Reader; and the index of a GPU-written sorted BAM byte for byte the one tests/bai_util.py writes from that file's bytes"""
    rd = bamio.Reader(p5_file[0])
    assert rd.header() == (bu.TEXT, bu.REFS)
    got = []
    while True:
        recs, _ = rd.next(1 << 20)
        if not recs:
            break
        got += recs
    rd.close()
    assert got == bu.sample_records(6000)
    stream = bu.bam_header(ba.TEXT, ba.REFS)
    raw, _ = write(bamio, tmp_path / "sorted.bam", [stream, "flush", b"".join(ba.sorted_records())])
    bamio.index_build(tmp_path / "sorted.bam")
    assert (tmp_path / "sorted.bam.bai").read_bytes() == ba.build_bai(raw)


def test_error_paths(bamio, ffi, tmp_path):
    with pytest.raises(ffi.SlxError) as e:
        bamio.Writer(tmp_path / "no_such_dir" / "a.bam")
    assert e.value.code == ffi.SLX_EIO and "no_such_dir" in str(e.value)
    w = bamio.Writer(tmp_path / "a.bam")
    assert bamio.lib().slx_bgzf_write(w.h, b"abc", -1) == ffi.SLX_EINVAL
    assert bamio.lib().slx_bgzf_write_device(w.h, None, -5) == ffi.SLX_EINVAL
    with pytest.raises(ffi.SlxError) as e:
        w.set("batch_bytes", 100)
    assert e.value.code == ffi.SLX_EINVAL
    with pytest.raises(ffi.SlxError):
        w.set("no_such_key", 1)
    assert w.counter("no_such_counter") == -1
    w.write(b"still works")                          # none of these is sticky: they never reached the writer
    w.close()
    assert bu.inflate_all((tmp_path / "a.bam").read_bytes()) == b"still works"
