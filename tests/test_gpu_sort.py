"""GPU tests of the coordinate sort (include/seqlib_amd_sort.h) through seqlib_amd/sortio.py: the sorted stream is Python's sorted() of the input records by
(tid as unsigned, pos) byte for byte, ties in input order; the knobs change nothing; the output is what slx_bam_index_build and the region iteration take; a
sorted file comes out unchanged; the edges and the refusals.  The C++ side is tests/test_cpp_sort.py."""
import re
import struct

import pytest

from tests import bai_util as ba
from tests import bam_util as bu

pytestmark = pytest.mark.gpu

N_TIES = 130
TIE_AT = (1, 4242)


def key(rec):
    refid, pos = struct.unpack_from("<ii", rec, 4)
    return (refid & 0xffffffff, pos)


def build_input():
    """bu.sample_records(400) with, scattered through it, a block of 130 records at one (tid, pos) with alternating strand flags and distinct names; a record at
    pos -1 on tid 0, one of 10 000 bytes and the 38-byte one"""
    recs = list(bu.sample_records(400))
    ties = [bu.bam_record("tie%03d" % i, 0x10 if i % 2 else 0, TIE_AT[0], TIE_AT[1], 30, [("M", 20)], "ACGTA" * 4, bytes([30]) * 20) for i in range(N_TIES)]
    for i, t in enumerate(ties):                             # every fourth place from 5 on: scattered, in order
        recs.insert(5 + 4 * i, t)
    recs.insert(17, bu.bam_record("minus_one", 0, 0, -1, 11, [("M", 20)], "ACGTA" * 4, bytes([30]) * 20))
    bare = len(bu.bam_record("big", 0, 2, 77, 9, [("M", 100)], "ACGT" * 25, bytes([33]) * 100))
    big = bu.bam_record("big", 0, 2, 77, 9, [("M", 100)], "ACGT" * 25, bytes([33]) * 100, b"XZZ" + b"x" * (10000 - bare - 4) + b"\0")
    assert len(big) == 10000
    recs.insert(301, big)
    tiny = bu.bam_record("a", 4, -1, -1, 0, [], "", b"")
    assert len(tiny) == 38
    recs.insert(99, tiny)
    return recs


@pytest.fixture(scope="module")
def data(sl, tmp_path_factory):
    """computed once: the input records, Python's answer, the input file (members of 0x2000 bytes)"""
    recs = build_input()
    order = sorted(range(len(recs)), key=lambda i: key(recs[i]))
    want = [recs[i] for i in order]
    assert want == sorted(recs, key=key)
    ties = [r for r in want if key(r) == TIE_AT]
    assert len(ties) == N_TIES and [r[36:42] for r in ties] == [b"tie%03d" % i for i in range(N_TIES)]          # Python's sort is stable: so is the expectation
    assert {struct.unpack_from("<H", r, 18)[0] & 0x10 for r in ties} == {0, 0x10}
    assert key(want[-1])[0] == 0xffffffff and want[0][36:45] == b"minus_one"
    d = tmp_path_factory.mktemp("sort")
    path = d / "in.bam"
    path.write_bytes(bu.bam_bytes(bu.TEXT, bu.REFS, recs, member_size=0x2000))
    return dict(recs=recs, order=order, want=want, path=path, dir=d, header=bu.bam_header(bu.TEXT.replace("SO:unsorted", "SO:coordinate"), bu.REFS))


def check_sorted(got, off, perm, data):
    want = data["want"]
    assert len(off) == len(want) + 1 and off[0] == 0 and off[-1] == len(got)
    for j, r in enumerate(want):
        assert got[off[j]:off[j + 1]] == r, "record %d of the sorted stream differs" % j
    assert got == b"".join(want)
    assert perm == data["order"]
    at = [j for j, r in enumerate(want) if key(r) == TIE_AT]
    assert perm[at[0]:at[-1] + 1] == sorted(perm[at[0]:at[-1] + 1]) and len(at) == N_TIES          # the 130 ties in input order


def test_order_and_stability_from_host(data):
    from seqlib_amd import sortio
    s = sortio.Sorter()
    recs = data["recs"]
    for a, b in ((0, 1), (1, 200), (200, 201), (201, len(recs))):          # several adds, two of one record: stable over the calls and inside them
        s.add_host(recs[a:b])
    assert s.counter("held_records") == len(recs) and s.counter("segments") == 4
    got, off, perm = s.to_host()
    check_sorted(got, off, perm, data)
    assert s.counter("held_records") == 0 and s.counter("records") == len(recs)
    s.close()


def test_order_and_stability_from_reader_batches(data):
    from seqlib_amd import bamio, sortio
    s = sortio.Sorter()
    rd = bamio.Reader(data["path"])
    n = 0
    while True:
        recs, b = rd.next(0x6000)
        if not recs:
            break
        assert recs == data["recs"][n:n + len(recs)]
        n += len(recs)
        s.add_device(b.d_stream, b.n_bytes, b.d_rec_off, b.n_records)          # the reader's buffers are reused by its next call: the sorter has its own copy
    rd.close()
    assert n == len(data["recs"]) and s.counter("segments") > 5
    got, off, perm = s.to_host()
    check_sorted(got, off, perm, data)
    s.close()


def test_knobs_change_nothing(data):
    from seqlib_amd import sortio
    first = None
    for batch_bytes in (0x2000, 3 * 0x2000 + 7, None):
        for slab_bytes in (2048, 6144, None):
            out = data["dir"] / ("out_%s_%s.bam" % (batch_bytes, slab_bytes))
            c = sortio.sort_file(data["path"], out, batch_bytes=batch_bytes, slab_bytes=slab_bytes)
            raw = out.read_bytes()
            if first is None:
                first = raw
                assert bu.inflate_all(raw) == data["header"] + b"".join(data["want"])
                text, refs, recs = bu.parse_bam(raw)
                assert text == bu.TEXT.replace("SO:unsorted", "SO:coordinate") and refs == bu.REFS and [r["raw"] for r in recs] == data["want"]
            assert raw == first, (batch_bytes, slab_bytes)
            if batch_bytes == 0x2000:
                assert c["segments"] > 10, c
            if slab_bytes == 2048:
                assert c["slabs"] == (sum(len(r) for r in data["recs"]) + 2047) // 2048 > 50, c
            if slab_bytes == 6144:
                assert c["slabs"] > 15, c
            if c:
                assert c["records"] == len(data["recs"]) and c["held_records"] == 0


def test_it_closes_the_loop(data):
    """the output is what the index build demands and what the region iteration serves"""
    from seqlib_amd import bamio, sortio
    out = data["dir"] / "loop.bam"
    sortio.sort_file(data["path"], out)
    bamio.index_build(out)
    raw = out.read_bytes()
    assert (data["dir"] / "loop.bam.bai").read_bytes() == ba.build_bai(raw)          # (the Python builder raises Unsorted on a bad order)
    _, _, recs = bu.parse_bam(raw)
    rd = bamio.Reader(out)
    assert rd.has_index()
    for region in ((1, 4000, 4300), (0, 0, 30000), (2, 50, 100)):
        rd.set_regions([region])
        got = []
        while True:
            r, _ = rd.next()
            if not r:
                break
            got += r
        want = ba.region_filter(recs, *region)
        assert got == want and want, region
    rd.close()


def test_a_sorted_file_comes_out_unchanged(data, tmp_path):
    from seqlib_amd import sortio
    src, out = tmp_path / "sorted.bam", tmp_path / "again.bam"
    src.write_bytes(ba.sorted_bam())
    sortio.sort_file(src, out)
    assert bu.inflate_all(out.read_bytes()) == bu.inflate_all(src.read_bytes())          # header unchanged, records unchanged


def test_empty_and_tiny(data, tmp_path):
    from seqlib_amd import sortio
    src, out = tmp_path / "in.bam", tmp_path / "out.bam"
    src.write_bytes(bu.bam_bytes(bu.TEXT, bu.REFS, []))
    sortio.sort_file(src, out)
    raw = out.read_bytes()
    assert bu.inflate_all(raw) == data["header"] and raw.endswith(bu.EOF_BLOCK) and len(bu.scan_members(raw)[0]) == 2          # header + EOF
    one = bu.sample_records(1)
    src.write_bytes(bu.bam_bytes(bu.TEXT, bu.REFS, one))
    sortio.sort_file(src, out)
    assert bu.inflate_all(out.read_bytes()) == data["header"] + one[0]
    s = sortio.Sorter()                                       # and the handle forms: nothing held, nothing comes down
    assert s.to_host() == (b"", [0], [])
    s.add_host(one)
    assert s.to_host() == (one[0], [0, len(one[0])], [0])
    s.close()


def test_refusals(data, tmp_path):
    from seqlib_amd import _ffi, sortio
    out = tmp_path / "out.bam"
    s = sortio.Sorter()
    # more than max_bytes: both figures, no file, the sorter goes on
    s.set("max_bytes", 100000)
    with pytest.raises(_ffi.SlxError) as e:
        s.sort_file(data["path"], out)
    figures = [int(x) for x in re.findall(r"\d+", str(e.value))]
    assert e.value.code == _ffi.SLX_EUNSUPPORTED and 100000 in figures and any(100000 < f <= sum(len(r) for r in data["recs"]) for f in figures), str(e.value)
    assert not out.exists() and s.counter("held_records") == 0
    s.set("max_bytes", 1 << 30)
    s.sort_file(data["path"], out)
    assert bu.inflate_all(out.read_bytes()) == data["header"] + b"".join(data["want"])
    out.unlink()
    # the output is the input
    with pytest.raises(_ffi.SlxError) as e:
        s.sort_file(data["path"], data["path"])
    assert e.value.code == _ffi.SLX_EINVAL
    with pytest.raises(_ffi.SlxError) as e:
        sortio.sort_file(data["path"], data["path"])
    assert e.value.code == _ffi.SLX_EINVAL and bu.inflate_all(data["path"].read_bytes())[:4] == b"BAM\1"
    # an offset table whose third entry disagrees with the block_size before it: record 2 is named, nothing is added
    recs = data["recs"][:6]
    off = [0]
    for r in recs:
        off.append(off[-1] + len(r))
    s.add_host(recs[:2])
    bad = list(off)
    bad[2] += 1
    with pytest.raises(_ffi.SlxError) as e:
        s.add_host(recs, offsets=bad)
    assert e.value.code == _ffi.SLX_EINVAL and "record 2 " in str(e.value), str(e.value)
    assert s.counter("held_records") == 2
    got, _, perm = s.to_host()
    assert got == b"".join(sorted(recs[:2], key=key)) and sorted(perm) == [0, 1]
    # slab_bytes: a multiple of the tile, at least one
    for v in (1000, 0, 2048 + 16):
        with pytest.raises(_ffi.SlxError) as e:
            s.set("slab_bytes", v)
        assert e.value.code == _ffi.SLX_EINVAL
    s.set("slab_bytes", 4096)
    assert s.counter("no_such_counter") == -1
    s.close()
