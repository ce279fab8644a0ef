"""GPU tests of the SAM text reader at the C-ABI (include/seqlib_amd_sam.h through seqlib_amd/samio.py) against the Python statement of the grammar in
tests/sam_util.py: the batches byte for byte over every source kind, batch size and tile size, host and device copies, the fast and the slow path, a 70 000-base
record, one-line files, files with one bad line, the batch going on to slx_bam_reads_device, a read filter, slx_bgzf_write_device and slx_sort_add_device, and the
refusal of index and region calls.  The C++ class is driven in tests/test_cpp_sam.py."""
import ctypes as C
import struct

import pytest

from tests import bam_util as bu
from tests import fastq_util
from tests import filter_util as fu
from tests import sam_util as su
from tests.test_gpu_filter import Hip

pytestmark = pytest.mark.gpu

MAX_BYTES = (1, 37, 500, 4097, 65536, 64 << 20)
SOURCES = {"plain": lambda t: t, "bgzf300": lambda t: bu.bgzf_bytes(t, 300), "bgzf3000": lambda t: bu.bgzf_bytes(t, 0x3000), "gzip": lambda t: fastq_util.gzip_(t)}
SOURCE_CODE = {"plain": 0, "bgzf300": 1, "bgzf3000": 1, "gzip": 2}


@pytest.fixture(scope="module")
def fx(sl, tmp_path_factory):
    """computed once: the lines (the canonical fixture with every good single-line case spread among it), Python's records, one file per source kind"""
    from seqlib_amd import _ffi, bamio, filterio, samio, sortio
    samio.lib()

    class F:
        pass
    f = F()
    f.ffi, f.bamio, f.filterio, f.samio, f.sortio, f.hip = _ffi, bamio, filterio, samio, sortio, Hip()
    lines, _ = su.canonical(400)
    good = [c[1] for c in su.CASES if c[2]]
    for i, ln in enumerate(good):
        lines.insert(3 * i + 1, ln)
    f.lines = lines
    f.text = su.sam_text(bu.TEXT, lines)
    text, refs, f.recs, bad = su.parse_text(f.text)
    assert bad is None and len(f.recs) == len(lines) and (text, refs) == (bu.TEXT.encode(), bu.REFS)
    f.n_slow = sum(su.is_slow(ln) for ln in lines)
    assert 3 <= f.n_slow < 20          # f, d and B:f fields among the good cases
    f.dir = tmp_path_factory.mktemp("sam")
    f.paths = {}
    for k, wrap in SOURCES.items():
        f.paths[k] = f.dir / ("all_%s.sam" % k)
        f.paths[k].write_bytes(wrap(f.text))
    return f


def read_all(f, rd, max_bytes, device_too=True):
    """every batch -> records from the host copies; the device copies are held against them"""
    out, batches, members = [], 0, 0
    while True:
        raws, b = rd.next(max_bytes)
        if not raws:
            assert b.n_records == 0
            return out, batches, members
        assert b.n_bytes == sum(len(x) for x in raws) and b.n_repaired_chunks == 0
        if device_too:
            assert f.hip.down(b.d_stream, b.n_bytes) == b"".join(raws)
            assert f.hip.down(b.d_rec_off, 8 * (b.n_records + 1)) == C.string_at(b.rec_off, 8 * (b.n_records + 1))
        out += raws
        batches += 1
        members += b.n_members


@pytest.mark.parametrize("tile", [16, 4096])
@pytest.mark.parametrize("source", list(SOURCES))
def test_batches_equal_the_python_parser(fx, source, tile):
    rd = fx.samio.Reader(fx.paths[source])
    assert rd.header() == (bu.TEXT, bu.REFS)
    assert rd.counter("sam") == 1 and rd.counter("source") == SOURCE_CODE[source] and not rd.has_index()
    rd.set("sam_tile_bytes", tile)
    n_batches = {}
    for mb in MAX_BYTES:
        got, n_batches[mb], members = read_all(fx, rd, mb, device_too=mb >= 500)
        assert got == fx.recs, (source, tile, mb, len(got))
        assert rd.counter("lines") == bu.TEXT.count("\n") + len(fx.lines)
        assert rd.counter("fast_records") == len(fx.lines) - fx.n_slow and rd.counter("slow_records") == fx.n_slow
        assert (members > 0) == (SOURCE_CODE[source] == 1)
        assert rd.next(mb)[0] == []          # the end stays the end
        rd.rewind()                          # and the next size starts over
    if source == "plain":
        # a batch is grown until it holds one whole line (it may then hold a few short ones); text that fits max_bytes is one batch
        assert n_batches[64 << 20] == 1 and 1 < n_batches[4097] < min(n_batches[500], n_batches[1]) and n_batches[1] <= len(fx.lines)
    rd.close()


def test_fast_and_slow_paths_give_the_same_bytes(fx):
    rd = fx.samio.Reader(fx.paths["plain"])
    rd.set("sam_fast_fail", 1)
    for mb in (500, 64 << 20):
        got, _, _ = read_all(fx, rd, mb)
        assert got == fx.recs
        assert rd.counter("fast_records") == 0 and rd.counter("slow_records") == len(fx.lines)
        rd.rewind()
    rd.set("sam_fast_fail", 0)
    got, _, _ = read_all(fx, rd, 64 << 20)
    assert got == fx.recs and rd.counter("fast_records") == len(fx.lines) - fx.n_slow
    assert rd.counter("us_fields") > 0 and rd.counter("us_size") > 0 and rd.counter("us_fill") > 0 and rd.counter("us_lines") > 0
    with pytest.raises(fx.ffi.SlxError):
        rd.set("sam_tile_bytes", 24)
    with pytest.raises(fx.ffi.SlxError):
        rd.set("sam_fast_fail", 2)
    rd.close()
    bam = fx.dir / "plain.bam"
    bam.write_bytes(bu.bam_bytes(bu.TEXT, bu.REFS, fx.recs[:10]))
    rb = fx.bamio.Reader(bam)
    assert rb.counter("sam") == 0
    with pytest.raises(fx.ffi.SlxError):
        rb.set("sam_fast_fail", 1)          # the names belong to a SAM reader
    rb.close()


def test_a_long_record_and_one_line_files(fx, tmp_path):
    import random
    rng = random.Random(11)
    L = 70000
    seq = "".join(rng.choice("ACGTNacgtRY") for _ in range(L)).encode()
    qual = bytes(rng.randrange(33, 127) for _ in range(L))
    long_line = su._l(qname=b"long", cigar=b"100S69800M100S", seq=seq, qual=qual, aux=[b"XZ:Z:" + b"z" * 3000, b"XI:i:-70000"])
    lines = fx.lines[:7] + [long_line] + fx.lines[7:15]
    want = [su.line_to_record(ln, bu.REFS) for ln in lines]
    p = tmp_path / "long.sam"
    p.write_bytes(su.sam_text(bu.TEXT, lines))
    for mb in (1000, 64 << 20):
        for ff in (0, 1):
            rd = fx.samio.Reader(p)
            rd.set("sam_fast_fail", ff)
            got, _, _ = read_all(fx, rd, mb)
            assert got == want, (mb, ff)
            rd.close()
    for hdr in (bu.TEXT, ""):
        for last_eol in (True, False):
            for eol in (b"\n", b"\r\n"):
                one = tmp_path / "one.sam"
                cr_at_the_end = b"\r" if eol == b"\r\n" and not last_eol else b""
                one.write_bytes(su.sam_text(hdr, [su.CASES[0][1] if hdr else su._l(rname=b"*", rnext=b"*")], eol, last_eol) + cr_at_the_end)
                text, refs, want1, bad = su.parse_text(one.read_bytes())
                rd = fx.samio.Reader(one)
                if eol == b"\r\n" and not last_eol:          # the input ends in CR without LF: an error, and nothing before it
                    assert bad is not None and want1 == []
                    with pytest.raises(fx.ffi.SlxError, match="line %d" % bad[0]):
                        rd.next()
                else:
                    assert bad is None and len(want1) == 1
                    assert rd.header() == (hdr.replace("\r", ""), refs)
                    assert read_all(fx, rd, 64 << 20)[0] == want1
                rd.close()
    empty = tmp_path / "header_only.sam"
    empty.write_bytes(bu.TEXT.encode())
    rd = fx.samio.Reader(empty)
    assert rd.header() == (bu.TEXT, bu.REFS) and rd.next()[0] == []
    rd.close()
    nosn = tmp_path / "nosn.sam"
    nosn.write_bytes(b"@HD\tVN:1.6\n@SQ\tLN:100\n" + su.CASES[0][1] + b"\n")
    with pytest.raises(fx.ffi.SlxError, match="@SQ") as e:
        fx.samio.Reader(nosn)
    assert e.value.code == fx.ffi.SLX_EIO


@pytest.mark.parametrize("max_bytes", [300, 64 << 20])
def test_error_files(fx, tmp_path, max_bytes):
    hdr_lines = bu.TEXT.count("\n")
    lines = fx.lines[:60]
    bads = [su._l(rname=b"chrZ"), b"", b"@CO\tlate", su._l(aux=[b"XF:f:1.0", b"XI:i:4294967296"]), su._l(qual=b"II\x7fI")]
    for where in (0, 31, 59):
        for bad in bads:
            if where == 0 and bad[:1] == b"@":
                continue
            body = lines[:where] + [bad] + lines[where + 1:]
            p = tmp_path / "bad.sam"
            p.write_bytes(su.sam_text(bu.TEXT, body))
            _, _, want, at = su.parse_text(p.read_bytes())
            assert at[0] == hdr_lines + where + 1 and want == fx.recs[:where]
            rd = fx.samio.Reader(p)
            got = []
            with pytest.raises(fx.ffi.SlxError, match=r"line %d:" % at[0]) as e:
                while True:
                    raws, b = rd.next(max_bytes)
                    assert raws, "the end of the file before the bad line is reported"
                    got += raws
            assert e.value.code == fx.ffi.SLX_EIO and got == want, (where, bad[:20])
            with pytest.raises(fx.ffi.SlxError, match=r"line %d:" % at[0]):          # and it stays reported
                rd.next(max_bytes)
            rd.rewind()
            assert rd.next(64 << 20)[0] == want if where else True
            rd.close()


def test_a_sam_batch_goes_on(fx, tmp_path):
    parsed = bu.parse_bam(bu.bam_bytes(bu.TEXT, bu.REFS, fx.recs))[2]
    bam = tmp_path / "same.bam"
    bam.write_bytes(bu.bam_bytes(bu.TEXT, bu.REFS, fx.recs, member_size=0x1800))

    def bases(rd):
        db, do, n, rmap = rd.reads_device(0x900, True)
        offs = struct.unpack("<%dQ" % (n + 1), fx.hip.down(do, 8 * (n + 1)))
        s = fx.hip.down(db, offs[-1])
        return [s[offs[i]:offs[i + 1]] for i in range(n)], rmap
    # slx_bam_reads_device
    rs, rb = fx.samio.Reader(fx.paths["bgzf300"]), fx.bamio.Reader(bam)
    raws, b = rs.next(64 << 20)
    raws_b, _ = rb.next(64 << 20)
    assert raws == fx.recs and raws_b == fx.recs
    got_s, got_b = bases(rs), bases(rb)
    assert got_s == got_b and len(got_s[0]) == sum(1 for r in parsed if not r["flag"] & 0x900) and any(got_s[0])
    # slx_bgzf_write_device: SAM to BAM with no host round trip
    out = tmp_path / "from_sam.bam"
    w = fx.bamio.Writer(out)
    w.write(bu.bam_header(bu.TEXT, bu.REFS))
    w.flush()
    w.write_device(b.d_stream, b.n_bytes)
    w.close()
    text, refs, back = bu.parse_bam(out.read_bytes())
    assert (text, refs) == (bu.TEXT, bu.REFS) and [r["raw"] for r in back] == fx.recs
    # slx_sort_add_device
    s1, s2 = fx.sortio.Sorter(), fx.sortio.Sorter()
    s1.add_device(b.d_stream, b.n_bytes, b.d_rec_off, b.n_records)
    s2.add_host(fx.recs)
    a, c = s1.to_host(), s2.to_host()
    assert a[0] == c[0] and list(a[1]) == list(c[1]) and list(a[2]) == list(c[2]) and len(a[0]) == sum(len(r) for r in fx.recs)
    s1.close()
    s2.close()
    rs.close()
    rb.close()
    # an attached read filter: the kept records of the BAM route, for a small and a large batch
    for name in ("len", "mapq"):
        for mb in (2000, 64 << 20):
            kept = {}
            for kind, rd in (("sam", fx.samio.Reader(fx.paths["plain"])), ("bam", fx.bamio.Reader(bam))):
                flt = fx.filterio.Filter(fu.RULE_SETS[name])
                flt.attach(rd)
                kept[kind] = read_all(fx, rd, mb)[0]
                assert flt.counter("seen") == len(fx.recs)
                rd.close()
                flt.close()
            assert kept["sam"] == kept["bam"] and 0 < len(kept["sam"]) < len(fx.recs), (name, mb)


def test_refusals(fx):
    rd = fx.samio.Reader(fx.paths["bgzf3000"])
    for call in (lambda: rd.set_regions([(0, 0, 1000)]), lambda: rd.index_load(), lambda: rd.index_load(str(fx.paths["plain"]))):
        with pytest.raises(fx.ffi.SlxError, match="SAM text has no index") as e:
            call()
        assert e.value.code == fx.ffi.SLX_EINVAL
    assert not rd.has_index()
    assert read_all(fx, rd, 64 << 20)[0] == fx.recs
    rd.close()
    with pytest.raises(fx.ffi.SlxError, match="SAM text") as e:          # slx_bam_open itself still refuses the text
        fx.bamio.Reader(fx.paths["bgzf3000"])
    assert e.value.code == fx.ffi.SLX_EIO
