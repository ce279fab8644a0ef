"""GPU tests of the BamReader path at the C-ABI (include/seqlib_amd_bam.h through seqlib_amd/bamio.py): k_bgzf_inflate + k_bgzf_crc against zlib on every
compression setting and payload of the corpus, the error paths (a flipped CRC byte, one damaged deflate byte -- the input the host-compiled build has
passed under the sanitizers in tests/test_bam_reader.py), records and header against the Python parser over a sweep of batch sizes, and the index's
repair path (the decoy, idx_fail).  The C++ class is driven in tests/test_cpp_bam.py.
Members no zlib writes (other encoders' valid DEFLATE, crafted bit by bit) go through the same kernels in tests/test_gpu_inflate_foreign.py."""
import pytest

from tests import bam_util as bu
from tests.test_bam_reader import corpus

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


def test_inflate_parity_with_zlib(bamio, tmp_path):
    """every corpus entry alone (its own file, EOF block behind it), then all of them in one file with empty members and the EOF member in mid-file"""
    entries = corpus()
    for i, (name, comp, payload) in enumerate(entries):
        p = tmp_path / ("m%d.gz" % i)
        p.write_bytes(bu.member_from_deflate(comp, payload) + bu.EOF_BLOCK)
        assert bamio.inflate_file(p) == payload, name
    allm = b"".join(bu.member_from_deflate(c, pl) + (bu.EOF_BLOCK if i % 5 == 2 else b"") for i, (_, c, pl) in enumerate(entries)) + bu.EOF_BLOCK
    p = tmp_path / "all.gz"
    p.write_bytes(allm)
    got = bamio.inflate_file(p)
    assert got == b"".join(pl for _, _, pl in entries) == bu.inflate_all(allm)
    # a file of many full members: one launch, members at their scanned offsets
    big = bu.bam_bytes(bu.TEXT, bu.REFS, bu.sample_records(6000))
    p.write_bytes(big)
    assert bamio.inflate_file(p) == bu.inflate_all(big) and len(bu.scan_members(big)[0]) > 30


def test_flipped_crc_byte_names_the_member(bamio, ffi, tmp_path):
    raw = bytearray(bu.bam_bytes(bu.TEXT, bu.REFS, bu.sample_records(900), member_size=0x4000))
    members = bu.scan_members(bytes(raw))[0]
    off, doff, dlen = members[5][:3]
    raw[off + doff + dlen + 1] ^= 0x40
    p = tmp_path / "crc.bam"
    p.write_bytes(bytes(raw))
    with pytest.raises(ffi.SlxError) as e:
        bamio.inflate_file(p)
    assert e.value.code == ffi.SLX_EIO and ("file offset %d " % off) in str(e.value) and "CRC32" in str(e.value)


def test_damaged_deflate_byte_is_an_error(bamio, ffi, tmp_path):
    """one input, one call: the error path returns SLX_EIO naming the member and the process goes on"""
    raw = bytearray(bu.bam_bytes(bu.TEXT, bu.REFS, bu.sample_records(900), member_size=0x4000))
    members = bu.scan_members(bytes(raw))[0]
    off, doff, dlen = members[3][:3]
    raw[off + doff + 40] ^= 0x10
    p = tmp_path / "dmg.bam"
    p.write_bytes(bytes(raw))
    with pytest.raises(ffi.SlxError) as e:
        bamio.inflate_file(p)
    assert e.value.code == ffi.SLX_EIO and ("file offset %d " % off) in str(e.value)
    good = tmp_path / "good.bam"
    good.write_bytes(bu.bam_bytes(bu.TEXT, bu.REFS, bu.sample_records(50)))
    assert len(bamio.inflate_file(good)) > 1000


def read_all(rd, max_bytes):
    out, rep, nb = [], 0, 0
    while True:
        recs, b = rd.next(max_bytes)
        if not recs:
            return out, rep, nb
        out += recs
        rep += b.n_repaired_chunks
        nb += 1


def test_records_and_header_equal_the_python_parser(bamio, ffi, tmp_path):
    recs = bu.sample_records(2500)
    for k, (msize, own) in enumerate(((bu.MEMBER_MAX, True), (0x1234, False), (300, True))):
        raw = bu.bam_bytes(bu.TEXT, bu.REFS, recs if msize > 1000 else recs[:300], member_size=msize, header_own_members=own)
        p = tmp_path / ("r%d.bam" % k)
        p.write_bytes(raw)
        text, refs, want = bu.parse_bam(raw)
        rd = bamio.Reader(p)
        assert rd.header() == (text, refs) == (bu.TEXT, bu.REFS)
        got, rep, _ = read_all(rd, 64 << 20)
        assert got == [w["raw"] for w in want] and rep == 0
        assert rd.next()[0] == []                                    # the end of the file stays the end
        rd.rewind()
        # batch sizes below one record, inside a record, inside a member, around a member
        for mb in (1, 37, 500, 4097, msize, msize + 1, 3 * msize + 11, 200001):
            rd.rewind()
            got, rep, nb = read_all(rd, mb)
            assert got == [w["raw"] for w in want] and rep == 0, (msize, mb)
            assert nb > 1 or mb > 100000
        rd.close()
    # a file without the EOF block opens (warning) and says so; a truncated last record is an error
    p = tmp_path / "noeof.bam"
    raw = bu.bam_bytes(bu.TEXT, bu.REFS, recs[:200])
    p.write_bytes(raw[:-28])
    rd = bamio.Reader(p)
    assert rd.counter("missing_eof") == 1 and len(read_all(rd, 1 << 20)[0]) == 200
    cut = bu.bgzf_bytes(bu.bam_header(bu.TEXT, bu.REFS) + b"".join(recs[:200])[:-9])
    p.write_bytes(cut)
    rd = bamio.Reader(p)
    with pytest.raises(ffi.SlxError) as e:
        read_all(rd, 1 << 20)
    assert e.value.code == ffi.SLX_EIO and "ends inside a record" in str(e.value)
    # not a BAM inside the BGZF
    p.write_bytes(bu.bgzf_bytes(b"@HD\tVN:1.6\nread1\t4\t*\t0\t0\t*\t*\t0\t0\tACGT\t*\n"))
    with pytest.raises(ffi.SlxError) as e:
        bamio.Reader(p)
    assert e.value.code == ffi.SLX_EIO and "SAM text" in str(e.value)


def test_index_repair(bamio, tmp_path):
    recs = bu.sample_records(2500)
    want = [bytes(r) for r in recs]
    p = tmp_path / "a.bam"
    p.write_bytes(bu.bam_bytes(bu.TEXT, bu.REFS, recs))
    rd = bamio.Reader(p)
    for chunk in (65536, 4096, 999):
        rd.rewind()
        rd.set("chunk_bytes", chunk)
        rd.set("idx_fail", 0)
        got, rep, _ = read_all(rd, 64 << 20)
        assert got == want and rep == 0, chunk
        rd.rewind()
        rd.set("idx_fail", 1)
        got, rep, _ = read_all(rd, 64 << 20)
        assert got == want and rep > 0, chunk
        rd.rewind()
        got, rep, _ = read_all(rd, 100000)                            # forced failure with batches that cut records
        assert got == want and rep > 0, chunk
    assert rd.counter("repaired_chunks") > 0
    rd.close()
    # the decoy: chunk 1 begins inside a B:C array that holds a chain of plausible headers
    dec = bu.decoy_records()
    p.write_bytes(bu.bam_bytes(bu.TEXT, bu.REFS, dec))
    rd = bamio.Reader(p)
    got, rep, nb = read_all(rd, 64 << 20)
    assert got == dec and rep >= 1 and nb == 1
    # records longer than a chunk
    long_recs = [bu.bam_record("long%d" % i, 4, -1, -1, 0, [], "ACGT" * 60000, bytes([9]) * 240000) for i in range(3)]
    mixed = recs[:50] + long_recs[:1] + recs[50:90] + long_recs[1:] + recs[90:200]
    p.write_bytes(bu.bam_bytes(bu.TEXT, bu.REFS, mixed))
    rd = bamio.Reader(p)
    got, rep, _ = read_all(rd, 64 << 20)
    assert got == mixed and rep == 0
    rd.rewind()
    got, rep, _ = read_all(rd, 70000)
    assert got == mixed and rep == 0


def test_reads_device_unpacks_the_kept_records(bamio, sl, tmp_path):
    """slx_bam_reads_device: flag filter, as stored and as sequenced (IUPAC reverse complement), in slx_align_batch_device's layout"""
    import ctypes as C
    import torch
    recs = bu.sample_records(700)
    raw = bu.bam_bytes(bu.TEXT, bu.REFS, recs)
    p = tmp_path / "a.bam"
    p.write_bytes(raw)
    want = bu.parse_bam(raw)[2]
    rd = bamio.Reader(p)
    _, b = rd.next()
    # the HIP runtime the library itself runs on, to read its device buffers with: the one mapped into the process (torch's own copy when torch initialised
    # the GPU first and the library's soname resolved to it; ROCm's otherwise)
    paths = sorted({ln.split()[-1] for ln in open("/proc/self/maps") if "libamdhip64" in ln}, key=lambda x: "torch" in x)
    assert paths, "no HIP runtime mapped"
    hip = C.CDLL(paths[0])
    hip.hipMemcpy.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int]
    for skip, orig in ((0x900, False), (0x900, True), (0, True), (0x4, False)):
        db, do, n, rmap = rd.reads_device(skip, orig)
        keep = [i for i, w in enumerate(want) if not (w["flag"] & skip)]
        assert rmap == keep and n == len(keep)
        offs = (C.c_uint64 * (n + 1))()
        assert hip.hipMemcpy(offs, do, 8 * (n + 1), 2) == 0
        offs = list(offs)
        bases = C.create_string_buffer(max(offs[-1], 1))
        assert hip.hipMemcpy(bases, db, offs[-1], 2) == 0
        for j, i in enumerate(keep):
            s = want[i]["seq"]
            if orig and want[i]["flag"] & 0x10:
                s = bu.revcomp(s)
            assert bases.raw[offs[j]:offs[j + 1]].decode() == s, (skip, orig, i)
    assert torch.cuda.is_available()
