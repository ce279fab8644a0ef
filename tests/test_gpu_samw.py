"""GPU tests of the SAM writer at the C-ABI (include/seqlib_amd_samw.h through seqlib_amd/samwio.py) against the Python statement of the rules in
tests/samw_util.py: slx_samw_format_device and the written file for the case list and the sample records, with the fast path and with every record on the slow
path; the batch shape; one 300 000-base record and a 65535-op CIGAR; the refusals; the round trip through the GPU SAM reader, plain and bgzip'd.  The C++
classes are driven in tests/test_cpp_samw.py."""
import ctypes as C
import struct

import pytest

from tests import bam_util as bu
from tests import sam_util as su
from tests import samw_util as wu

pytestmark = pytest.mark.gpu
REF_NAMES = [n for n, _ in bu.REFS]


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
def fx(sl):
    """the records and the lines of the Python statement, once"""
    from seqlib_amd import _ffi, samio, samwio
    samwio.lib()

    class F:
        pass
    f = F()
    f.ffi, f.samio, f.samwio, f.hip = _ffi, samio, samwio, Hip()
    f.good = [r for _, r, ok in wu.CASES if ok] + bu.sample_records(400)
    f.lines = [wu.record_to_line(r, bu.REFS) for r in f.good]
    f.n_slow = sum(wu.is_slow(r) for r in f.good)
    f.n_wide = sum(wu.is_wide(r) for r in f.good)
    return f


def up_batch(hip, recs):
    stream, off = wu.stream_of(recs)
    return hip.up(stream), len(stream), hip.up(struct.pack("<%dQ" % len(off), *off))


def open_writer(fx, path, bgzf=False, header=True):
    w = fx.samwio.Writer(path, bgzf=bgzf)
    if header:
        w.header(bu.TEXT, REF_NAMES)
    return w


@pytest.mark.parametrize("fast_fail", [0, 1])
def test_format_device_and_the_file_equal_python(fx, tmp_path, fast_fail):
    p = tmp_path / "a.sam"
    w = open_writer(fx, p)
    w.set("fast_fail", fast_fail)
    d_s, n_bytes, d_off = up_batch(fx.hip, fx.good)
    t = w.format_device(d_s, n_bytes, d_off, len(fx.good))
    want = b"".join(fx.lines)
    assert (t.n_bytes, t.n_records) == (len(want), len(fx.good))
    off = struct.unpack("<%dQ" % (len(fx.good) + 1), fx.hip.down(t.d_line_off, 8 * (len(fx.good) + 1)))
    want_off = [0]
    for ln in fx.lines:
        want_off.append(want_off[-1] + len(ln))
    assert list(off) == want_off
    text = fx.hip.down(t.d_text, t.n_bytes)
    bad = [i for i in range(len(fx.good)) if text[off[i]:off[i + 1]] != fx.lines[i]]
    assert not bad, (bad[:5], text[off[bad[0]]:off[bad[0] + 1]][:300], fx.lines[bad[0]][:300])
    n_slow = len(fx.good) if fast_fail else fx.n_slow
    assert (w.counter("records"), w.counter("slow_records"), w.counter("fast_records")) == (len(fx.good), n_slow, len(fx.good) - n_slow)
    assert w.counter("wide_records") == fx.n_wide > 5 and w.counter("bytes") == len(want) and w.counter("nonsense") == -1
    w.write_device(d_s, n_bytes, d_off, len(fx.good))
    w.close()
    assert p.read_bytes() == bu.TEXT.encode() + want
    with pytest.raises(fx.ffi.SlxError) as e:
        open_writer(fx, tmp_path / "b.sam").set("fast_fail", 2)
    assert e.value.code == fx.ffi.SLX_EINVAL
    fx.hip.free(d_s)
    fx.hip.free(d_off)


def test_batch_shape_does_not_show(fx, tmp_path):
    recs, want = fx.good[:120], bu.TEXT.encode() + b"".join(fx.lines[:120])
    for name, step, host in (("one", 1, True), ("seven", 7, False), ("all", len(recs), False), ("all_host", len(recs), True), ("all_small_stages", len(recs), False)):
        p = tmp_path / (name + ".sam")
        w = open_writer(fx, p)
        if name == "all_small_stages":          # the text comes down in many pieces
            w.set("stage_bytes", 4096)
            assert len(want) > 10 * 4096
        for i in range(0, len(recs), step):
            if host:
                w.write_host(*wu.stream_of(recs[i:i + step]))
            else:
                d_s, n_bytes, d_off = up_batch(fx.hip, recs[i:i + step])
                w.write_device(d_s, n_bytes, d_off, len(recs[i:i + step]))
                fx.hip.free(d_s)
                fx.hip.free(d_off)
        d_off = fx.hip.up(struct.pack("<Q", 0))
        w.write_device(None, 0, d_off, 0)          # an empty batch
        t = w.format_device(None, 0, d_off, 0)
        assert (t.n_bytes, t.n_records) == (0, 0) and fx.hip.down(t.d_line_off, 8) == bytes(8)
        w.write_host(b"", [0])
        fx.hip.free(d_off)
        w.close()
        assert p.read_bytes() == want, name
    p = tmp_path / "header_only.sam"
    open_writer(fx, p).close()
    assert p.read_bytes() == bu.TEXT.encode()
    p = tmp_path / "nothing.sam"
    open_writer(fx, p, header=False).close()
    assert p.read_bytes() == b""


def test_one_long_record_takes_several_waves(fx, tmp_path):
    n = 300000
    seq = "".join("ACGTN"[(i * i + i // 7) % 5] for i in range(n))
    long_rec = wu.make(name=b"contig", cigar=(("M", n),), seq=seq, qual=bytes((i * 7) % 94 for i in range(n)), aux=b"NMC\x03")
    cig_rec = wu.make(name=b"ops", cigar=wu._ms(65535, 3), seq="ACGT", qual=None)
    recs = [fx.good[0], long_rec, cig_rec, fx.good[1]]
    p = tmp_path / "long.sam"
    w = open_writer(fx, p)
    w.write_host(*wu.stream_of(recs))
    assert w.counter("extra_waves") == n // 8192 and w.counter("wide_records") == 1 and w.counter("slow_records") == 0
    w.close()
    assert p.read_bytes() == bu.TEXT.encode() + b"".join(wu.record_to_line(r, bu.REFS) for r in recs)


def test_a_refused_record_refuses_its_batch_only(fx, tmp_path):
    good = fx.good[:30]
    for name, rec, ok in wu.CASES:
        if ok:
            continue
        p = tmp_path / (name + ".sam")
        w = open_writer(fx, p)
        w.write_host(*wu.stream_of(good[:10]))
        with pytest.raises(fx.ffi.SlxError, match="record 13 of the batch") as e:
            w.write_host(*wu.stream_of(good[:13] + [rec] + good[13:]))
        assert e.value.code == fx.ffi.SLX_EIO, name
        w.write_host(*wu.stream_of(good[10:]))
        w.close()
        assert p.read_bytes() == bu.TEXT.encode() + b"".join(fx.lines[:30]), name
    # offsets that leave the stream, or run backwards
    w = open_writer(fx, tmp_path / "span.sam")
    stream, off = wu.stream_of(good[:3])
    for bad_off in ([0, off[1], off[2], off[3] + 4], [0, off[2], off[1], off[3]]):
        with pytest.raises(fx.ffi.SlxError, match="of the batch") as e:
            w.write_host(stream, bad_off)
        assert e.value.code == fx.ffi.SLX_EIO
    w.close()


def test_round_trip_through_the_gpu_sam_reader(fx, tmp_path):
    lines, recs = su.canonical(400)
    plain, bgz = tmp_path / "rt.sam", tmp_path / "rt.sam.gz"
    for p, bgzf in ((plain, False), (bgz, True)):
        w = open_writer(fx, p, bgzf=bgzf)
        for i in range(0, len(recs), 150):
            w.write_host(*wu.stream_of(recs[i:i + 150]))
        w.close()
    assert plain.read_bytes() == su.sam_text(bu.TEXT, lines)
    z = bgz.read_bytes()
    assert bu.scan_members(z)[1] and bu.inflate_all(z) == plain.read_bytes()
    for p in (plain, bgz):
        rd = fx.samio.Reader(p)
        got = []
        while True:
            r, _ = rd.next()
            if not r:
                break
            got += r
        rd.close()
        assert got == recs, p
