"""GPU tests of the BAI index build and of region iteration at the C-ABI (slx_bam_index_build, slx_bam_index_load, slx_bam_set_regions of
include/seqlib_amd_bam.h through seqlib_amd/bamio.py) against the Python statement in tests/bai_util.py: the index byte for byte, the refusal of unsorted
files, and for a sweep of regions the served records against the brute-force filter, in order and byte for byte.  The C++ classes are driven in
tests/test_cpp_region.py."""
import ctypes as C

import pytest

from tests import bai_util as ba
from tests import bam_util as bu

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


@pytest.fixture(scope="module")
def fx(tmp_path_factory, bamio):
    """the sorted fixture once: the file with the Python writer's index beside it (py), with the GPU's (gpu) and alone (bare)"""
    class F:
        pass
    f = F()
    f.raw = ba.sorted_bam()
    f.bai = ba.build_bai(f.raw)
    f.model = ba.parse_bai(f.bai)
    f.recs = bu.parse_bam(f.raw)[2]
    f.members = bu.scan_members(f.raw)[0]
    f.inflated = sum(m[3] for m in f.members)
    d = tmp_path_factory.mktemp("bai")
    f.dir = d
    for name in ("py", "gpu", "bare"):
        (d / name).mkdir()
        (d / name / "s.bam").write_bytes(f.raw)
    (d / "py" / "s.bam.bai").write_bytes(f.bai)
    f.py, f.gpu, f.bare = d / "py" / "s.bam", d / "gpu" / "s.bam", d / "bare" / "s.bam"
    return f


def test_index_build_equals_the_python_writer(bamio, fx):
    """byte for byte; again with 64-byte index chunks, and with batches small enough for nine or more (open runs and the order check across joins)"""
    bamio.index_build(fx.gpu)
    assert (fx.dir / "gpu" / "s.bam.bai").read_bytes() == fx.bai
    out = fx.dir / "other.bai"
    bamio.index_build(fx.bare, out, chunk_bytes=64)
    assert out.read_bytes() == fx.bai
    batch = 10 * ba.MEMBER_SIZE
    assert fx.inflated // batch >= 8
    for b in (batch, ba.MEMBER_SIZE, 3 * ba.MEMBER_SIZE + 7):
        bamio.index_build(fx.bare, out, batch_bytes=b)
        assert out.read_bytes() == fx.bai, b
    bamio.index_build(fx.bare, out, batch_bytes=batch, chunk_bytes=64)
    assert out.read_bytes() == fx.bai
    assert not (fx.dir / "bare" / "s.bam.bai").exists()


def test_unsorted_files_are_refused(bamio, ffi, fx, tmp_path):
    """one call each: the unsorted sample file, and the sorted fixture with one pair swapped across the first batch join"""
    raw = bu.bam_bytes(bu.TEXT, bu.REFS, bu.sample_records(400))
    with pytest.raises(ba.Unsorted) as m:
        ba.build_bai(raw)
    p = tmp_path / "u.bam"
    p.write_bytes(raw)
    with pytest.raises(ffi.SlxError) as e:
        bamio.index_build(p)
    assert e.value.code == ffi.SLX_EINVAL and ("record %d " % m.value.ordinal) in str(e.value) and not (tmp_path / "u.bam.bai").exists()
    # the pair (k, k + 1): k the last whole record of the first batch, k + 1 the one the batch's end cuts, before and after the swap
    recs = ba.sorted_records()
    specs = ba.sorted_specs()
    off = [0]
    for r in recs:
        off.append(off[-1] + len(r))
    found = None
    for nmem in range(4, 40):
        B = nmem * ba.MEMBER_SIZE
        k = max(i for i in range(len(recs)) if off[i + 1] <= B)
        key = lambda s: (s["refid"] & 0xffffffff, s["pos"])
        if key(specs[k]) < key(specs[k + 1]) and off[k] + len(recs[k + 1]) <= B < off[k + 2]:
            found = (B, k)
            break
    assert found
    B, k = found
    recs[k], recs[k + 1] = recs[k + 1], recs[k]
    raw = bu.bam_bytes(ba.TEXT, ba.REFS, recs, member_size=ba.MEMBER_SIZE)
    with pytest.raises(ba.Unsorted) as m:
        ba.build_bai(raw)
    assert m.value.ordinal == k + 1
    p = tmp_path / "swap.bam"
    p.write_bytes(raw)
    with pytest.raises(ffi.SlxError) as e:
        bamio.index_build(p, batch_bytes=B)
    assert e.value.code == ffi.SLX_EINVAL and ("record %d " % (k + 1)) in str(e.value) and not (tmp_path / "swap.bam.bai").exists()


def read_all(rd, max_bytes):
    out = []
    while True:
        recs, _ = rd.next(max_bytes)
        if not recs:
            return out
        out += recs


# (tid, beg, end): each edge case of the fixture, and around it
REGIONS = [
    (0, 0, 1),                                               # the record at pos 0
    (0, 16383, 16384), (0, 16384, 16385), (0, 16384, 16500),   # a record whose end is 16384: in, out (beg equal to its end), out
    (1, 16000, 16384), (1, 16384, 16385),                    # a record whose pos is 16384: out (end equal to its pos), in
    (0, 60000, 60001),                                       # inside the long N
    (1, 70000, 70001), (1, 70010, 70011),                    # mapped without CIGAR; 0x4 with coordinates
    (0, ba.CIG300_POS + 149, ba.CIG300_POS + 150), (0, ba.CIG300_POS + 150, ba.CIG300_POS + 151),      # 300 ops: its last base in, the base behind it out
    (1, 50000, 50001),                                       # the record that ends where a member ends
    (2, 0, 50000),                                           # the reference without records
    (3, 0, 100001), (0, 0, 1 << 29),                         # whole references
    (3, 1 << 20, 1 << 21),                                   # beg past the last window
]
ONE_WINDOW = [r for r in REGIONS if r[2] - r[1] <= 16384 and r[1] >> 14 == (r[2] - 1) >> 14]


@pytest.mark.parametrize("source", ["py", "gpu"])
def test_regions_equal_the_brute_force_filter(bamio, fx, source):
    if source == "gpu" and not (fx.dir / "gpu" / "s.bam.bai").exists():
        bamio.index_build(fx.gpu)
    rd = bamio.Reader(getattr(fx, source))
    assert rd.has_index()
    name_of = {r["raw"]: r["name"] for r in fx.recs}
    names = lambda raws: {name_of[x] for x in raws}
    for chunk in (65536, 64):
        rd.set("chunk_bytes", chunk)
        for mb in (ba.MEMBER_SIZE, 50000, 64 << 20):
            for reg in REGIONS:
                want = ba.region_filter(fx.recs, *reg)
                kept0, done0 = rd.counter("region_kept"), rd.counter("members_done")
                rd.set_regions([reg])
                got = read_all(rd, mb)
                assert got == want, (chunk, mb, reg)
                assert rd.counter("region_kept") - kept0 == len(want) and rd.counter("regions_done") == 1
                assert rd.counter("region_candidates") >= rd.counter("region_kept")
                if reg in ONE_WINDOW:                # a cap on the work: no more members than the plan names
                    assert rd.counter("members_done") - done0 <= ba.plan_members(fx.members, ba.query(fx.model, *reg)), (chunk, mb, reg)
    # the sweep holds what it is for
    got = {reg: names(ba.region_filter(fx.recs, *reg)) for reg in REGIONS}
    assert "at_zero" in got[REGIONS[0]] and "ends_16384" in got[REGIONS[1]] and "ends_16384" not in got[REGIONS[2]] | got[REGIONS[3]]
    assert "starts_16384" not in got[REGIONS[4]] and "starts_16384" in got[REGIONS[5]] and "long_n" in got[REGIONS[6]]
    assert "no_cigar" in got[REGIONS[7]] and "unmapped_placed" in got[REGIONS[8]] and "cig300" in got[REGIONS[9]] and "cig300" not in got[REGIONS[10]]
    assert "pad" in got[REGIONS[11]] and not got[REGIONS[12]] and len(got[REGIONS[13]]) > 400 and not got[REGIONS[15]]
    assert len(ONE_WINDOW) >= 10
    rd.close()


def test_region_lists(bamio, ffi, fx):
    """regions are served in the order given, a record once per region it overlaps; n = 0 and rewind give the whole file back; no index, no regions"""
    rd = bamio.Reader(fx.py)
    regs = [(1, 60000, 90000), (0, 16000, 17000), (0, 16300, 70000), (2, 0, 100), (1, 69000, 70011), (0, 0, 1)]
    want = [r for reg in regs for r in ba.region_filter(fx.recs, *reg)]
    assert len(set(want)) < len(want)
    whole = [r["raw"] for r in fx.recs]
    for mb in (64 << 20, 30000, 1):
        rd.set_regions(regs)
        assert read_all(rd, mb) == want, mb
        assert rd.counter("regions_done") == len(regs) and rd.next(mb)[0] == []
    rd.set_regions([])
    assert read_all(rd, 64 << 20) == whole
    rd.set_regions(regs)
    first = rd.next(30000)[0]
    assert 0 < len(first) < len(want) and first == want[:len(first)]
    rd.rewind()
    assert read_all(rd, 100000) == whole and rd.counter("regions_done") == 0
    with pytest.raises(ffi.SlxError) as e:
        rd.set_regions([(4, 0, 10)])
    assert e.value.code == ffi.SLX_EINVAL
    rd.close()
    bare = bamio.Reader(fx.bare)
    assert not bare.has_index()
    with pytest.raises(ffi.SlxError) as e:
        bare.set_regions([(0, 0, 10)])
    assert e.value.code == ffi.SLX_EINVAL and "no index" in str(e.value)
    bare.index_load(fx.dir / "py" / "s.bam.bai")
    bare.set_regions([(0, 0, 1)])
    assert read_all(bare, 64 << 20) == ba.region_filter(fx.recs, 0, 0, 1)
    # an index of another file: refused with a message, the file stays open and unindexed
    other = fx.dir / "other_refs.bai"
    other.write_bytes(ba.build_bai(bu.bam_bytes(bu.TEXT, bu.REFS, [])))
    bare2 = bamio.Reader(fx.bare)
    with pytest.raises(ffi.SlxError) as e:
        bare2.index_load(other)
    assert e.value.code == ffi.SLX_EINVAL and not bare2.has_index()


def test_reads_device_on_a_region_batch(bamio, fx):
    """the sequences slx_bam_reads_device unpacks from a region batch are those of the kept records, as stored and as sequenced"""
    rd = bamio.Reader(fx.py)
    reg = (0, 16000, 60000)
    rd.set_regions([reg])
    raws, b = rd.next()
    want = [r for r in fx.recs if r["refid"] == reg[0] and r["pos"] < reg[2] and ba.rec_end(r) > reg[1]]
    assert raws == [w["raw"] for w in want] and len(want) > 100
    paths = sorted({ln.split()[-1] for ln in open("/proc/self/maps") if "libamdhip64" in ln}, key=lambda x: "torch" in x)
    assert paths, "no HIP runtime mapped"
    hip = C.CDLL(paths[0])
    hip.hipMemcpy.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int]
    for skip, orig in ((0x900, False), (0, True)):
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
