"""CPU tests of the BAI index's host side (seqlib_amd/csrc/slx_bai.cpp behind slx_bai_query / slx_bai_stats of include/seqlib_amd_bam.h) against the Python
statement in tests/bai_util.py: the reference project's own index file (tests/golden/sim.sorted.bam.bai, 1 296 bytes), every truncation of it, the parser
under ASan + UBSan, and an index the Python writer made for the sorted fixture.  No test here needs a GPU."""
import os
import subprocess

import pytest

from tests import bai_util as ba
from tests import bam_util as bu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN_BAI = os.path.join(ROOT, "tests", "golden", "sim.sorted.bam.bai")


@pytest.fixture(scope="module")
def bamio():
    import __graft_entry__ as g
    if not os.path.exists(os.path.join(ROOT, "seqlib_amd", "libseqlib_amd.so")):
        g.build()
    from seqlib_amd import bamio as b
    b.lib()
    return b


@pytest.fixture(scope="module")
def ffi(bamio):
    from seqlib_amd import _ffi
    return _ffi


def test_reference_index_file_stats(bamio):
    """the figures of the reference tree's own .bai, read from the file with the Python parser when the fixture was added"""
    assert os.path.getsize(GOLDEN_BAI) == 1296
    assert bamio.bai_stats(GOLDEN_BAI) == dict(n_ref=4, n_no_coor=0)
    for tid, (n_bin, n_intv, n_mapped) in enumerate(((12, 9, 93250), (15, 11, 107279), (4, 2, 13006), (2, 1, 6494))):
        assert bamio.bai_stats(GOLDEN_BAI, tid) == dict(n_ref=4, n_no_coor=0, n_mapped=n_mapped, n_unmapped=0, n_bin=n_bin, n_intv=n_intv), tid
    model = ba.parse_bai(open(GOLDEN_BAI, "rb").read())
    assert [(r["n_bin"], len(r["ioffset"]), r["meta"][2]) for r in model["refs"]] == [(12, 9, 93250), (15, 11, 107279), (4, 2, 13006), (2, 1, 6494)]


def sweep(n_intv):
    """every window edge, beg beyond n_intv, empty and inverted ranges, a whole reference"""
    out = []
    for w in range(n_intv + 2):
        e = w << 14
        out += [(e, e + 1), (max(e - 1, 0), e), (max(e - 1, 0), e + 1), (e, e + 16384), (e + 100, e + 40000)]
    out += [((n_intv + 5) << 14, (n_intv + 6) << 14), (5000, 5000), (6000, 5000), (0, 1 << 29), (0, 1 << 40), (-5, 10), (0, 1)]
    return out


def test_query_equals_the_python_plan_on_the_reference_file(bamio, ffi):
    model = ba.parse_bai(open(GOLDEN_BAI, "rb").read())
    n = 0
    for tid in range(4):
        for beg, end in sweep(len(model["refs"][tid]["ioffset"])):
            got = bamio.bai_query(GOLDEN_BAI, tid, beg, end)
            assert got == ba.query(model, tid, beg, end), (tid, beg, end)
            n += len(got)
    assert n > 100 and bamio.bai_query(GOLDEN_BAI, 0, 5000, 5000) == [] and bamio.bai_query(GOLDEN_BAI, 0, 11 << 14, 12 << 14) != []
    for tid in (-1, 4):
        with pytest.raises(ffi.SlxError) as e:
            bamio.bai_query(GOLDEN_BAI, tid, 0, 100)
        assert e.value.code == ffi.SLX_EINVAL
    with pytest.raises(ffi.SlxError) as e:
        bamio.bai_query(os.path.join(ROOT, "tests", "golden", "missing.bai"), 0, 0, 100)
    assert e.value.code == ffi.SLX_EIO and "cannot open" in str(e.value)


def test_every_truncation_is_refused(bamio, ffi, tmp_path):
    """cut at every length from 0 to 1 295: SLX_EIO, or a clean load where only the optional trailing n_no_coor is missing (1 288 bytes)"""
    raw = open(GOLDEN_BAI, "rb").read()
    p = tmp_path / "cut.bai"
    clean = []
    for n in range(len(raw)):
        p.write_bytes(raw[:n])
        try:
            st = bamio.bai_stats(p, 3)
            clean.append(n)
            assert st == dict(n_ref=4, n_no_coor=0, n_mapped=6494, n_unmapped=0, n_bin=2, n_intv=1)
        except ffi.SlxError as e:
            assert e.code == ffi.SLX_EIO and "cut.bai" in str(e), n
    assert clean == [len(raw) - 8]
    # wild counts: each count of the file in turn set far beyond the bytes left
    for at in (4, 8, 16):
        p.write_bytes(raw[:at] + b"\xff\xff\xff\x7f" + raw[at + 4:])
        with pytest.raises(ffi.SlxError) as e:
            bamio.bai_query(p, 0, 0, 100)
        assert e.value.code == ffi.SLX_EIO, at


def test_host_parser_under_asan_ubsan(tmp_path):
    """tests/cpp/san_bai_test.cpp: every cut parsed from an exactly sized heap copy, then a sweep of queries"""
    from tests.test_sanitizers import ENV, SAN
    exe = str(tmp_path / "san_bai")
    c = os.path.join(ROOT, "seqlib_amd", "csrc")
    subprocess.check_call(["g++", "-std=c++17"] + SAN + ["-I" + os.path.join(ROOT, "include"), "-I" + c, os.path.join(c, "slx_index.cpp"), os.path.join(c, "slx_bai.cpp"),
                           os.path.join(ROOT, "tests", "cpp", "san_bai_test.cpp"), "-o", exe])
    r = subprocess.run([exe, GOLDEN_BAI], capture_output=True, text=True, env=ENV, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "runtime error" not in r.stderr and "AddressSanitizer" not in r.stderr, r.stderr
    w = r.stdout.split()
    assert w[:6] == ["cuts", "1297", "eio", "1295", "clean", "2"] and int(w[7]) > 0, r.stdout


def test_query_on_the_sorted_fixture_covers_the_brute_force_filter(bamio, tmp_path):
    """the Python writer's index of the sorted fixture through the library's parser: same plan as the model's, and every record the brute-force filter
    serves begins inside one of the plan's chunks"""
    raw = ba.sorted_bam()
    bai = ba.build_bai(raw)
    p = tmp_path / "s.bam.bai"
    p.write_bytes(bai)
    model = ba.parse_bai(bai)
    _, refs, recs = bu.parse_bam(raw)
    assert refs == ba.REFS and 2000 <= len(recs) <= 4000
    assert bamio.bai_stats(p, 2) == dict(n_ref=4, n_no_coor=sum(r["refid"] < 0 for r in recs), n_mapped=0, n_unmapped=0, n_bin=0, n_intv=0)
    assert bamio.bai_stats(p, 1)["n_unmapped"] == 1
    vmap, off = ba.VoffMap(bu.scan_members(raw)[0]), ba.record_offsets(raw, recs)
    for tid, beg, end in [(0, 0, 1), (0, 16383, 16384), (0, 16384, 16385), (0, 60000, 60001), (0, ba.N_POS + 30, ba.N_POS + 100030), (1, 70000, 70001), (2, 0, 50000), (3, 0, 100001),
                          (0, 0, 200000), (1, 140000, 150000), (3, 1 << 20, 1 << 21)]:
        got = bamio.bai_query(p, tid, beg, end)
        assert got == ba.query(model, tid, beg, end), (tid, beg, end)
        for i, r in enumerate(recs):
            if r["refid"] == tid and r["pos"] < end and ba.rec_end(r) > beg:
                assert any(u <= vmap(off[i]) < v for u, v in got), (tid, beg, end, i)


def test_fixture_holds_its_edge_cases():
    """what the GPU tests rely on the generated file to contain"""
    raw = ba.sorted_bam()
    _, _, recs = bu.parse_bam(raw)
    by = {r["name"]: r for r in recs}
    assert by["at_zero"]["pos"] == 0 and ba.rec_end(by["ends_16384"]) == 16384
    n = by["long_n"]
    assert bu.reg2bin(n["pos"], ba.rec_end(n)) < 4681 - 512 and ((ba.rec_end(n) - 1) >> 14) - (n["pos"] >> 14) >= 6
    assert by["no_cigar"]["n_cigar"] == 0 and not by["no_cigar"]["flag"] & 4 and ba.rec_end(by["no_cigar"]) == by["no_cigar"]["pos"] + 1
    assert by["unmapped_placed"]["flag"] & 4 and by["unmapped_placed"]["refid"] == 1 and ba.rec_end(by["unmapped_placed"]) == by["unmapped_placed"]["pos"] + 1
    assert by["cig300"]["n_cigar"] == 300 and ba.rec_end(by["cig300"]) == by["cig300"]["pos"] + 150
    assert not any(r["refid"] == 2 for r in recs) and recs[-1]["refid"] == -1
    # the record "pad" ends exactly where a member ends: its end's virtual offset is the next member's first byte
    members = bu.scan_members(raw)[0]
    vmap, off = ba.VoffMap(members), ba.record_offsets(raw, recs)
    k = [r["name"] for r in recs].index("pad")
    assert vmap(off[k + 1]) & 0xffff == 0 and (vmap(off[k + 1]) >> 16) in [m[0] for m in members]
    assert len(members) > 40 and any(vmap(o) >> 16 != vmap(o2 - 1) >> 16 for o, o2 in zip(off, off[1:]))          # records straddle members
    with pytest.raises(ba.Unsorted) as e:
        ba.build_bai(bu.bam_bytes(bu.TEXT, bu.REFS, bu.sample_records(50)))
    assert e.value.ordinal >= 1


def test_device_record_bodies_on_the_host(tmp_path):
    """dev_bai.h compiled for the host under ASan + UBSan: tid, pos, end and bin of every record of the sorted fixture equal the Python statement's, the
    strided sum of the cooperative CIGAR walk equals the plain one, and a record whose n_cigar_op passes its block_size is refused without a read past it"""
    import struct
    from tests.test_sanitizers import ENV, SAN
    exe = str(tmp_path / "bai_fields")
    subprocess.check_call(["g++", "-std=c++17"] + SAN + ["-I" + os.path.join(ROOT, "seqlib_amd", "csrc"), os.path.join(ROOT, "tests", "cpp", "bai_fields_test.cpp"), "-o", exe])
    recs = bu.parse_bam(ba.sorted_bam())[2]
    wild = bytearray(recs[10]["raw"])
    struct.pack_into("<H", wild, 16, 0xffff)                 # n_cigar_op far beyond the record
    p = tmp_path / "records.bin"
    p.write_bytes(b"".join(r["raw"] for r in recs) + bytes(wild))
    r = subprocess.run([exe, str(p)], capture_output=True, text=True, env=ENV, timeout=300)
    assert r.returncode == 0 and "runtime error" not in r.stderr and "AddressSanitizer" not in r.stderr, r.stdout[-500:] + r.stderr[-3000:]
    got = [tuple(int(x) for x in ln.split()) for ln in r.stdout.strip().splitlines()]
    want = [(x["refid"], x["pos"], ba.rec_end(x), bu.reg2bin(max(x["pos"], 0), max(ba.rec_end(x), max(x["pos"], 0) + 1)), 1) for x in recs]
    assert got[:-1] == want and got[-1][4] == 0 and got[-1][2] == recs[10]["pos"] + 1
