"""SeqLib::DuplicateMarker and BamWriter::MarkDuplicates through the headers only (tests/cpp/dup_api_test.cpp): the program compiles with -Wall -Werror and
links; without a GPU the class refuses as it should; on the GPU BamReader -> DuplicateMarker, MarkFile and the chain Next() -> sorting, marking GPU BamWriter
-> Close() -> BuildIndex() are held against the Python statement of the rules (tests/dup_util.py).  slx_dup_file at the C-ABI is tested here too."""
import os
import random
import struct
import subprocess

import pytest

from tests import bam_util as bu
from tests import dup_util as du

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
REFS = [("chrA", 200000), ("chrB", 150000), ("chrC", 100001)]
TEXT = "@HD\tVN:1.6\tSO:unsorted\n" + "".join("@SQ\tSN:%s\tLN:%d\n" % r for r in REFS) + du.HEADER.split("\n", 2)[2]


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    import __graft_entry__ as g
    lib = os.path.join(ROOT, "seqlib_amd")
    if not os.path.exists(os.path.join(lib, "libseqlib_amd.so")):
        g.build()
    out = str(tmp_path_factory.mktemp("dupapi") / "dup_api_test")
    subprocess.check_call(["g++", "-std=c++17", "-O2", "-Wall", "-Werror", "-I" + os.path.join(ROOT, "include"), os.path.join(ROOT, "tests", "cpp", "dup_api_test.cpp"), "-o", out,
                           "-L" + lib, "-lseqlib_amd", "-Wl,-rpath," + lib, "-lz", "-lpthread"])
    return out


@pytest.fixture(scope="module")
def case(tmp_path_factory):
    """a shuffled, unsorted BAM with read groups of two libraries, pairs, orphans, fragments and ignored records"""
    from tests.test_gpu_dup import pair_cases
    recs = pair_cases() + du.bulk(700, seed=12)
    random.Random(6).shuffle(recs)
    d = tmp_path_factory.mktemp("dupbam")
    (d / "in.bam").write_bytes(bu.bam_bytes(TEXT, REFS, recs, member_size=3000))
    return d, recs, du.mark([recs], TEXT)


def test_the_class_without_a_gpu(exe):
    r = subprocess.run([exe, "host"], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and r.stdout.startswith("dup api host OK "), r.stdout[-2000:] + r.stderr[-2000:]


def same_but_for_the_flags(got, recs, want):
    assert [g["raw"] for g in got] == [du.marked(r, v) for r, v in zip(recs, want)]


@pytest.mark.gpu
def test_file_route(sl, case):
    from seqlib_amd import _ffi, dupio
    d, recs, (want, counters) = case
    m = dupio.Marker()
    m.mark_file(d / "in.bam", d / "out.bam", batch_bytes=4096)          # mates fall into different batches
    assert m.flags() == want and m.counter("duplicates") == counters["duplicates"] > 0 and m.counter("libraries") == 4
    m.close()
    raw = (d / "out.bam").read_bytes()
    text, refs, got = bu.parse_bam(raw)
    assert (text, refs) == (TEXT.rstrip("\0"), REFS) and bu.scan_members(raw)[1]
    same_but_for_the_flags(got, recs, want)
    dupio.mark_file(d / "in.bam", d / "out2.bam")
    assert bu.inflate_all((d / "out2.bam").read_bytes()) == bu.inflate_all(raw)
    (d / "cut.bam").write_bytes((d / "in.bam").read_bytes()[:-300])
    for src, dst in ((d / "cut.bam", d / "none.bam"), (d / "missing.bam", d / "none.bam")):
        with pytest.raises(_ffi.SlxError):
            dupio.mark_file(src, dst)
        assert not (d / "none.bam").exists()          # no output file is left behind
    with pytest.raises(_ffi.SlxError) as e:
        dupio.mark_file(d / "in.bam", d / "in.bam")
    assert e.value.code == _ffi.SLX_EINVAL


@pytest.mark.gpu
def test_duplicate_marker_and_marking_writer(exe, sl, case):
    d, recs, (want, counters) = case
    r = subprocess.run([exe, "chain", str(d / "in.bam"), str(d)], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and r.stdout == "dup api chain OK %d %d %d\n" % (len(recs), counters["duplicates"], counters["pairs"]), r.stdout[-2000:] + r.stderr[-3000:]
    assert [int(x) for x in (d / "flags.txt").read_text().split()] == [1 if v == du.DUP else 0 for v in want]
    same_but_for_the_flags(bu.parse_bam((d / "marked.bam").read_bytes())[2], recs, want)
    order = sorted(range(len(recs)), key=lambda i: (struct.unpack_from("<i", recs[i], 4)[0] & 0xffffffff, struct.unpack_from("<i", recs[i], 8)[0]))
    text, refs, got = bu.parse_bam((d / "sorted.bam").read_bytes())
    assert "SO:coordinate" in text and refs == REFS and len(got) == len(recs)
    # the writer computes the bin itself: everything but the bin is the input's, with the marks
    strip = lambda raw: raw[:14] + raw[16:]
    assert [strip(g["raw"]) for g in got] == [strip(du.marked(recs[i], want[i])) for i in order]
    assert (d / "sorted.bam.bai").exists() or (d / "sorted.bai").exists()
