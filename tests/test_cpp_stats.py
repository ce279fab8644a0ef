"""SeqLib::BamStats through the headers only (tests/cpp/stats_api_test.cpp): the program compiles and links; without a GPU addRead works on the host and gives the
text of tests/stats_util.py while addReads and addBatch throw; on the GPU an addRead loop and addReads(BamReader&) over the same file print the same text, that of
stats_util, and addBatch runs on the records the builder behind alignToBam leaves in HBM for the golden reads."""
import os
import struct
import subprocess

import pytest

from tests import bam_util as bu
from tests import stats_util as su

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    import __graft_entry__ as g
    lib = os.path.join(ROOT, "seqlib_amd")
    if not os.path.exists(os.path.join(lib, "libseqlib_amd.so")):
        g.build()
    out = str(tmp_path_factory.mktemp("statsapi") / "stats_api_test")
    subprocess.check_call(["g++", "-std=c++17", "-O2", "-Wall", "-Werror", "-I" + os.path.join(ROOT, "include"), os.path.join(ROOT, "tests", "cpp", "stats_api_test.cpp"), "-o", out,
                           "-L" + lib, "-lseqlib_amd", "-Wl,-rpath," + lib, "-lz", "-lpthread"])
    return out


def text_of(recs):
    return su.text(su.accumulate([su.parse(r) for r in recs]))


def test_cpp_mirror_links_and_throws_without_a_gpu(exe):
    r = subprocess.run([exe, "errors"], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and r.stdout.startswith("stats api errors OK"), r.stdout[-2000:] + r.stderr[-2000:]


def test_add_read_on_the_host(exe, tmp_path):
    """no GPU: BamStats::addRead record by record, Groups, Group, Merge and clear; the text is stats_util's"""
    recs = su.GOOD + [r for r in su.bulk() if len(r) < 3000]
    p = tmp_path / "recs.bin"
    p.write_bytes(struct.pack("<I", len(recs)) + b"".join(recs))
    r = subprocess.run([exe, "host", str(p)], capture_output=True, timeout=120)
    assert r.returncode == 0 and r.stdout == text_of(recs), r.stdout[-2000:] + r.stderr[-2000:]


@pytest.mark.gpu
def test_cpp_mirror_on_the_gpu(exe, tmp_path):
    recs = su.GOOD + [r for r in su.bulk() if len(r) < 3000]
    bam = tmp_path / "cases.bam"
    bam.write_bytes(bu.bam_bytes(bu.TEXT, bu.REFS, recs, member_size=3000))
    r = subprocess.run([exe, "run", str(bam)], capture_output=True, timeout=300)
    assert r.returncode == 0 and r.stdout == text_of(recs), r.stdout[-2000:] + r.stderr[-3000:]


@pytest.mark.gpu
def test_add_batch_on_the_builders_records(exe, tmp_path):
    out = tmp_path / "built.bin"
    r = subprocess.run([exe, "builder", os.path.join(GOLDEN, "tiny.fa"), os.path.join(GOLDEN, "sim1_bcr.head3000.fq"), str(out)], capture_output=True, timeout=300)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-3000:]
    raw = out.read_bytes()
    n, at, recs = struct.unpack_from("<I", raw)[0], 4, []
    for _ in range(n):
        bs = struct.unpack_from("<I", raw, at)[0]
        recs.append(raw[at:at + 4 + bs])
        at += 4 + bs
    assert n >= 500 and at == len(raw)
    assert r.stdout == text_of(recs) and r.stdout.count(b"\n") >= 2
