"""SeqLib::Pileup through the headers only (tests/cpp/pile_api_test.cpp): the program compiles and links without a GPU and its error cases run there; on the GPU an
addRead loop, addReads(BamReader&), the floors, a narrower window and Sites(RefGenome&) are held against tests/pile_util.py, and the file WriteSites leaves against
its text."""
import os
import subprocess

import pytest

from tests import bam_util as bu
from tests import pile_util as pu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FA = os.path.join(ROOT, "tests", "golden", "tiny.fa")


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    import __graft_entry__ as g
    lib = os.path.join(ROOT, "seqlib_amd")
    if not os.path.exists(os.path.join(lib, "libseqlib_amd.so")):
        g.build()
    out = str(tmp_path_factory.mktemp("pileapi") / "pile_api_test")
    subprocess.check_call(["g++", "-std=c++17", "-O2", "-Wall", "-Werror", "-I" + os.path.join(ROOT, "include"), os.path.join(ROOT, "tests", "cpp", "pile_api_test.cpp"), "-o", out,
                           "-L" + lib, "-lseqlib_amd", "-Wl,-rpath," + lib, "-lz", "-lpthread"])
    return out


def test_cpp_mirror_links_and_throws_without_a_gpu(exe):
    r = subprocess.run([exe, "errors"], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and r.stdout.startswith("pile api errors OK"), r.stdout[-2000:] + r.stderr[-2000:]


@pytest.mark.gpu
def test_cpp_mirror_on_the_gpu(exe, tmp_path):
    contigs = pu.fasta_contigs(FA)
    refs = [(n, len(s)) for n, s in contigs]
    tid, window, narrow = 2, (2, 900, 3200), (2, 1490, 1710)
    edits = {1500: ("X", 1, 0), 1600: ("X", 3, 0), 1700: ("I", 2, 3), 1800: ("D", 2, 3)}
    recs = pu.cut_reads(contigs[tid][1], tid, 1000, 3000, 7, 120, edits) + [r for r in pu.random_records(500, seed=12, span=4000, tid=tid) if 0 <= pu.parse(r)[0] < 4]
    recs.sort(key=lambda r: pu.parse(r)[:2])
    text = "@HD\tVN:1.6\tSO:coordinate\n" + "".join("@SQ\tSN:%s\tLN:%d\n" % r for r in refs)
    bam = tmp_path / "reads.bam"
    bam.write_bytes(bu.bam_bytes(text, refs, recs, member_size=3000))
    want = pu.planes(recs, window, refs)
    floors = pu.planes(recs, window, refs, min_baseq=20, min_mapq=30)
    q = (10, 3, 1, 5)
    sites = pu.sites(want, window[1], contigs[tid][1], *q)
    assert {1500, 1600, 1700, 1800, 1801, 1802} <= {s[0] for s in sites} and (floors != want).any()
    E = {"n_records": [len(recs)], "window": list(window), "narrow": list(narrow[1:]), "at": [1700], "site_params": list(q),
         "planes": want.reshape(-1).tolist(), "planes_floors": floors.reshape(-1).tolist(), "planes_narrow": pu.planes(recs, narrow, refs).reshape(-1).tolist(),
         "sites": [v for s in sites for v in s[:5]]}
    exp = tmp_path / "expect.txt"
    exp.write_text("".join("%s %d %s\n" % (k, len(v), " ".join(map(str, v))) for k, v in E.items()))
    r = subprocess.run([exe, "run", str(bam), FA, str(exp), str(tmp_path)], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and r.stdout.endswith("pile api OK\n"), r.stdout[-2000:] + r.stderr[-3000:]
    assert (tmp_path / "sites.tsv").read_bytes() == pu.tsv(sites, refs[tid][0])
