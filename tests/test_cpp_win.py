"""SeqLib::AssemblyWindows, FermiAssembler::AssembleRegions and BamRecord::QualityTrimmedSequence through the headers only (tests/cpp/win_api_test.cpp): the
program compiles with -Wall -Werror and links; without a GPU QualityTrimmedSequence gives the reference's pairs for the trim profiles and a host-only collector
refuses as it should; on the GPU BamReader -> AssemblyWindows -> Assemble and AssembleRegions are compared read for read and contig for contig with the loop
Next() + overlap test + AddRead + AssembleWindows (whole file, SetRegions with records served twice), and with the Python statement of tests/win_util.py."""
import os
import random
import subprocess

import pytest

from tests import bam_util as bu
from tests import fml_util as fu
from tests import win_util as wu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
THRESHOLDS = (0, 4, 41, 93)
LENGTHS = (0, 1, 2, 63, 64, 65)


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    import __graft_entry__ as g
    lib = os.path.join(ROOT, "seqlib_amd")
    if not os.path.exists(os.path.join(lib, "libseqlib_amd.so")):
        g.build()
    out = str(tmp_path_factory.mktemp("winapi") / "win_api_test")
    subprocess.check_call(["g++", "-std=c++17", "-O2", "-Wall", "-Werror", "-I" + os.path.join(ROOT, "include"), os.path.join(ROOT, "tests", "cpp", "win_api_test.cpp"), "-o", out,
                           "-L" + lib, "-lseqlib_amd", "-Wl,-rpath," + lib, "-lz", "-lpthread"])
    return out


def test_quality_trimmed_sequence_without_a_gpu(exe, tmp_path):
    quals = []
    for t in THRESHOLDS:
        for n in LENGTHS:
            quals += [q for _, q in sorted(wu.profile_quals(n, t).items())]
    rng = random.Random(2)
    recs = [wu.record("q%d" % i, 0, 100, wu.rand_seq(rng, len(q)), q) for i, q in enumerate(quals)]
    (tmp_path / "in.bin").write_bytes(b"".join(recs))
    r = subprocess.run([exe, "host", str(tmp_path / "in.bin"), str(tmp_path / "out.txt")], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and r.stdout == "win api host OK %d\n" % len(recs), r.stdout[-2000:] + r.stderr[-2000:]
    got = [tuple(int(x) for x in line.split()) for line in (tmp_path / "out.txt").read_text().splitlines()]
    want = [(i, t) + wu.quality_trim(q, t) for i, q in enumerate(quals) for t in THRESHOLDS]
    assert got == want
    assert {(a == 0, e == -1) for _, _, a, e in want} == {(True, True), (False, True), (True, False), (False, False)}


@pytest.fixture(scope="module")
def myc_bam(tmp_path_factory):
    """the end-to-end case of tests/win_util.py as a sorted, indexed BAM over one contig"""
    from seqlib_amd import bamio
    myc = fu.fixture_genome()["myc"]
    recs = wu.e2e_records(myc)
    d = tmp_path_factory.mktemp("winbam")
    refs = [("myc", len(myc))]
    text = "@HD\tVN:1.6\tSO:coordinate\n@SQ\tSN:myc\tLN:%d\n" % len(myc)
    (d / "in.bam").write_bytes(bu.bam_bytes(text, refs, recs, member_size=16000))
    (d / "windows.txt").write_text("".join("%d %d %d\n" % w for w in wu.E2E_WINDOWS))
    bamio.index_build(d / "in.bam")
    return d, recs


def parse_out(text):
    wins = []
    for line in text.splitlines():
        f = line.split(" ")
        if f[0] == "W":
            wins.append(dict(n_reads=int(f[2]), n_contigs=int(f[3]), reads=[], contigs=[]))
        elif f[0] == "R":
            wins[-1]["reads"].append((int(f[1]), f[2].encode(), bytes.fromhex(f[3])))
        elif f[0] == "C":
            wins[-1]["contigs"].append(f[1])
    return wins


@pytest.mark.gpu
@pytest.mark.parametrize("how", ["all", "regions"])
def test_assembly_windows_equal_the_host_loop(exe, sl, myc_bam, how):
    d, recs = myc_bam
    out = d / ("out_%s.txt" % how)
    r = subprocess.run([exe, "asm", str(d / "in.bam"), str(d / "windows.txt"), how, str(out)], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and r.stdout.startswith("win api asm OK "), r.stdout[-2000:] + r.stderr[-3000:]
    n_records, n_reads, n_contigs = (int(x) for x in r.stdout.split()[-3:])
    wins = parse_out(out.read_text())
    assert len(wins) == 3 and all(w["n_reads"] == len(w["reads"]) and w["n_contigs"] == len(w["contigs"]) for w in wins)
    assert wins[0]["n_contigs"] >= 1 and wins[1]["n_contigs"] >= 1 and max(len(c) for c in wins[0]["contigs"]) > 3000
    if how == "all":
        want = wu.collect(wu.E2E_WINDOWS, [recs])
        assert n_records == len(recs) and n_reads == len(want[4]) and wins[2]["n_reads"] == 3
        for w in range(3):
            a, b = want[3][w], want[3][w + 1]
            assert wins[w]["reads"] == [(want[4][r], want[0][want[2][r]:want[2][r + 1]], want[1][want[2][r]:want[2][r + 1]]) for r in range(a, b)]
    else:
        assert n_records > len(recs) and all(len({o for o, _, _ in w["reads"]}) == len(w["reads"]) for w in wins)          # a record served twice has two ordinals
        assert len({(s, q) for _, s, q in wins[0]["reads"]}) < len(wins[0]["reads"])
