"""SeqLib::GenomicRegion / GRC (include/SeqLib/GenomicRegion.h, GenomicRegionCollection.h) on the CPU, and region iteration through the C++ classes on the
GPU (tests/cpp/bam_region_test.cpp): BamWriter::BuildIndex, BamReader::Open finding the index, SetRegions / SetRegion, Next and NextBatch."""
import os
import subprocess

import pytest

from tests import bai_util as ba

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def compile_test(tmp, name, link):
    out = str(tmp / name)
    lib = os.path.join(ROOT, "seqlib_amd")
    cmd = ["g++", "-std=c++17", "-O2", "-Wall", "-Werror", "-I" + os.path.join(ROOT, "include"), os.path.join(ROOT, "tests", "cpp", name + ".cpp"), "-o", out]
    if link:
        cmd += ["-L" + lib, "-lseqlib_amd", "-Wl,-rpath," + lib, "-lz", "-lpthread"]
    subprocess.check_call(cmd)
    return out


def test_cpp_genomic_region(tmp_path):
    """headers only: the test program links nothing of the library"""
    r = subprocess.run([compile_test(tmp_path, "genomic_region_test", False)], capture_output=True, text=True)
    assert r.returncode == 0 and r.stdout.strip() == "genomic_region OK", r.stdout + r.stderr


def test_interval_tree_queries_are_not_declared(tmp_path):
    """the container side only: a use of the reference's interval-tree queries does not compile (no stub that answers nothing)"""
    for call in ("g.FindOverlaps(g, true)", "g.MergeOverlappingIntervals()", "g.CreateTreeMap()"):
        src = tmp_path / "use.cpp"
        src.write_text('#include "SeqLib/GenomicRegionCollection.h"\nint main() { SeqLib::GRC g; %s; return 0; }\n' % call)
        r = subprocess.run(["g++", "-std=c++17", "-fsyntax-only", "-I" + os.path.join(ROOT, "include"), str(src)], capture_output=True, text=True)
        assert r.returncode != 0 and "no member named" in r.stderr.replace("has no member named", "no member named"), call
    src.write_text('#include "SeqLib/GenomicRegionCollection.h"\nint main() { SeqLib::GRC g; g.add(SeqLib::GenomicRegion(0, 1, 2)); return (int)g.size() - 1; }\n')
    assert subprocess.run(["g++", "-std=c++17", "-fsyntax-only", "-I" + os.path.join(ROOT, "include"), str(src)]).returncode == 0


@pytest.mark.gpu
def test_cpp_region_iteration(tmp_path):
    import __graft_entry__ as g
    if not os.path.exists(os.path.join(ROOT, "seqlib_amd", "libseqlib_amd.so")):
        g.build()
    exe = compile_test(tmp_path, "bam_region_test", True)
    r = subprocess.run([exe, str(tmp_path)], capture_output=True, text=True)
    assert r.returncode == 0 and r.stdout.startswith("region OK"), r.stdout[-2000:] + r.stderr[-2000:]
    assert int(r.stdout.split()[2]) > 300 and int(r.stdout.split()[3]) > 0
    assert r.stderr.count("Failed to create index") == 2 and "not coordinate-sorted" in r.stderr and "Trying to make index, but no BAM specified" in r.stderr
    # the index the class wrote is one the Python parser reads, with the file's counts
    bai = ba.parse_bai((tmp_path / "sorted.bam.bai").read_bytes())
    assert [r["meta"][2] for r in bai["refs"]] == [1200, 1200, 1200] and bai["n_no_coor"] == 25
