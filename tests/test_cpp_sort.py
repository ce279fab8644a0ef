"""BamWriter::SortByCoordinate, alignToBam into a sorting writer and the BamRecordSort functors through the C++ headers on the GPU
(tests/cpp/bam_sort_test.cpp, compiled -Wall -Werror as tests/test_cpp_region.py compiles its programs)."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")


@pytest.mark.gpu
def test_cpp_sort_by_coordinate(tmp_path):
    import __graft_entry__ as g
    if not os.path.exists(os.path.join(ROOT, "seqlib_amd", "libseqlib_amd.so")):
        g.build()
    exe, lib = str(tmp_path / "bam_sort_test"), os.path.join(ROOT, "seqlib_amd")
    subprocess.check_call(["g++", "-std=c++17", "-O2", "-Wall", "-Werror", "-I" + os.path.join(ROOT, "include"), os.path.join(ROOT, "tests", "cpp", "bam_sort_test.cpp"), "-o", exe,
                           "-L" + lib, "-lseqlib_amd", "-Wl,-rpath," + lib, "-lz", "-lpthread"])
    r = subprocess.run([exe, os.path.join(GOLDEN, "tiny.fa"), os.path.join(GOLDEN, "sim1_bcr.head3000.fq"), "3000", str(tmp_path)], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0 and r.stdout.startswith("sort OK"), r.stdout[-2000:] + r.stderr[-2000:]
    assert int(r.stdout.split()[2]) >= 3000 and int(r.stdout.split()[3]) > 0
    # the refusals said why
    for words in ("only BAM output is sorted on the GPU", "call UseGpu() first", "SortByCoordinate - call it before Open()", "use WriteDevice(d, n, d_rec_off, n_records)"):
        assert words in r.stderr, words
    # the index the sorting writer's file got is one the Python parser reads
    from tests import bai_util as ba
    from tests import bam_util as bu
    raw = (tmp_path / "sorted.bam").read_bytes()
    assert (tmp_path / "sorted.bam.bai").read_bytes() == ba.build_bai(raw)
    assert bu.inflate_all(raw) == bu.inflate_all((tmp_path / "host_sorted.bam").read_bytes())


def test_cpp_sort_headers_compile_without_the_library(tmp_path):
    """headers only: BamRecordSort needs nothing of the library, and BamWriter.h with the sort entry points compiles clean under -Wall -Werror"""
    src = tmp_path / "use.cpp"
    src.write_text('#include <algorithm>\n#include "SeqLib/BamWriter.h"\nint main() { SeqLib::BamRecordVector v; std::sort(v.begin(), v.end(), SeqLib::BamRecordSort::ByReadPosition()); '
                   'std::sort(v.begin(), v.end(), SeqLib::BamRecordSort::ByMatePosition()); return (int)v.size(); }\n')
    subprocess.check_call(["g++", "-std=c++17", "-Wall", "-Werror", "-fsyntax-only", "-I" + os.path.join(ROOT, "include"), str(src)])
