"""SeqLib::GenomicRegionCollection (include/SeqLib/GenomicRegionCollection.h) through tests/cpp/grc_api_test.cpp on the CPU: the reference's own test shapes
(seq_test.cpp `merge`, `interval_queries` part 1), the host-only members, ReadBED / ReadVCF, the single queries on a host-only index, the exceptions, and a
program of the container members alone that links nothing.  The collection join runs in tests/test_gpu_grc.py."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    out = str(tmp_path_factory.mktemp("grcapi") / "grc_api_test")
    lib = os.path.join(ROOT, "seqlib_amd")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-Werror", "-DSEQLIB_GRC_QUERIES", "-I" + os.path.join(ROOT, "include"), os.path.join(ROOT, "tests", "cpp", "grc_api_test.cpp"), "-o", out,
                           "-L" + lib, "-lseqlib_amd", "-Wl,-rpath," + lib, "-Wl,-rpath,/opt/rocm/lib", "-lz", "-lpthread"])
    return out


def test_the_reference_surface_on_the_host(exe, tmp_path):
    r = subprocess.run([exe, "host", str(tmp_path)], capture_output=True, text=True)
    assert r.returncode == 0 and "grc_api_test host OK" in r.stdout, r.stdout[-2000:] + r.stderr[-3000:]
    assert "Need to run this->CreateTreeMap()" in r.stderr          # CountOverlaps before CreateTreeMap warns, as the reference does


def test_collection_join_without_a_gpu_is_a_runtime_error(exe):
    import torch
    if torch.cuda.is_available():
        pytest.skip("a GPU is present: tests/test_gpu_grc.py runs the join")
    r = subprocess.run([exe, "nogpu"], capture_output=True, text=True)
    assert r.returncode == 0 and "grc_api_test nogpu OK" in r.stdout, r.stdout[-2000:] + r.stderr[-3000:]


def test_container_only_program_links_without_the_library(tmp_path):
    """without SEQLIB_GRC_QUERIES: the container and the members that need no library, from the headers alone"""
    src = tmp_path / "use.cpp"
    src.write_text('#include "SeqLib/GenomicRegionCollection.h"\n'
                   'int main() { SeqLib::GRC g; g.add(SeqLib::GenomicRegion(0, 1, 2)); SeqLib::GRC h(g.AsGenomicRegionVector()); SeqLib::GRC k(g[0]);\n'
                   '  for (const auto &x : h) if (x.pos1 != 1) return 2;\n'
                   '  h.clear(); h.Concat(g); h.Pad(1); h.CoordinateSort(); h.clear(); return (int)(g.size() + k.size() + h.size() + (g.IsEmpty() ? 5 : 0) + (size_t)(g.at(0).pos2 - 2)) - 2; }\n')
    out = str(tmp_path / "use")
    subprocess.check_call(["g++", "-std=c++17", "-O2", "-Wall", "-Werror", "-I" + os.path.join(ROOT, "include"), str(src), "-o", out])
    assert subprocess.run([out]).returncode == 0


def test_the_interval_queries_are_declared(tmp_path):
    """with SEQLIB_GRC_QUERIES defined: every call of the reference's surface; without it the header stays what needs no library (tests/test_cpp_region.py)"""
    calls = ["g.CreateTreeMap()", "g.FindOverlaps(r, true)", "g.FindOverlapWidth(r, true)", "g.FindOverlappedIntervals(r, true)", "g.CountOverlaps(r)", "g.CountContained(r)",
             "g.OverlapSameInterval(r, r)", "g.MergeOverlappingIntervals()", "g.Intersection(g, true)", "g.FindOverlaps(g, q, q, true)", "g.Concat(g)", "g.CoordinateSort()",
             "g.SortAndStretchLeft(0)", "g.SortAndStretchRight(0)", "g.Shuffle()", "g.Pad(1)", "g.TotalWidth()", "g.NumTree()", "g.Rewind()", "g.AsBEDString(h)", "g.ReadBED(\"x\", h)",
             "g.ReadVCF(\"x\", h)", "g.empty()", "std::cout << g"]
    src = tmp_path / "all.cpp"
    src.write_text('#include "SeqLib/GenomicRegionCollection.h"\nint main() { SeqLib::GRC g; SeqLib::GenomicRegion r(0, 1, 2); SeqLib::BamHeader h; std::vector<int32_t> q;\n'
                   + "".join("  (void)(%s);\n" % c for c in calls) + "  return 0; }\n")
    r = subprocess.run(["g++", "-std=c++17", "-fsyntax-only", "-Wall", "-Werror", "-DSEQLIB_GRC_QUERIES", "-I" + os.path.join(ROOT, "include"), str(src)], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]
