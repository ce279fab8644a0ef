"""SeqLib::BamMerger (Next, NextBatch, MergeTo, Header) and BamWriter::SortByCoordinate(spill_prefix) through the C++ headers on the GPU
(tests/cpp/bam_merge_test.cpp, compiled -Wall -Werror as tests/test_cpp_sort.py compiles its program); the files it writes are held against Python's answer."""
import glob
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def compile_program(tmp_path, extra=()):
    exe, lib = str(tmp_path / "bam_merge_test"), os.path.join(ROOT, "seqlib_amd")
    subprocess.check_call(["g++", "-std=c++17", "-O2", "-Wall", "-Werror", "-I" + os.path.join(ROOT, "include"), os.path.join(ROOT, "tests", "cpp", "bam_merge_test.cpp"), "-o", exe,
                           "-L" + lib, "-lseqlib_amd", "-Wl,-rpath," + lib, "-lz", "-lpthread"] + list(extra))
    return exe


@pytest.mark.gpu
def test_cpp_merger_and_spilling_writer(tmp_path):
    import __graft_entry__ as g
    if not os.path.exists(os.path.join(ROOT, "seqlib_amd", "libseqlib_amd.so")):
        g.build()
    from tests import bai_util as ba
    from tests import bam_util as bu
    from tests import merge_util as mu
    k = 3
    inputs = mu.build_inputs(k, block_in=k - 1)
    for i, recs in enumerate(inputs):
        (tmp_path / ("in_%02d.bam" % i)).write_bytes(bu.bam_bytes(bu.TEXT, bu.REFS, recs, member_size=0x2000))
    unsorted = mu.base_records()
    (tmp_path / "unsorted.bam").write_bytes(bu.bam_bytes(bu.TEXT, bu.REFS, unsorted, member_size=0x2000))
    exe = compile_program(tmp_path)
    r = subprocess.run([exe, str(tmp_path), str(k)], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0 and r.stdout.startswith("merge OK"), r.stdout[-2000:] + r.stderr[-2000:]
    want, frm = mu.expected_merge(inputs)
    assert int(r.stdout.split()[2]) == len(want) and int(r.stdout.split()[3]) >= 2
    # Next(): every record, in Python's order, from the input Python says
    names = [ln.split() for ln in (tmp_path / "next.txt").read_text().splitlines()]
    assert names == [[rec[36:36 + rec[12] - 1].decode(), str(i)] for rec, i in zip(want, frm)]          # (l_read_name at byte 12, the name from byte 36)
    # MergeTo: header and records byte for byte
    assert bu.inflate_all((tmp_path / "merged.bam").read_bytes()) == bu.bam_header(mu.header_rule([bu.TEXT] * k), bu.REFS) + b"".join(want)
    # the spilling writer wrote the file the writer that held everything wrote, and its index is one the Python parser reads
    raw = (tmp_path / "spilled.bam").read_bytes()
    assert raw == (tmp_path / "in_hbm.bam").read_bytes()
    assert (tmp_path / "spilled.bam.bai").read_bytes() == ba.build_bai(raw)
    _, _, recs = bu.parse_bam(raw)
    assert [(x["refid"] & 0xffffffff, x["pos"]) for x in recs] == [mu.key(x) for x in sorted(unsorted, key=mu.key)]
    assert [x["name"] for x in recs if (x["refid"], x["pos"]) == mu.TIE_AT] == ["tie%03d" % i for i in range(mu.N_TIES)]          # stable over the runs
    assert not glob.glob(str(tmp_path / "*.run*.bam")) and not (tmp_path / "refused.bam").exists() and not (tmp_path / "nothing.bam").exists()
    # the refusals said why
    for words in ("does not combine with SortByCoordinate(spill_prefix)", "call UseGpu() first", "an empty spill prefix", "no input; AddFile() first", "is an input: the output must be another file",
                  "the merge has begun", "no open sorting writer"):
        assert words in r.stderr, words


def test_cpp_merge_headers_compile_without_the_library(tmp_path):
    """headers only: BamMerger.h and BamWriter.h with the spill entry points compile clean under -Wall -Werror"""
    src = tmp_path / "use.cpp"
    src.write_text('#include "SeqLib/BamMerger.h"\n#include "SeqLib/BamWriter.h"\nint main() { SeqLib::BamMerger m; SeqLib::BamWriter w; return (int)m.NumFiles() + (w.SortByCoordinate("x") ? 1 : 0); }\n')
    subprocess.check_call(["g++", "-std=c++17", "-Wall", "-Werror", "-fsyntax-only", "-I" + os.path.join(ROOT, "include"), str(src)])
