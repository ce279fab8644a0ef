"""SeqLib::Filter (include/SeqLib/ReadFilter.h) and the BamRecord accessors its rules call, through tests/cpp/read_filter_test.cpp: isValid record by record on
the host against the masks of the Python statement (tests/filter_util.py), the accessors against its values, the JSON entry points that are not declared, and
-- on the GPU -- BamReader::SetReadFilter + NextBatch."""
import os
import struct
import subprocess

import pytest

from tests import bam_util as bu
from tests import filter_util as fu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SETS = ("everything", "excluder", "regions_mate", "orient_rf_or_rr", "motif_links")          # the order of read_filter_test.cpp's collections; then no filter at all


def build_lib():
    import __graft_entry__ as g
    if not os.path.exists(os.path.join(ROOT, "seqlib_amd", "libseqlib_amd.so")):
        g.build()


def compile_test(tmp):
    out = str(tmp / "read_filter_test")
    lib = os.path.join(ROOT, "seqlib_amd")
    subprocess.check_call(["g++", "-std=c++17", "-O2", "-Wall", "-Werror", "-I" + os.path.join(ROOT, "include"), os.path.join(ROOT, "tests", "cpp", "read_filter_test.cpp"), "-o", out,
                           "-L" + lib, "-lseqlib_amd", "-Wl,-rpath," + lib, "-Wl,-rpath,/opt/rocm/lib", "-lz", "-lpthread"])
    return out


def write_inputs(tmp):
    recs = fu.records()
    parsed = fu.parsed(recs)
    masks = fu.coverage(parsed)
    (tmp / "recs.bin").write_bytes(struct.pack("<I", len(recs)) + b"".join(recs))
    (tmp / "motifs.txt").write_text("".join(m + "\n" for m in fu.RULE_SETS["motif_links"][0]["rules"][0]["motifs"]))
    lines = []
    for i, p in enumerate(parsed):
        f = fu.features(p)
        bits = "".join("1" if masks[s][i] else "0" for s in SETS) + "1"
        lines.append("%s %d %d %d %d %d %d %d %d %d rg=%s" % (bits, f["full_insert_size"], f["pair_orientation"], f["interchromosomal"], f["pair_mapped"], f["num_clip"],
                                                             f["num_hard_clip"], f["max_ins"], f["max_del"], f["n_bases_n"], f["read_group"]))
    (tmp / "expect.txt").write_text("\n".join(lines) + "\n")
    return recs


def test_cpp_read_filter_on_the_host(tmp_path):
    build_lib()
    write_inputs(tmp_path)
    r = subprocess.run([compile_test(tmp_path), str(tmp_path)], capture_output=True, text=True)
    assert r.returncode == 0 and r.stdout.startswith("read_filter OK"), r.stdout[-2000:] + r.stderr[-2000:]
    assert int(r.stdout.split()[2]) > 780


def test_json_entry_points_are_not_declared(tmp_path):
    """jsoncpp is not in the tree: a use of the JSON constructor, addGlobalRule or parseJson does not compile (no stub that parses nothing)"""
    inc = "-I" + os.path.join(ROOT, "include")
    head = '#include "SeqLib/ReadFilter.h"\n#include "SeqLib/BamHeader.h"\nusing namespace SeqLib::Filter;\n'
    src = tmp_path / "use.cpp"
    for body in ('ReadFilterCollection c(std::string("{}"), SeqLib::BamHeader());', 'ReadFilterCollection c; c.addGlobalRule("{}");', 'Range r; r.parseJson(0, "mapq");',
                 'AbstractRule a; a.parseJson(0);', 'FlagRule f; f.parseJson(0);'):
        src.write_text(head + "int main() { %s return 0; }\n" % body)
        r = subprocess.run(["g++", "-std=c++17", "-fsyntax-only", inc, str(src)], capture_output=True, text=True)
        assert r.returncode != 0 and ("no member named" in r.stderr.replace("has no member named", "no member named") or "no matching function" in r.stderr), body
    src.write_text(head + "int main() { ReadFilterCollection c; ReadFilter f; AbstractRule a; a.mapq = Range(1, 2, false); f.AddRule(a); c.AddReadFilter(f); return (int)c.size() - 1; }\n")
    assert subprocess.run(["g++", "-std=c++17", "-fsyntax-only", inc, str(src)]).returncode == 0


@pytest.mark.gpu
def test_cpp_set_read_filter_on_the_gpu(tmp_path):
    build_lib()
    recs = write_inputs(tmp_path)
    bam = tmp_path / "f.bam"
    bam.write_bytes(bu.bam_bytes(bu.TEXT, bu.REFS, recs, member_size=0x1800))
    r = subprocess.run([compile_test(tmp_path), str(tmp_path), str(bam)], capture_output=True, text=True)
    assert r.returncode == 0 and r.stdout.startswith("read_filter OK"), r.stdout[-2000:] + r.stderr[-2000:]
