"""FastqReader::NextBatch and the FastqReader overloads of BWAAligner, through the C++ headers as a SeqLib user compiles them (tests/cpp/fastq_batch_test.cpp)."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BATCHES = ("0", "70000")          # the default (one batch) and several batches


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    import __graft_entry__ as g
    if not os.path.exists(os.path.join(ROOT, "seqlib_amd", "libseqlib_amd.so")):
        g.build()
    out = str(tmp_path_factory.mktemp("cpp") / "fastq_batch_test")
    lib = os.path.join(ROOT, "seqlib_amd")
    subprocess.check_call(["g++", "-std=c++17", "-O2", "-Wall", "-I" + os.path.join(ROOT, "include"), os.path.join(ROOT, "tests", "cpp", "fastq_batch_test.cpp"), "-o", out,
                           "-L" + lib, "-lseqlib_amd", "-Wl,-rpath," + lib, "-lz", "-lpthread"])
    return out


def test_per_read_program_needs_no_library(tmp_path):
    """a program that calls only Open and GetNextSequence compiles and links with zlib alone: the batch entry names library symbols only where it is used"""
    src = tmp_path / "per_read.cpp"
    src.write_text('#include "SeqLib/FastqReader.h"\n'
                   "int main(int argc, char **argv) { SeqLib::FastqReader r; SeqLib::UnalignedSequence s; int n = 0;\n"
                   "  if (argc > 1 && r.Open(argv[1])) while (r.GetNextSequence(s)) ++n;\n  return n == 3000 ? 0 : 1; }\n")
    exe = str(tmp_path / "per_read")
    subprocess.check_call(["g++", "-std=c++17", "-fsyntax-only", "-Wall", "-I" + os.path.join(ROOT, "include"), str(src)])
    subprocess.check_call(["g++", "-std=c++17", "-O0", "-Wall", "-I" + os.path.join(ROOT, "include"), str(src), "-o", exe, "-lz"])
    assert subprocess.run([exe, os.path.join(ROOT, "tests", "golden", "sim1_bcr.head3000.fq")]).returncode == 0


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["sim1_bcr.head3000.fq", "tiny.fa"])
def test_next_batch_equals_the_per_read_loop(exe, golden_dir, name):
    for mb in BATCHES:
        r = subprocess.run([exe, "batch", os.path.join(golden_dir, name), mb], capture_output=True, text=True)
        assert r.returncode == 0 and r.stdout.startswith("BATCH OK"), r.stdout + r.stderr
        n, batches = map(int, r.stdout.split()[2:4])
        assert n > 0 and (batches == 2 if mb == "0" else batches >= 2)          # counted over the two passes


@pytest.mark.gpu
def test_mixing_the_two_forms_throws(exe, golden_dir):
    r = subprocess.run([exe, "mix", os.path.join(golden_dir, "sim1_bcr.head3000.fq")], capture_output=True, text=True)
    assert r.returncode == 0 and "MIX OK" in r.stdout, r.stdout + r.stderr


@pytest.mark.gpu
@pytest.mark.parametrize("hardclip", ["0", "1"])
def test_align_sequences_from_a_fastq_reader(exe, golden_dir, hardclip):
    r = subprocess.run([exe, "records", os.path.join(golden_dir, "tiny.fa"), os.path.join(golden_dir, "sim1_bcr.head3000.fq"), "70000", hardclip], capture_output=True, text=True)
    assert r.returncode == 0 and r.stdout.startswith("RECORDS OK 3000 "), r.stdout + r.stderr
    assert int(r.stdout.split()[3]) >= 3000


@pytest.mark.gpu
@pytest.mark.parametrize("hardclip", ["0", "1"])
def test_align_to_bam_from_a_fastq_reader_is_byte_identical(exe, golden_dir, tmp_path, hardclip):
    for mb in BATCHES:
        out = str(tmp_path / ("o" + mb))
        r = subprocess.run([exe, "tobam", os.path.join(golden_dir, "tiny.fa"), os.path.join(golden_dir, "sim1_bcr.head3000.fq"), out, mb, hardclip], capture_output=True, text=True)
        assert r.returncode == 0 and r.stdout.startswith("TOBAM"), r.stdout + r.stderr
        nv, nf, slow = map(int, r.stdout.split()[1:4])
        assert nv == nf >= 3000 and slow == 0
        assert open(out + ".v.bam", "rb").read() == open(out + ".f.bam", "rb").read()
