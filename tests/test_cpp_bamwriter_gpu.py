"""SeqLib::BamWriter with UseGpu() through the C++ classes on the GPU (tests/cpp/bam_writer_gpu_test.cpp): fixture reads aligned, the records written by the
host writer, by UseGpu() + WriteRecord and by UseGpu() + WriteRecords; the inflated streams and the ISIZE lists are equal, BamReader reads the GPU-written
file, BuildIndex succeeds on a sorted one."""
import os
import subprocess

import pytest

from tests import bai_util as ba
from tests import bam_util as bu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.gpu
def test_cpp_writer_on_the_gpu(golden_dir, tmp_path):
    import __graft_entry__ as g
    lib = os.path.join(ROOT, "seqlib_amd")
    if not os.path.exists(os.path.join(lib, "libseqlib_amd.so")):
        g.build()
    exe = str(tmp_path / "bam_writer_gpu_test")
    subprocess.check_call(["g++", "-std=c++17", "-O2", "-Wall", "-Werror", "-I" + os.path.join(ROOT, "include"), os.path.join(ROOT, "tests", "cpp", "bam_writer_gpu_test.cpp"), "-o", exe,
                           "-L" + lib, "-lseqlib_amd", "-Wl,-rpath," + lib, "-lz", "-lpthread"])
    r = subprocess.run([exe, os.path.join(golden_dir, "tiny.fa"), os.path.join(golden_dir, "sim1_bcr.head3000.fq"), "3000", str(tmp_path)], capture_output=True, text=True)
    assert r.returncode == 0 and r.stdout.startswith("writer OK") and int(r.stdout.split()[2]) >= 3000, r.stdout[-2000:] + r.stderr[-2000:]
    assert "BamWriter::UseGpu - call it before Open()" in r.stderr and "Trying to index open BAM" in r.stderr
    host, one, many = ((tmp_path / n).read_bytes() for n in ("host.bam", "gpu_one.bam", "gpu_many.bam"))
    assert one == many                                # the splitting over calls does not show
    stream = bu.inflate_all(host)
    assert bu.inflate_all(one) == stream and len(stream) > 500000
    isizes = lambda raw: [m[3] for m in bu.scan_members(raw)[0]]
    assert isizes(one) == isizes(host) and bu.scan_members(one)[1]
    assert not (tmp_path / "again.bam").exists()
    # the index the class wrote from the GPU-written sorted file parses, and counts that file's records
    bai = ba.parse_bai((tmp_path / "gpu_sorted.bam.bai").read_bytes())
    n_sorted = len(bu.parse_bam((tmp_path / "gpu_sorted.bam").read_bytes())[2])
    assert sum(r["meta"][2] + r["meta"][3] for r in bai["refs"] if r["meta"]) + (bai["n_no_coor"] or 0) == n_sorted >= 3000
