"""SeqLib::BamWriter with UseGpuSam() through the C++ classes on the GPU (tests/cpp/sam_writer_gpu_test.cpp): fixture reads aligned and written as SAM by the host
writer, by UseGpuSam() + WriteRecord, + WriteRecords and + alignToBam in its three forms; every file is the host writer's, byte for byte; the bgzip'd one inflates
to it; what stays refused stays refused."""
import os
import subprocess

import pytest

from tests import bam_util as bu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
N_READS = 1200


@pytest.mark.gpu
def test_cpp_sam_writer_on_the_gpu(golden_dir, tmp_path):
    import __graft_entry__ as g
    lib = os.path.join(ROOT, "seqlib_amd")
    if not os.path.exists(os.path.join(lib, "libseqlib_amd.so")):
        g.build()
    exe = str(tmp_path / "sam_writer_gpu_test")
    subprocess.check_call(["g++", "-std=c++17", "-O2", "-Wall", "-Werror", "-I" + os.path.join(ROOT, "include"), os.path.join(ROOT, "tests", "cpp", "sam_writer_gpu_test.cpp"), "-o", exe,
                           "-L" + lib, "-lseqlib_amd", "-Wl,-rpath," + lib, "-lz", "-lpthread"])
    # the same reads as FASTQ and as unaligned BAM records
    L = open(os.path.join(golden_dir, "sim1_bcr.head3000.fq")).read().split("\n")[:4 * N_READS]
    fq, bam = tmp_path / "reads.fq", tmp_path / "reads.bam"
    fq.write_text("\n".join(L) + "\n")
    recs = [bu.bam_record(L[i][1:].split()[0], 4, -1, -1, 0, [], L[i + 1], bytes(ord(c) - 33 for c in L[i + 3])) for i in range(0, 4 * N_READS, 4)]
    bam.write_bytes(bu.bam_bytes(bu.TEXT, bu.REFS, recs))
    r = subprocess.run([exe, os.path.join(golden_dir, "tiny.fa"), str(fq), str(bam), str(tmp_path)], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0 and r.stdout.startswith("sam writer OK"), r.stdout[-2000:] + r.stderr[-3000:]
    n_recs, n_a2b, n_rd, n_fq, fast, slow = (int(x) for x in r.stdout.split()[3:9])
    assert n_recs == n_a2b == n_rd == n_fq >= N_READS and fast == n_recs and slow == 0
    for msg in ("BamWriter::UseGpuSam - call it before Open()", "BamWriter::UseGpuSam - only SAM output", "BamWriter::UseGpu - only BAM output", "needs the records' offsets",
                "only BAM output takes records from the GPU", "Failed to create index"):
        assert msg in r.stderr, msg
    host = (tmp_path / "host.sam").read_bytes()
    lines = host.split(b"\n")
    assert lines[-1] == b"" and sum(1 for ln in lines[:-1] if ln[:1] != b"@") == n_recs and lines[0][:1] == b"@"
    assert len(host) > 100 * n_recs          # (every line carries its read's bases)
    for name in ("gpu_one.sam", "gpu_many.sam", "gpu_a2b.sam", "gpu_rd.sam", "gpu_fq.sam"):
        assert (tmp_path / name).read_bytes() == host, name
    z = (tmp_path / "gpu_a2b.sam.gz").read_bytes()
    assert bu.scan_members(z)[1] and bu.inflate_all(z) == host
    assert not (tmp_path / "again.sam").exists()
    # the shape of a record line: eleven fields and more, SEQ over the alphabet
    first = next(ln for ln in lines if ln[:1] != b"@").split(b"\t")
    assert len(first) >= 11 and set(first[9].decode()) <= set(bu.SEQ_CODES) and first[1].isdigit()
