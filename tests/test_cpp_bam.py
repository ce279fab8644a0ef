"""The C++ mirror of SeqLib::BamReader (include/SeqLib/BamReader.h) and BWAAligner::alignSequences(BamReader&) compiled with g++ through the headers only
and driven as a SeqLib user drives them (tests/cpp/bam_reader_test.cpp): records and header against the Python parser of tests/bam_util.py, the round
trip with BamWriter, realignment from a BAM against aligning the FASTQ directly (the path pinned to the oracle), and the reference README's two loops."""
import os
import subprocess

import pytest

from tests import bam_util as bu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    import __graft_entry__ as g
    if not os.path.exists(os.path.join(ROOT, "seqlib_amd", "libseqlib_amd.so")):
        g.build()
    out = str(tmp_path_factory.mktemp("cpp") / "bam_reader_test")
    lib = os.path.join(ROOT, "seqlib_amd")
    subprocess.check_call(["g++", "-std=c++17", "-O2", "-Wall", "-I" + os.path.join(ROOT, "include"), os.path.join(ROOT, "tests", "cpp", "bam_reader_test.cpp"),
                           "-o", out, "-L" + lib, "-lseqlib_amd", "-Wl,-rpath," + lib, "-lz", "-lpthread"])
    return out


def run(exe, *args):
    r = subprocess.run([exe] + [str(a) for a in args], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    return r


def test_cpp_bam_reader_refuses_without_a_file(exe, tmp_path):
    r = run(exe, "refuse", tmp_path / "missing.bam")
    assert "refuse OK" in r.stdout and "failed to open" in r.stderr and "cannot open" in r.stderr


def fastq_reads(golden_dir):
    out = []
    for fn in ("sim1_bcr.head3000.fq", "sim2_bcr.head3000.fq"):
        L = open(os.path.join(golden_dir, fn)).read().split("\n")
        out += [(L[i][1:].split()[0], L[i + 1], L[i + 3]) for i in range(0, 4 * 3000, 4)]
    return out


@pytest.mark.gpu
def test_cpp_bam_reader_yields_the_parsers_records(exe, tmp_path):
    recs = bu.sample_records(4000)
    raw = bu.bam_bytes(bu.TEXT, bu.REFS, recs, member_size=0x7000)
    p = tmp_path / "a.bam"
    p.write_bytes(raw)
    text, refs, want = bu.parse_bam(raw)
    blob = b"".join(w["raw"] for w in want)
    hdr = text + "--\n" + "".join("%s\t%d\n" % r for r in refs)
    for k, (batch, how, fail, chunk) in enumerate(((64 << 20, "next", 0, 65536), (100000, "batch", 0, 65536), (5000, "reset", 0, 4096), (64 << 20, "batch", 1, 65536), (1, "next", 0, 65536))):
        out = tmp_path / ("out%d.bin" % k)
        r = run(exe, "dump", p, out, batch, how, fail, chunk)
        assert out.read_bytes() == blob, (batch, how)
        assert open(str(out) + ".hdr").read() == hdr
        d = dict(ln.split() for ln in r.stdout.strip().splitlines())
        assert int(d["RECORDS"]) == len(recs) and (int(d["REPAIRED"]) > 0) == bool(fail), d
    # the decoy file through the class
    dec = bu.decoy_records()
    p.write_bytes(bu.bam_bytes(bu.TEXT, bu.REFS, dec))
    out = tmp_path / "dec.bin"
    r = run(exe, "dump", p, out, 64 << 20, "next", 0, 65536)
    assert out.read_bytes() == b"".join(dec) and "REPAIRED 0" not in r.stdout
    # a header whose text carries no @SQ lines: the dictionary is the binary one
    p.write_bytes(bu.bam_bytes("@HD\tVN:1.6\n", bu.REFS, recs[:50]))
    run(exe, "dump", p, out, 64 << 20, "next", 0, 65536)
    assert open(str(out) + ".hdr").read().split("--\n")[1] == "".join("%s\t%d\n" % r for r in bu.REFS)
    r = run(exe, "refuse_open", p)
    assert "refuse_open OK" in r.stdout and "already open" in r.stderr and "SetRegion" in r.stderr and "SetRegions" in r.stderr and "CRAM" in r.stderr


@pytest.mark.gpu
def test_cpp_round_trip_with_the_writer(exe, golden_dir, tmp_path):
    r = run(exe, "roundtrip", os.path.join(golden_dir, "tiny.fa"), os.path.join(golden_dir, "sim1_bcr.head3000.fq"), 3000, tmp_path / "rt.bam")
    assert r.stdout.startswith("roundtrip OK") and int(r.stdout.split()[2]) >= 3000


def realign_lines(exe, golden_dir, tmp_path, original_strand):
    reads = fastq_reads(golden_dir)
    recs, stored = [], []
    for i, (name, seq, qual) in enumerate(reads):
        q = bytes(ord(c) - 33 for c in qual)
        if i % 2:                                   # the record shows the reverse complement, 0x10 says so: the read as sequenced is `seq`
            recs.append(bu.bam_record(name, 0x10, 0, 100 + i, 20, [("M", len(seq))], bu.revcomp(seq), q[::-1]))
            stored.append(bu.revcomp(seq))
        else:
            recs.append(bu.bam_record(name, 4, -1, -1, 0, [], seq, q))
            stored.append(seq)
        if i % 5 == 0:                              # secondary and supplementary lines of the same read: skipped by 0x900
            recs.append(bu.bam_record(name, 0x100 if i % 10 else 0x800, 1, 5 + i, 0, [("M", 40), ("S", len(seq) - 40)], seq, None))
    bam = tmp_path / "in.bam"
    bam.write_bytes(bu.bam_bytes(bu.TEXT, bu.REFS, recs))
    fq = tmp_path / "direct.fq"
    with open(fq, "w") as f:
        for (name, seq, qual), st in zip(reads, stored):
            f.write("@%s\n%s\n+\n%s\n" % (name, seq if original_strand else st, qual))
    r = run(exe, "realign", os.path.join(golden_dir, "tiny.fa"), fq, bam, len(reads), 1 if original_strand else 0)
    a = [ln[2:] for ln in r.stdout.split("\n") if ln.startswith("A\t")]
    b = [ln[2:] for ln in r.stdout.split("\n") if ln.startswith("B\t")]
    return a, b, len(reads)


@pytest.mark.gpu
@pytest.mark.parametrize("original_strand", [True, False])
def test_cpp_realignment_from_a_bam_equals_the_fastq(exe, golden_dir, tmp_path, original_strand):
    """6 000 fixture reads in a Python-built BAM, half of them stored reverse-complemented with 0x10, 0x100 / 0x800 records interleaved: every field of
    every record of alignSequences(BamReader&, ..., 0x900, original_strand) equals aligning the FASTQ directly (original_strand) / the stored strings"""
    a, b, n = realign_lines(exe, golden_dir, tmp_path, original_strand)
    assert a == b
    assert len(a) >= n and len({ln.split("\t")[0] for ln in a}) == n


@pytest.mark.gpu
def test_cpp_readme_loops(exe, golden_dir, tmp_path):
    reads = fastq_reads(golden_dir)[:3000]          # (the first fixture file: enough coverage for contigs)
    recs = [bu.bam_record(name, 4, -1, -1, 0, [], seq, bytes(ord(c) - 33 for c in qual)) for name, seq, qual in reads]
    bam = tmp_path / "small.bam"
    bam.write_bytes(bu.bam_bytes(bu.TEXT, bu.REFS, recs))
    out = tmp_path / "out.bam"
    r = run(exe, "readme", os.path.join(golden_dir, "tiny.fa"), bam, out)
    d = {ln.split()[0]: [int(x) for x in ln.split()[1:]] for ln in r.stdout.strip().splitlines()}
    assert d["REALIGNED"][0] == 3000 and d["REALIGNED"][1] >= 2900
    assert d["CONTIGS"][0] == 3000 and d["CONTIGS"][1] >= 1 and d["CONTIGS"][2] > 200
    # what the loop wrote is a BAM this project's own parser statement reads: one record per alignment, names from the input
    text, refs, got = bu.parse_bam(out.read_bytes())
    assert len(got) == d["REALIGNED"][1] and [r[0] for r in refs] == ["bcr", "abl", "tp53", "myc"]
    assert {g["name"] for g in got} <= {name for name, _, _ in reads}
