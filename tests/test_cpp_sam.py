"""SeqLib::BamReader over SAM text (include/SeqLib/BamReader.h) compiled with g++ through the headers only and driven as a SeqLib user drives it
(tests/cpp/sam_reader_test.cpp): what BamWriter(SAM) writes is read back as what BamWriter(BAM) writes from the same records, through Next and NextBatch; the
aligner's two reader forms give from the SAM what they give from the BAM; SAM text has no regions."""
import os
import subprocess

import pytest

from tests import bam_util as bu
from tests import sam_util as su

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    import __graft_entry__ as g
    if not os.path.exists(os.path.join(ROOT, "seqlib_amd", "libseqlib_amd.so")):
        g.build()
    out = str(tmp_path_factory.mktemp("cpp") / "sam_reader_test")
    lib = os.path.join(ROOT, "seqlib_amd")
    subprocess.check_call(["g++", "-std=c++17", "-O2", "-Wall", "-Werror", "-I" + os.path.join(ROOT, "include"), os.path.join(ROOT, "tests", "cpp", "sam_reader_test.cpp"),
                           "-o", out, "-L" + lib, "-lseqlib_amd", "-Wl,-rpath," + lib, "-lz", "-lpthread"])
    return out


def run(exe, *args):
    r = subprocess.run([exe] + [str(a) for a in args], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-3000:]
    return r


def split_records(blob):
    out, p = [], 0
    while p < len(blob):
        n = 4 + int.from_bytes(blob[p:p + 4], "little")
        out.append(blob[p:p + n])
        p += n
    return out


def test_cpp_open_of_sam_text_without_a_gpu_is_false(exe, tmp_path):
    import torch
    if torch.cuda.is_available():
        pytest.skip("GPU present")
    p = tmp_path / "a.sam"
    p.write_bytes(su.sam_text(bu.TEXT, su.canonical(5)[0]))
    r = run(exe, "refuse", p)
    assert "refuse OK" in r.stdout and "failed to open" in r.stderr and "no HIP device" in r.stderr


@pytest.fixture(scope="module")
def pair(exe, tmp_path_factory):
    """the same BamRecords written by BamWriter(SAM) and by BamWriter(BAM)"""
    d = tmp_path_factory.mktemp("pair")
    recs = bu.sample_records(2000)
    src = d / "src.bam"
    src.write_bytes(bu.bam_bytes(bu.TEXT, bu.REFS, recs))
    sam, bam = d / "w.sam", d / "w.bam"
    r = run(exe, "write", src, sam, bam)
    assert "WRITTEN %d" % len(recs) in r.stdout
    return dict(dir=d, recs=recs, sam=sam, bam=bam)


@pytest.mark.gpu
@pytest.mark.parametrize("how,batch_bytes", [("next", 64 << 20), ("batch", 64 << 20), ("next", 3000), ("batch", 100000)])
def test_cpp_sam_and_bam_of_the_same_records_read_back_equal(exe, pair, tmp_path, how, batch_bytes):
    got = {}
    for kind in ("sam", "bam"):
        out = tmp_path / (kind + ".bin")
        r = run(exe, "dump", pair[kind], out, how, batch_bytes)
        d = dict(ln.split() for ln in r.stdout.strip().splitlines())
        assert d == dict(SAM="1" if kind == "sam" else "0", INDEX="0", REGION="0", RECORDS=str(len(pair["recs"]))), d
        if kind == "sam":
            assert "SAM text, which has no index" in r.stderr
        got[kind] = split_records(out.read_bytes())
        assert open(str(out) + ".hdr").read() == bu.TEXT
    assert got["bam"] == pair["recs"]
    # the text of the written SAM is what the Python statement reads, and the reader's records are its records
    text, refs, want, bad = su.parse_text(pair["sam"].read_bytes())
    assert bad is None and (text.decode(), refs) == (bu.TEXT, bu.REFS) and got["sam"] == want
    # fields and data equal, integer aux compared by value (they come back in the smallest type): the two records print the same line
    assert [su.record_to_line(r, bu.REFS) for r in got["sam"]] == [su.record_to_line(r, bu.REFS) for r in got["bam"]]
    same = sum(a == b for a, b in zip(got["sam"], got["bam"]))
    assert 0 < same < len(want)          # records without integer aux are the same bytes; the others differ in the type letter only


@pytest.fixture(scope="module")
def unaligned(tmp_path_factory):
    """fixture reads as unaligned records, some stored reverse-complemented (0x10), some 0x900 records the realignment skips: as SAM text and as BAM"""
    L = open(os.path.join(GOLDEN, "sim1_bcr.head3000.fq")).read().split("\n")
    recs = []
    for i in range(0, 4 * 1500, 4):
        name, seq, qual = L[i][1:].split()[0], L[i + 1], bytes(ord(c) - 33 for c in L[i + 3])
        k = i // 4
        if k % 13 == 5:
            recs.append(bu.bam_record(name, 0x900 if k % 2 else 0x100, -1, -1, 0, [], seq[:40]))
        elif k % 11 == 3:
            recs.append(bu.bam_record(name, 0x14, -1, -1, 0, [], bu.revcomp(seq), qual[::-1]))
        else:
            recs.append(bu.bam_record(name, 4, -1, -1, 0, [], seq, qual))
    d = tmp_path_factory.mktemp("unal")
    bam, sam = d / "reads.bam", d / "reads.sam"
    bam.write_bytes(bu.bam_bytes(bu.TEXT, bu.REFS, recs))
    lines = [su.record_to_line(r, bu.REFS) for r in recs]
    assert [su.line_to_record(ln, bu.REFS) for ln in lines] == recs          # no integer aux here: the two files hold the same records
    sam.write_bytes(su.sam_text(bu.TEXT, lines))
    return sam, bam


@pytest.mark.gpu
@pytest.mark.parametrize("batch_bytes", [0, 60000])
def test_cpp_aligning_from_sam_equals_aligning_from_bam(exe, unaligned, tmp_path, batch_bytes):
    sam, bam = unaligned
    out = {}
    for kind, path in (("sam", sam), ("bam", bam)):
        r = run(exe, "align", os.path.join(GOLDEN, "tiny.fa"), path, tmp_path / kind, batch_bytes)
        n_a, n_b = (int(x) for x in r.stdout.split()[1:3])
        assert n_a == n_b > 1000
        out[kind] = ((tmp_path / (kind + ".recs.bin")).read_bytes(), (tmp_path / (kind + ".bam")).read_bytes())
    if batch_bytes == 0:
        assert out["sam"][0] == out["bam"][0]          # alignSequences(BamReader&): the same records (one batch on both: the same draws of lrand48)
        assert out["sam"][1] == out["bam"][1]          # alignToBam(BamReader&): the same file, byte for byte
    else:                                              # batches are cut at other places (text bytes against inflated bytes): the records are the same set read by read
        a, b = (sorted(split_records(out[k][0])) for k in ("sam", "bam"))
        assert len(a) == len(b)
        names = lambda rs: sorted(r[36:36 + r[12] - 1] for r in rs)
        assert names(a) == names(b)
