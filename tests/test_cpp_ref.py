"""SeqLib::RefGenome through the headers only (tests/cpp/ref_api_test.cpp): the program compiles with -Wall -Werror and links; without a GPU LoadIndex throws and
QueryRegion on an empty object throws std::invalid_argument; on the GPU the index text, QueryRegion and its exceptions, QueryRegions and FetchBatch are held
against tests/ref_util.py, NmMd(BamReader&) against the Python statement on the records the reader serves (whole file, SetRegions, SetReadFilter, a header with a
contig the FASTA lacks, a header with a wrong length), NmMd over the builder's records in HBM, and the MD of bwa-mem records against their host-built MD:Z."""
import os
import struct
import subprocess

import pytest

from tests import bam_util as bu
from tests import ref_util as ru

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")
TINY = os.path.join(GOLDEN, "tiny.fa")
FQ = os.path.join(GOLDEN, "sim1_bcr.head3000.fq")


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    import __graft_entry__ as g
    lib = os.path.join(ROOT, "seqlib_amd")
    if not os.path.exists(os.path.join(lib, "libseqlib_amd.so")):
        g.build()
    out = str(tmp_path_factory.mktemp("refapi") / "ref_api_test")
    subprocess.check_call(["g++", "-std=c++17", "-O2", "-Wall", "-Werror", "-I" + os.path.join(ROOT, "include"), os.path.join(ROOT, "tests", "cpp", "ref_api_test.cpp"), "-o", out,
                           "-L" + lib, "-lseqlib_amd", "-Wl,-rpath," + lib, "-lz", "-lpthread"])
    return out


@pytest.fixture(scope="module")
def sorted_records():
    """generated records over three contigs, coordinate-sorted, the unplaced ones last; the FASTA text of the contigs"""
    contigs = ru.bulk_contigs()
    recs = [r for r in ru.bulk_records(contigs, n=700) if len(r) < 3000]
    tid = lambda r: struct.unpack_from("<i", r, 4)[0]
    pos = lambda r: struct.unpack_from("<i", r, 8)[0]
    recs = sorted((r for r in recs if (0 <= tid(r) < 3 and pos(r) >= 0) or tid(r) < 0), key=lambda r: (tid(r) & 0xffffffff, pos(r)))
    return contigs, recs, ru.fasta([(b"c%d" % i, c) for i, c in enumerate(contigs)], 80)


def lines_of(want):
    return ["%d %s" % (nm, md.decode() or "-") for nm, md in want]


def test_cpp_mirror_links_and_throws_without_a_gpu(exe):
    r = subprocess.run([exe, "errors", TINY], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and r.stdout.startswith("ref api errors OK"), r.stdout[-2000:] + r.stderr[-2000:]
    assert "RefGenome::LoadIndex - " in r.stderr          # the unreadable file's sentence


@pytest.mark.gpu
def test_cpp_mirror_on_the_gpu(exe, tmp_path):
    bad = tmp_path / "bad.fa"
    bad.write_bytes(ru.BAD["ragged_short"][0])
    r = subprocess.run([exe, "run", TINY, str(bad)], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and r.stdout.endswith("ref api run OK\n"), r.stdout[-2000:] + r.stderr[-3000:]
    assert ru.bad_message("ragged_short") in r.stderr
    text = open(TINY, "rb").read()
    contigs = ru.contigs_of(text)
    out = r.stdout.split("\n")
    fai = open(TINY + ".fai").read()
    assert out[0] == "FAI" and "\n".join(out[1:5]) + "\n" == fai and (tmp_path / "bad.fa.written.fai").read_text() == fai
    want = []
    for name, ln, _, _, _, seq in contigs:
        for p1, p2 in ((0, 0), (0, 49), (ln - 10, ln + 100), (ln - 1, ln - 1)):
            want.append("Q %s %d %d %s" % (name.decode(), p1, p2, seq[p1:p2 + 1].decode()))
    assert [l for l in out if l.startswith("Q ")] == want
    l0 = contigs[0][1]
    regs = [(0, 10, 19), (3, 0, 2047), (0, l0 - 3, l0 + 3), (0, l0 + 3, l0 + 9)]
    assert [l for l in out if l.startswith("R ")] == ["R %d:%d-%d %s" % (t, a, b, contigs[t][5][a:b + 1].decode()) for t, a, b in regs]
    assert not os.path.exists(TINY + ".written.fai")


@pytest.mark.gpu
@pytest.mark.parametrize("how", ["all", "regions", "filter"])
def test_nm_md_of_a_readers_batches(exe, sl, tmp_path, sorted_records, how):
    from seqlib_amd import bamio, filterio
    contigs, recs, fa_text = sorted_records
    fa, bam = tmp_path / "ref.fa", tmp_path / "sorted.bam"
    fa.write_bytes(fa_text)
    refs = [("c%d" % i, len(c)) for i, c in enumerate(contigs)]
    text = "@HD\tVN:1.6\tSO:coordinate\n" + "".join("@SQ\tSN:%s\tLN:%d\n" % x for x in refs)
    bam.write_bytes(bu.bam_bytes(text, refs, recs, member_size=3000))
    bamio.index_build(bam)
    # the records the reader serves, through the C-ABI
    rd = bamio.Reader(bam)
    rd.index_load()
    if how == "regions":
        rd.set_regions([(0, 1000, 9000), (1, 0, 2000), (0, 8000, 20000)])
    if how == "filter":
        flt = filterio.Filter([dict(rules=[dict(mapq=(30, 255, False))])])
        flt.attach(rd)
    served = []
    while True:
        got, _ = rd.next(6000)
        if not got:
            break
        served += got
    rd.close()
    assert len(served) > 100 and (how != "all" or served == recs) and (how == "all" or served != recs)
    r = subprocess.run([exe, "reader", str(fa), str(bam), how], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and r.stdout.endswith("ref api reader OK %d\n" % len(served)), r.stdout[-2000:] + r.stderr[-3000:]
    want = [ru.nm_md(x, contigs) for x in served]
    assert r.stdout.split("\n")[:len(served)] == lines_of(want) and sum(nm > 0 for nm, _ in want) > 50


@pytest.mark.gpu
def test_a_header_that_differs_from_the_fasta(exe, sl, tmp_path, sorted_records):
    contigs, recs, fa_text = sorted_records
    fa = tmp_path / "ref.fa"
    fa.write_bytes(fa_text)
    # contig 1 under a name the FASTA lacks: its records are not eligible; the others are walked as before
    refs = [("c0", len(contigs[0])), ("elsewhere", len(contigs[1])), ("c2", len(contigs[2]))]
    bam = tmp_path / "missing.bam"
    bam.write_bytes(bu.bam_bytes("@HD\tVN:1.6\n", refs, recs, member_size=3000))
    r = subprocess.run([exe, "reader", str(fa), str(bam), "all"], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-3000:]
    want = [ru.nm_md(x, contigs, [0, -1, 2]) for x in recs]
    assert r.stdout.split("\n")[:len(recs)] == lines_of(want)
    assert sum(nm < 0 and ru.nm_md(x, contigs)[0] >= 0 for x, (nm, _) in zip(recs, want)) > 20
    # a contig of another length: std::invalid_argument
    refs = [("c0", len(contigs[0]) - 1), ("c1", len(contigs[1])), ("c2", len(contigs[2]))]
    bam = tmp_path / "wrong.bam"
    bam.write_bytes(bu.bam_bytes("@HD\tVN:1.6\n", refs, recs[:50], member_size=3000))
    r = subprocess.run([exe, "header", str(fa), str(bam)], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and "contig 'c0' has 29999 bases in the header and 30000 in the FASTA" in r.stdout, r.stdout[-2000:] + r.stderr[-3000:]


@pytest.mark.gpu
def test_nm_md_of_the_builders_records(exe, tmp_path):
    out = tmp_path / "built.bin"
    r = subprocess.run([exe, "builder", TINY, FQ, str(out)], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-3000:]
    raw = out.read_bytes()
    n, at, recs = struct.unpack_from("<I", raw)[0], 4, []
    for _ in range(n):
        bs = struct.unpack_from("<I", raw, at)[0]
        recs.append(raw[at:at + 4 + bs])
        at += 4 + bs
    assert n >= 500 and at == len(raw)
    seqs = [c[5] for c in ru.contigs_of(open(TINY, "rb").read())]
    assert r.stdout.split("\n")[:n] == lines_of([ru.nm_md(x, seqs) for x in recs])


@pytest.mark.gpu
def test_md_equals_the_host_built_md_of_bwa_mem_records(exe):
    """UseBwaMemRecords on the golden reads: on every forward-strand record the device's MD is the host-built MD:Z and its NM the NM tag (reverse-strand records
    are left out of this comparison only: the glue's kept quirk leaves C and G uncomplemented in their SEQ)"""
    r = subprocess.run([exe, "mdz", TINY, FQ], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and "ref api mdz OK" in r.stdout, r.stdout[-2000:] + r.stderr[-3000:]
    n_fwd = 0
    for line in r.stdout.split("\n")[:-2]:
        qname, flag, nm, md, mdz, tag = line.split(" ")
        if int(flag) & (4 | 16):
            continue
        assert md == mdz and int(nm) == int(tag), line
        n_fwd += 1
    assert n_fwd >= 1400
