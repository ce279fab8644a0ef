"""GPU tests of the record builder and BWAAligner::alignToBam (include/seqlib_amd_rec.h, include/SeqLib/BWAAligner.h): the file alignToBam writes is byte for
byte the file alignSequences + WriteRecords write through the same kind of writer; its records are the restated layout (tests/rec_util.py) applied to the host
hits; the reader form, the C-ABI through seqlib_amd/recio.py, one 70 000 bp read, and the edges.  The C++ side is tests/cpp/align_to_bam_test.cpp, compiled with
g++ through the headers as tests/test_cpp_bam.py does."""
import os
import random
import struct
import subprocess

import pytest

from tests import bam_util as bu
from tests import fml_util
from tests import rec_util as ru

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")
INDEX = os.path.join(GOLDEN, "tiny.fa")
RNG_STATE = (4242 << 16) | 0x330E          # the lrand48 state srand48(4242) leaves: what the C++ program starts every route from
PARAMS = [(False, 0.0, 0), (True, 0.9, 10), (False, 0.9, 10)]


@pytest.fixture(scope="module")
def exe(sl, tmp_path_factory):
    out = str(tmp_path_factory.mktemp("a2b") / "align_to_bam_test")
    lib = os.path.join(ROOT, "seqlib_amd")
    subprocess.check_call(["g++", "-std=c++17", "-O2", "-Wall", "-Werror", "-I" + os.path.join(ROOT, "include"), os.path.join(ROOT, "tests", "cpp", "align_to_bam_test.cpp"), "-o", out,
                           "-L" + lib, "-lseqlib_amd", "-Wl,-rpath," + lib, "-lz", "-lpthread"])
    return out


def run(exe, *args):
    r = subprocess.run([exe] + [str(a) for a in args], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-3000:]
    return r.stdout.strip().splitlines()


def constructed_reads():
    """a few dozen reads cut from tiny.fa: lengths 25-151 of both parities on both strands, some with a mismatch or an indel, some with N and lower case, a
    repeat of abl (two equal hits: a secondary), two-contig chimeras (clips), and random ones that yield no record"""
    rng = random.Random(17)
    g = {k: v.decode().upper() for k, v in fml_util.fixture_genome().items()}
    out = []
    for j, L in enumerate([25, 26, 31, 40, 63, 64, 65, 77, 100, 101, 127, 128, 149, 150, 151, 33, 48, 90]):
        name = rng.choice(sorted(g))
        at = rng.randrange(1000, len(g[name]) - 1000)
        s = g[name][at:at + L]
        if j % 2:
            s = bu.revcomp(s)
        if j % 3 == 0 and L > 60:
            p = L // 2
            s = s[:p] + ("A" if s[p] != "A" else "C") + s[p + 1:]                # a mismatch
        if j % 4 == 1 and L > 60:
            s = s[:L // 3] + "GT" + s[L // 3:]                                     # an insertion
        if j % 4 == 3 and L > 60:
            s = s[:L // 3] + s[L // 3 + 3:]                                        # a deletion
        if j % 5 == 2:
            s = s[:7] + "N" + s[8:12] + s[12:20].lower() + s[20:]                  # N and lower case
        out.append(("cut%d_%s_%d" % (j, name, at), s))
    out.append(("repeat_abl", g["abl"][66520:66650]))                             # abl 66514.. is repeated at 66970..: two equal hits
    out.append(("repeat_abl_rc", bu.revcomp(g["abl"][66530:66660])))
    for j in range(4):                                                             # chimeras: each half aligns alone, the other half is clipped
        a, b = rng.randrange(2000, 100000), rng.randrange(2000, 20000)
        s = g["bcr"][a:a + 70 + j] + g["tp53"][b:b + 75]
        out.append(("chimera%d" % j, bu.revcomp(s) if j & 1 else s))
    for j in range(6):
        out.append(("random%d" % j, "".join(rng.choice("ACGT") for _ in range(40 + 17 * j))))
    out.append(("x", g["myc"][500:560]))                                           # a one-byte name
    out.append(("L" * 254, g["myc"][700:795]))                                     # the longest name a record holds
    return out


@pytest.fixture(scope="module")
def reads():
    L = open(os.path.join(GOLDEN, "sim1_bcr.head3000.fq")).read().split("\n")
    fq = [(L[i][1:].split()[0], L[i + 1]) for i in range(0, len(L) - 3, 4)]
    assert len(fq) == 3000
    allr = fq[:1500] + constructed_reads() + fq[1500:]
    return [n.encode() for n, _ in allr], [s.encode() for _, s in allr]


@pytest.fixture(scope="module")
def tsv(reads, tmp_path_factory):
    p = tmp_path_factory.mktemp("reads") / "reads.tsv"
    p.write_bytes(b"".join(n + b"\t" + s + b"\n" for n, s in zip(*reads)))
    return p


@pytest.fixture(scope="module")
def aligner(sl):
    idx = sl.BWAIndex()
    idx.LoadIndex(INDEX)
    return sl.BWAAligner(idx)


@pytest.fixture(scope="module")
def vec_runs(exe, tsv, tmp_path_factory):
    """per parameter set, computed once: (file of route b, file of route c, the RECORDS line)"""
    cache = {}

    def get(params, chunk=0):
        key = (params, chunk)
        if key not in cache:
            hardclip, ksf, maxsec = params
            out = tmp_path_factory.mktemp("vec") / "out"
            lines = run(exe, "vec", INDEX, tsv, out, int(hardclip), ksf, maxsec, chunk)
            cache[key] = (open(str(out) + ".b.bam", "rb").read(), open(str(out) + ".c.bam", "rb").read(), [int(x) for x in lines[-1].split()[1:]])
        return cache[key]
    return get


def host_hits(aligner, seqs, hardclip, ksf, maxsec):
    aligner.rng_state, aligner.ordinal = RNG_STATE, 0
    return aligner.alignSequences(seqs, hardclip, ksf, maxsec)


@pytest.mark.parametrize("params", PARAMS)
def test_file_identity_vector_form(vec_runs, aligner, reads, params):
    """alignToBam's file is alignSequences + WriteRecords' file, and its records are the restated layout of the host hits"""
    names, seqs = reads
    fb, fc, (n_b, n_c, n_counter, _) = vec_runs(params)
    assert fb == fc and len(fc) > 10000
    text, refs, recs = bu.parse_bam(fc)
    assert n_b == n_c == n_counter == len(recs) and [r[0] for r in refs] == ["bcr", "abl", "tp53", "myc"]
    h = host_hits(aligner, seqs, *params)
    exp = ru.records_from_hits(h, seqs, names, params[0])
    assert len(exp) == len(recs)
    for k, (e, r) in enumerate(zip(exp, recs)):
        assert e == r["raw"], "record %d (%s) differs from the layout" % (k, r["name"])
    # the input produced what it is there for
    per_read = [int(h["hit_off"][i + 1] - h["hit_off"][i]) for i in range(len(seqs))]
    assert any(r["flag"] & 0x10 for r in recs) and any(not r["flag"] & 0x10 for r in recs)
    assert 0 in per_read and any(names[i].startswith(b"random") and per_read[i] == 0 for i in range(len(seqs)))
    if params[2] > 0:
        assert any(r["flag"] & 0x100 for r in recs) and max(per_read) >= 2
    clipped = [r for r in recs if any((w & 15) == (5 if params[0] else 4) for w in struct.unpack_from("<%dI" % r["n_cigar"], r["data"], r["l_name"]))]
    assert clipped
    if params[0]:
        assert any(r["l_seq"] < len(seqs[names.index(r["name"].encode())]) for r in clipped)          # a hard-clipped record shows less than its read


def test_file_identity_in_several_chunks(vec_runs):
    """the same input cut into chunks of 1 024 reads: chunk boundaries change neither the draws nor the bytes"""
    assert vec_runs(PARAMS[2], 1024)[1] == vec_runs(PARAMS[2])[1]


@pytest.fixture(scope="module")
def unaligned_bam(reads, tmp_path_factory):
    """the same reads as an unaligned BAM; every 11th record carries 0x10 (stored reverse-complemented), every 13th is a 0x900 record the realignment skips"""
    names, seqs = reads
    recs, kept = [], 0
    for i, (n, s) in enumerate(zip(names, seqs)):
        s = "".join(c if c in "ACGT" else "N" for c in s.decode().upper())
        if i % 13 == 5:
            recs.append(bu.bam_record(n.decode(), 0x900 if i % 2 else 0x100, -1, -1, 0, [], s[:40]))
            continue
        kept += 1
        recs.append(bu.bam_record(n.decode(), 0x14, -1, -1, 0, [], bu.revcomp(s)) if i % 11 == 3 else bu.bam_record(n.decode(), 4, -1, -1, 0, [], s))
    p = tmp_path_factory.mktemp("ubam") / "reads.bam"
    p.write_bytes(bu.bam_bytes(bu.TEXT, bu.REFS, recs))
    return p, kept


@pytest.mark.parametrize("batch_bytes,orig", [(150000, False), (150000, True), (0, False), (0, True)])
def test_file_identity_reader_form(exe, unaligned_bam, tmp_path, batch_bytes, orig):
    path, kept = unaligned_bam
    lines = run(exe, "reader", INDEX, path, tmp_path / "out", batch_bytes, int(orig), 0)
    n_b, n_c, n_counter, _ = (int(x) for x in lines[0].split()[1:])
    fb, fc = (tmp_path / "out.b.bam").read_bytes(), (tmp_path / "out.c.bam").read_bytes()
    assert fb == fc
    recs = bu.parse_bam(fc)[2]
    assert n_b == n_c == n_counter == len(recs) and len(recs) > kept // 2
    batches = int(lines[1].split()[1])
    assert batches >= 3 if batch_bytes else batches >= 1


def test_c_abi_build_and_refusals(sl, aligner, reads, vec_runs):
    """slx_rec_build on a device result through recio: the offsets are the record starts, the stream is the one the files hold; host-resident and REG2SAM results
    are refused"""
    from seqlib_amd import _ffi, recio
    names, seqs = reads
    params = PARAMS[2]
    rb = recio.Builder(aligner._handle())
    d_bases, d_offs, d_names, d_name_offs = rb.upload(seqs, names)
    aligner.rng_state = RNG_STATE
    hits = aligner.align_device(d_bases, d_offs, len(seqs), 0, *params)
    b = rb.build(hits, d_bases, d_offs, d_names, d_name_offs, params[0])
    stream, off = rb.to_host(b)
    recs = bu.parse_bam(vec_runs(params)[1])[2]
    assert b.n_records == len(recs) == len(off) - 1 and off[0] == 0 and off[-1] == b.n_bytes == len(stream)
    for k, r in enumerate(recs):
        assert off[k + 1] - off[k] == len(r["raw"])
    assert stream == b"".join(r["raw"] for r in recs)
    assert rb.counter("records") == len(recs) and rb.counter("bytes") == len(stream) and rb.counter("us_fill") >= 0 and rb.counter("nonsense") == -1
    # a host-resident result
    bases = b"".join(seqs[:50])
    offs = recio.flatten(seqs[:50])[1]
    hh = aligner.align_host_raw(bases, offs.ctypes.data, 50, 0)
    with pytest.raises(_ffi.SlxError) as e:
        rb.build(hh, d_bases, d_offs, d_names, d_name_offs)
    assert e.value.code == _ffi.SLX_EINVAL and "host-resident" in str(e.value)
    aligner.free_hits(hh)
    # bwa's own record selection: host-built tags
    aligner.opt.flag |= _ffi.SLX_F_REG2SAM
    try:
        hits = aligner.align_device(d_bases, d_offs, len(seqs), 0, *params)
        with pytest.raises(_ffi.SlxError) as e:
            rb.build(hits, d_bases, d_offs, d_names, d_name_offs)
        assert e.value.code == _ffi.SLX_EUNSUPPORTED and "REG2SAM" in str(e.value)
    finally:
        aligner.opt.flag &= ~_ffi.SLX_F_REG2SAM
    rb.close()


def test_one_long_read(exe, tmp_path):
    """70 000 bp of abl with a handful of edits (the aligner's wide build), and 20 000 bp with a base deleted every 60 (a CIGAR of hundreds of operations: sized
    by a wave): the files are identical and the first record shows all 70 000 bases"""
    g = fml_util.fixture_genome()["abl"].decode().upper()
    s = list(g[20000:90001])          # 70 001 bases: three go in and four come out below
    for p, c in ((5000, "A"), (21000, "C"), (40000, "G"), (65000, "T")):
        s[p] = c if s[p] != c else "ACGT"[("ACGT".index(c) + 1) % 4]
    long_read = "".join(s[:30000]) + "ACG" + "".join(s[30000:50000]) + "".join(s[50004:])
    gappy = "".join(g[100000 + i:100000 + i + 59] for i in range(0, 20000, 60))
    p = tmp_path / "long.tsv"
    assert len(long_read) == 70000
    p.write_text("contig70k\t%s\ngappy\t%s\n" % (long_read, gappy))
    lines = run(exe, "vec", INDEX, p, tmp_path / "out", 0, 0.9, 10)
    n_b, n_c, n_counter, wide = (int(x) for x in lines[-1].split()[1:])
    fb, fc = (tmp_path / "out.b.bam").read_bytes(), (tmp_path / "out.c.bam").read_bytes()
    assert fb == fc and n_b == n_c == n_counter >= 2
    recs = bu.parse_bam(fc)[2]
    assert recs[0]["name"] == "contig70k" and recs[0]["l_seq"] == 70000 and recs[0]["seq"] == long_read
    assert wide >= 1 and max(r["n_cigar"] for r in recs if r["name"] == "gappy") > 256


def test_edges(exe, reads, tmp_path):
    """an empty input, the writers and the record mode alignToBam refuses, WriteDevice's refusals, a name of 255 bytes"""
    names, seqs = reads
    (tmp_path / "read.tsv").write_bytes(b"good\t" + seqs[0] + b"\n")
    lines = run(exe, "edges", INDEX, tmp_path, tmp_path / "read.tsv")
    assert lines[-1] == "edges OK"
    eb, ec = (tmp_path / "empty.b.bam").read_bytes(), (tmp_path / "empty.c.bam").read_bytes()
    assert eb == ec and bu.parse_bam(ec)[2] == [] and ec.endswith(bu.EOF_BLOCK)
    recs = bu.parse_bam((tmp_path / "name255.bam").read_bytes())[2]          # nothing of the refused batch, all of the one that followed
    got = [r["name"] for r in recs]
    assert got.count("good") == got.count("n" * 254) == got.count("after") >= 1 and set(got) == {"good", "n" * 254, "after"}
    assert got.index("good") < got.index("n" * 254) < got.index("after")
    assert bu.parse_bam((tmp_path / "host.bam").read_bytes())[2] == [] and bu.parse_bam((tmp_path / "mem.bam").read_bytes())[2] == []
