"""CPU tests of the record builder (include/seqlib_amd_rec.h, seqlib_amd/csrc/slx_rec.hip, dev_rec.h): the exports, the refusal without a GPU, and the
host-compiled size and fill bodies under ASan + UBSan against the Python restatement of the record layout (tests/rec_util.py).  No test here needs a GPU."""
import os
import random
import re
import subprocess

import pytest

from tests import rec_util as ru
from tests.test_sanitizers import ENV, SAN

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
L_SEQS = (1, 2, 15, 16, 17, 33, 150, 151)


@pytest.fixture(scope="module")
def ffi():
    import __graft_entry__ as g
    if not os.path.exists(os.path.join(ROOT, "seqlib_amd", "libseqlib_amd.so")):
        g.build()
    from seqlib_amd import _ffi
    _ffi.lib()
    return _ffi


def test_rec_exports_match_header(ffi):
    from seqlib_amd import bamio, recio
    hdr = open(os.path.join(ROOT, "include", "seqlib_amd_rec.h")).read()
    body = hdr[hdr.index("extern \"C\""):]
    declared = set(re.findall(r"\b(slx_rec_[a-z0-9_]+)\s*\(", body))
    assert declared == set(recio.REC_EXPORTS) and len(declared) == 7, declared ^ set(recio.REC_EXPORTS)
    L = recio.lib()
    for name in declared:
        assert hasattr(L, name), name
    head = hdr[:hdr.index("#ifndef")]
    for name in ("slx_rec_create", "slx_rec_build", "slx_rec_build_from_bam", "slx_rec_to_host", "slx_rec_counter"):
        assert name in head
    assert "src/BWAAligner.cpp:151-248" in head and "src/BamWriter.cpp:103-113" in head and "Not carried" in head
    for other in ("seqlib_amd.h", "seqlib_amd_bam.h"):
        assert "slx_rec_" not in open(os.path.join(ROOT, "include", other)).read(), other
    assert not any(e.startswith("slx_rec_") for e in ffi.EXPORTS + bamio.EXPORTS + bamio.BAI_EXPORTS + bamio.BGZF_EXPORTS)


def test_rec_no_gpu_fails_loudly(ffi):
    import torch
    if torch.cuda.is_available():
        pytest.skip("GPU present")
    from seqlib_amd import recio
    with pytest.raises(ffi.SlxError) as e:
        recio.Builder(None)
    assert e.value.code == ffi.SLX_ENODEVICE and "no CPU fallback" in str(e.value)


@pytest.fixture(scope="module")
def host_exe(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("rec") / "rec_host_test")
    subprocess.check_call(["g++", "-std=c++17"] + SAN + ["-Wall", "-Wno-unknown-pragmas", "-o", exe, os.path.join(ROOT, "tests", "cpp", "rec_host_test.cpp")])
    return exe


def run_host(exe, image, out):
    r = subprocess.run([exe, str(image), str(out)], capture_output=True, text=True, env=ENV, timeout=300)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    assert "runtime error" not in r.stderr and "AddressSanitizer" not in r.stderr and "LeakSanitizer" not in r.stderr, r.stderr[-3000:]
    return r.stdout.strip().splitlines()


ALPHABET = "ACGT" * 6 + "NacgtRY=n"


def synthetic(hardclip, seed):
    """reads, names and hits that cover what the issue lists; -> (per-read hit lists, seqs, names)"""
    rng = random.Random(seed)
    clip = "H" if hardclip else "S"
    per_read, seqs, names = [], [], []

    def read(length):
        return "".join(rng.choice(ALPHABET) for _ in range(length)).encode()

    def add(seq, name, hits):
        seqs.append(seq); names.append(name); per_read.append(hits)

    def hit(cigar, pos=None, flag=0, rid=0):
        return dict(rid=rid, pos=rng.randrange(1000, 5000000) if pos is None else pos, flag=flag, mapq=rng.randrange(61), score=rng.randrange(-5, 300), nm=rng.randrange(12),
                    na=rng.randrange(1, 9), cigar=ru.cig(cigar))

    n = 0
    for L in L_SEQS:
        for a, b in ((0, 0), (3, 0), (0, 4), (2, 5)):
            for flag in (0, 0x10):
                # hardclip: the window is L, the read L + a + b; otherwise the read is L and the clips lie inside it
                q = L if hardclip else L - a - b
                if q < 1:
                    continue
                core = "%dM" % q if q < 6 else rng.choice(["%dM" % q, "%dM2I%dM" % (2, q - 4), "%dM3D%dM" % (q - 2, 2), "1M1I1M1D%dM" % (q - 3)])
                cigar = ("%d%s" % (a, clip) if a else "") + core + ("%d%s" % (b, clip) if b else "")
                name = ("r%d" % n).encode()
                n += 1
                add(read(L + a + b if hardclip else L), name, [hit(cigar, flag=flag), hit(cigar, flag=flag | 0x100, rid=1)] if n % 5 == 0 else [hit(cigar, flag=flag)])
                if n % 7 == 0:
                    add(read(40), b"nohit%d" % n, [])          # a read without hits between two with hits
    add(read(30), b"x", [hit("30M")])                                                          # names of 1 and 254 bytes
    add(read(31), b"N" * 254, [hit("31M", flag=0x10)])
    add(read(20), b"span", [hit("10M1000D10M", pos=16000)])                                    # the deletion moves end, and the bin, across a 16 KiB boundary
    add(read(10), b"bin0", [hit("10M", pos=(1 << 26) - 5)])                                    # spans a 64 MiB boundary: bin 0
    add(read(12), b"noref", [hit("12I", pos=77777)])                                           # nothing consumes the reference: end = pos + 1
    add(read(600), b"wide", [hit("1M1I" * 299 + "2M", flag=0x10)])                             # more operations than one lane is given
    return per_read, seqs, names


@pytest.mark.parametrize("hardclip", [0, 1])
def test_rec_host_build_against_layout(host_exe, tmp_path, hardclip):
    """dev_rec.h on the host, one lane: the stream equals the restated layout byte for byte, exactly sized buffers, no sanitizer report; and the cases the
    input is there for"""
    per_read, seqs, names = synthetic(hardclip, 11 + hardclip)
    h = ru.hits_from_lists(per_read)
    exp = ru.records_from_hits(h, seqs, names, hardclip)
    # the input covers what it is meant to cover
    flags = [f for f in h["flag"]]
    assert any(f & 0x10 for f in flags) and any(not f & 0x10 for f in flags)
    ops = {ru.OPS[w & 15] for w in h["cigar"]}
    assert {"M", "I", "D"} <= ops and ("H" if hardclip else "S") in ops
    kinds = set()
    l_seqs = set()
    for i, hits in enumerate(per_read):
        for r in hits:
            o = [ru.OPS[w & 15] for w in r["cigar"]]
            c = "H" if hardclip else "S"
            kinds.add((o[0] == c, o[-1] == c))
            l_seqs.add(ru.clip_window(r["cigar"], len(seqs[i]), hardclip)[1])
    assert kinds == {(False, False), (True, False), (False, True), (True, True)}
    assert set(L_SEQS) <= l_seqs
    assert {1, 254} <= {len(x) for x in names}
    assert any(not hits and i and per_read[i - 1] and i + 1 < len(per_read) and per_read[i + 1] for i, hits in enumerate(per_read))
    span = per_read[names.index(b"span")][0]
    assert ru.reg2bin(span["pos"], span["pos"] + 20) != ru.reg2bin(span["pos"], ru.end_pos(span["pos"], span["cigar"])) and span["pos"] >> 14 != (ru.end_pos(span["pos"], span["cigar"]) - 1) >> 14
    b0 = per_read[names.index(b"bin0")][0]
    assert ru.reg2bin(b0["pos"], ru.end_pos(b0["pos"], b0["cigar"])) == 0
    assert any(c not in b"ACGT" for s in seqs for c in s)
    starts = [0]
    for r in exp:
        starts.append(starts[-1] + len(r))
    assert {s % 4 for s in starts[:-1]} == {0, 1, 2, 3}
    image, out = tmp_path / "image.bin", tmp_path / "stream.bin"
    ru.write_image(image, h, seqs, names, hardclip)
    lines = run_host(host_exe, image, out)
    assert lines[0] == "ok %d %d" % (len(exp), starts[-1]), lines[0]
    assert [int(x) for x in lines[1].split()] == starts
    got = out.read_bytes()
    for k, r in enumerate(exp):
        assert got[starts[k]:starts[k + 1]] == r, "record %d differs" % k
    assert got == b"".join(exp)


def test_rec_pack_seq_is_the_reference_map():
    """the restatement itself: A C G T = 1 2 4 8, anything else 15, lower case not folded; reverse = backwards with A and T swapped only; odd length pads with 0"""
    assert ru.pack_seq(b"ACGTN", False) == bytes([0x12, 0x48, 0xf0])
    assert ru.pack_seq(b"ACGTN", True) == bytes([0xf1, 0x42, 0x80])
    assert ru.pack_seq(b"acgt", False) == bytes([0xff, 0xff])


@pytest.mark.parametrize("case", ["name255", "ops65536", "xa", "window", "host"])
def test_rec_host_build_refusals(host_exe, tmp_path, case):
    """what the host path truncates or asserts on is refused with the C-ABI's code, and names the read"""
    rng = random.Random(3)
    mk = lambda L: "".join(rng.choice("ACGT") for _ in range(L)).encode()
    base = dict(rid=0, pos=100, flag=0, mapq=60, score=30, nm=0, na=1)
    seqs, names, per_read = [mk(30), mk(30), mk(30)], [b"a", b"b", b"c"], [[dict(base, cigar=ru.cig("30M"))], [], [dict(base, cigar=ru.cig("30M"))]]
    hardclip, xa, on_device, want = 0, False, True, None
    if case == "name255":
        names[2] = b"n" * 255
        want = (-5, 1, 2)
    elif case == "ops65536":
        seqs[2] = mk(65536)
        per_read[2] = [dict(base, cigar=ru.cig("1M1I" * 32768))]
        want = (-5, 2, 2)
    elif case == "xa":
        xa, want = True, (-5, 5, -1)
    elif case == "window":
        hardclip = 1
        per_read[0] = [dict(base, cigar=ru.cig("5H30M"))]          # the window passes the 30-base read
        want = (-1, 3, 0)
    else:
        on_device, want = False, (-1, 4, -1)
    image, out = tmp_path / "image.bin", tmp_path / "stream.bin"
    ru.write_image(image, ru.hits_from_lists(per_read), seqs, names, hardclip, xa=xa, on_device=on_device)
    lines = run_host(host_exe, image, out)
    assert lines[0] == "refused %d %d %d" % want, lines
    assert not out.exists()


def test_rec_host_build_on_real_hits(host_exe, orc, golden_dir, tmp_path):
    """the same bodies on what the aligner really produces: the CPU oracle's hits (bit-identical to the GPU path's) for fixture reads, reads cut from tiny.fa
    with clips and secondaries, a 70 000 bp read whose record spans 50 tiles and a read whose CIGAR has hundreds of operations"""
    from tests import fml_util
    from tests.test_gpu_rec import constructed_reads
    L = open(os.path.join(golden_dir, "sim1_bcr.head3000.fq")).read().split("\n")
    reads = [(L[i][1:].split()[0], L[i + 1]) for i in range(0, 4 * 400, 4)] + constructed_reads()
    g = fml_util.fixture_genome()["abl"].decode().upper()
    reads.append(("contig70k", g[20000:50000] + "ACG" + g[50000:89997]))
    reads.append(("gappy", "".join(g[100000 + i:100000 + i + 59] for i in range(0, 20000, 60))))
    names, seqs = [n.encode() for n, _ in reads], [s.encode() for _, s in reads]
    oidx = orc.Index.load(os.path.join(golden_dir, "tiny.fa"))
    for hardclip in (0, 1):
        h = orc.align_batch(orc.default_opt(), oidx, seqs, bool(hardclip), 0.9, 10)
        assert max(h["n_cigar"]) > 256 and any(f & 0x100 for f in h["flag"]) and any((w & 15) == (5 if hardclip else 4) for w in h["cigar"])
        exp = b"".join(ru.records_from_hits(h, seqs, names, hardclip))
        assert len(exp) > 70000 + 50 * 2048
        image, out = tmp_path / ("real%d.bin" % hardclip), tmp_path / ("real%d.stream" % hardclip)
        ru.write_image(image, h, seqs, names, hardclip)
        lines = run_host(host_exe, image, out)
        assert lines[0] == "ok %d %d" % (h["n_hits"], len(exp)), lines[0]
        assert out.read_bytes() == exp
