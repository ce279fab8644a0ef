"""SeqLib::RecordEditor and RefGenome::WriteNmMd through the headers only (tests/cpp/edit_api_test.cpp): the program compiles with -Wall -Werror and links; without
a GPU the four host calls BamRecord gained (RemoveTag, RemoveAllTags, ClearSeqQualAndTags, GetFloatTag) are held against hand-written bytes and the plan's
refusals arrive as std::invalid_argument; on the GPU BamReader -> RecordEditor -> BamWriter(UseGpu) is compared record for record with the host loop Next() +
RemoveTag / AddZTag / AddIntTag + WriteRecord (whole file, SetRegions, SetReadFilter), and WriteNmMd with NmMd + the host calls; both against the Python
statement of tests/edit_util.py too."""
import os
import struct
import subprocess

import pytest

from tests import bam_util as bu
from tests import edit_util as eu
from tests import ref_util as ru

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    import __graft_entry__ as g
    lib = os.path.join(ROOT, "seqlib_amd")
    if not os.path.exists(os.path.join(lib, "libseqlib_amd.so")):
        g.build()
    out = str(tmp_path_factory.mktemp("editapi") / "edit_api_test")
    subprocess.check_call(["g++", "-std=c++17", "-O2", "-Wall", "-Werror", "-I" + os.path.join(ROOT, "include"), os.path.join(ROOT, "tests", "cpp", "edit_api_test.cpp"), "-o", out,
                           "-L" + lib, "-lseqlib_amd", "-Wl,-rpath," + lib, "-lz", "-lpthread"])
    return out


def with_bin(rec):
    """the record with the bin of its alignment span (SAMv1 5.3): the host writer computes it afresh from pos and the CIGAR, the editor keeps the bytes it is given,
    and the generated records carry the bin of a stand-in CIGAR"""
    pos, l_name, n_cig = struct.unpack_from("<i", rec, 8)[0], rec[12], struct.unpack_from("<H", rec, 16)[0]
    words = struct.unpack_from("<%dI" % n_cig, rec, 36 + l_name)
    span = [w >> 4 for w in words if (w & 15) in (0, 2, 3, 7, 8)]
    end = pos + sum(span) if span else pos + 1
    return rec[:14] + struct.pack("<H", bu.reg2bin(pos, end) & 0xffff) + rec[16:]


@pytest.fixture(scope="module")
def sorted_bam(tmp_path_factory):
    """the record cases and generated records with generated aux areas over three contigs, coordinate-sorted and indexed; the FASTA of the contigs"""
    from seqlib_amd import bamio
    contigs = ru.bulk_contigs()
    tid = lambda r: struct.unpack_from("<i", r, 4)[0]
    pos = lambda r: struct.unpack_from("<i", r, 8)[0]
    recs = [r for _, r in eu.REC_CASES] + [r for r in eu.bulk_records(n=700) if len(r) < 3000]
    recs = sorted((with_bin(r) for r in recs if (0 <= tid(r) < 3 and pos(r) >= 0) or tid(r) < 0), key=lambda r: (tid(r) & 0xffffffff, pos(r)))
    d = tmp_path_factory.mktemp("editbam")
    refs = [("c%d" % i, len(c)) for i, c in enumerate(contigs)]
    text = "@HD\tVN:1.6\tSO:coordinate\n" + "".join("@SQ\tSN:%s\tLN:%d\n" % x for x in refs)
    (d / "in.bam").write_bytes(bu.bam_bytes(text, refs, recs, member_size=3000))
    (d / "ref.fa").write_bytes(ru.fasta([(b"c%d" % i, c) for i, c in enumerate(contigs)], 80))
    bamio.index_build(d / "in.bam")
    return d, contigs, recs


def test_host_calls_without_a_gpu(exe):
    r = subprocess.run([exe, "host"], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and r.stdout == "edit api host OK\n", r.stdout[-2000:] + r.stderr[-2000:]


def test_the_host_loop_equals_python(exe, tmp_path):
    """the loop the GPU path is compared with, on its own: RemoveTag / AddZTag / AddIntTag over the record cases and generated records give the Python statement"""
    recs = [r for _, r in eu.REC_CASES] + [r for r in eu.bulk_records(n=700) if len(r) < 3000]
    (tmp_path / "in.bin").write_bytes(b"".join(recs))
    r = subprocess.run([exe, "hostloop", str(tmp_path / "in.bin"), str(tmp_path / "out.bin")], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and r.stdout == "edit api hostloop OK %d\n" % len(recs), r.stdout[-2000:] + r.stderr[-2000:]
    plan = eu.Plan(drops=[b"XA", b"SA"], adds=[(b"RG", "Z", b"grp1", False), (b"XN", "i", 7, False), (b"NM", "i", 3, True)])
    assert (tmp_path / "out.bin").read_bytes() == b"".join(eu.apply_batch(recs, plan))


@pytest.mark.gpu
@pytest.mark.parametrize("how", ["all", "regions", "filter"])
def test_editor_equals_the_host_loop(exe, sl, sorted_bam, how):
    d, contigs, recs = sorted_bam
    gpu, host = d / ("gpu_%s.bam" % how), d / ("host_%s.bam" % how)
    r = subprocess.run([exe, "edit", str(d / "in.bam"), str(gpu), str(host), how], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and r.stdout.startswith("edit api edit OK "), r.stdout[-2000:] + r.stderr[-3000:]
    got = [x["raw"] for x in bu.parse_bam(gpu.read_bytes())[2]]
    want = [x["raw"] for x in bu.parse_bam(host.read_bytes())[2]]
    assert len(got) == int(r.stdout.split()[-1]) > 100 and got == want
    plan = eu.Plan(drops=[b"XA", b"SA"], adds=[(b"RG", "Z", b"grp1", False), (b"XN", "i", 7, False), (b"NM", "i", 3, True)])
    if how == "all":
        assert got == eu.apply_batch(recs, plan)
    else:
        model = set(eu.apply_batch(recs, plan))
        assert len(got) < len(recs) and all(g in model for g in got)


@pytest.mark.gpu
def test_write_nm_md_equals_nm_md_and_the_host_calls(exe, sl, sorted_bam):
    d, contigs, recs = sorted_bam
    gpu, host = d / "gpu_calmd.bam", d / "host_calmd.bam"
    r = subprocess.run([exe, "calmd", str(d / "ref.fa"), str(d / "in.bam"), str(gpu), str(host)], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and r.stdout == "edit api calmd OK %d\n" % len(recs), r.stdout[-2000:] + r.stderr[-3000:]
    got = [x["raw"] for x in bu.parse_bam(gpu.read_bytes())[2]]
    assert got == [x["raw"] for x in bu.parse_bam(host.read_bytes())[2]]
    nm_md = [ru.nm_md(x, contigs) for x in recs]
    plan = eu.Plan(drops=[b"XA"], adds=[(b"NM", "ic", -1, True), (b"MD", "Zc", None, False)])
    assert got == eu.apply_batch(recs, plan, {0: [nm for nm, _ in nm_md], 1: [md for _, md in nm_md]})
    assert sum(nm >= 0 for nm, _ in nm_md) > 300 and sum(nm < 0 for nm, _ in nm_md) > 5
