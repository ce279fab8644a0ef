"""CPU tests of the BGZF writer path (include/seqlib_amd_bam.h slx_bgzf_*, seqlib_amd/csrc/slx_bgzf.hip, dev_deflate.h): the exports, the refusal without a
GPU, the host-compiled DEFLATE encoder body against zlib under ASan + UBSan, the code-length builder alone, and SeqLib::BamWriter's unchanged host path
next to its GPU opt-in.  No test here needs a GPU."""
import os
import re
import struct
import subprocess

import pytest

from tests import bam_util as bu
from tests import bgzf_payloads as bp
from tests.test_sanitizers import ENV, SAN

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def ffi():
    import __graft_entry__ as g
    if not os.path.exists(os.path.join(ROOT, "seqlib_amd", "libseqlib_amd.so")):
        g.build()
    from seqlib_amd import _ffi
    _ffi.lib()
    return _ffi


def test_bgzf_exports_match_header(ffi):
    from seqlib_amd import bamio
    hdr = open(os.path.join(ROOT, "include", "seqlib_amd_bam.h")).read()
    body = hdr[hdr.index("extern \"C\""):]
    declared = set(re.findall(r"\b(slx_bgzf_[a-z0-9_]+)\s*\(", body))
    assert declared == set(bamio.BGZF_EXPORTS) and len(declared) == 7, declared ^ set(bamio.BGZF_EXPORTS)
    L = bamio.lib()
    for name in declared:
        assert hasattr(L, name), name
    head = hdr[:hdr.index("#ifndef")]
    for name in ("slx_bgzf_open", "slx_bgzf_write", "slx_bgzf_write_device", "slx_bgzf_flush", "slx_bgzf_close"):
        assert name in head
    assert "src/BamWriter.cpp" in head and "hts_open" in head and "sam_write1" in head
    assert not any(e.startswith("slx_bgzf_") for e in bamio.EXPORTS + ffi.EXPORTS)


def test_bgzf_no_gpu_fails_loudly(ffi, tmp_path):
    import torch
    if torch.cuda.is_available():
        pytest.skip("GPU present")
    from seqlib_amd import bamio
    p = tmp_path / "out.bam"
    with pytest.raises(ffi.SlxError) as e:
        bamio.Writer(p)
    assert e.value.code == ffi.SLX_ENODEVICE and "no CPU fallback" in str(e.value)
    assert not p.exists()


@pytest.fixture(scope="module")
def host_exe(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("deflate") / "deflate_host_test")
    subprocess.check_call(["g++", "-std=c++17"] + SAN + ["-Wall", "-Wno-unknown-pragmas", "-o", exe, os.path.join(ROOT, "tests", "cpp", "deflate_host_test.cpp"), "-lz"])
    return exe


def run_host(exe, *args):
    r = subprocess.run([exe] + [str(a) for a in args], capture_output=True, text=True, env=ENV, timeout=600)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    assert "runtime error" not in r.stderr and "AddressSanitizer" not in r.stderr, r.stderr[-3000:]
    last = r.stdout.strip().splitlines()[-1].split()
    assert last[1] == "checked" and int(last[2]) == 0, r.stdout[-2000:]
    return r.stdout.strip().splitlines(), int(last[0])


def test_deflate_host_build_against_zlib(host_exe, tmp_path):
    """dev_deflate.h on the host, one lane: every member of P1..P5 inflated by zlib and compared, exactly sized buffers, no sanitizer report; and the size
    conditions the payloads are there for"""
    names, f = [], tmp_path / "members.bin"
    with open(f, "wb") as fh:
        for name, p in bp.everything():
            for i, b in enumerate(bp.blocks(p)):
                fh.write(struct.pack("<I", len(b)) + b)
                names.append((name, i))
    lines, checked = run_host(host_exe, "members", f)
    assert checked == len(names)
    rows = {}
    for key, line in zip(names, lines):
        n, out, stored, ntok, nmatch, maxlen, maxdist = (int(x) for x in line.split())
        rows[key] = dict(n=n, out=out, stored=stored, ntok=ntok, nmatch=nmatch, maxlen=maxlen, maxdist=maxdist)
    total = lambda name: sum(r["out"] for k, r in rows.items() if k[0] == name)
    for (name, i), r in rows.items():
        assert r["out"] <= 5 + r["n"] and r["maxdist"] <= 32768 and r["maxlen"] <= 258
        if name.startswith("p1/random/"):                                   # random blocks come out stored
            assert r["stored"] == 1 and r["out"] == 5 + r["n"], (name, r)
    assert rows["p2/dist32768", 0]["maxdist"] == 32768                      # the repeat at the cap is used ...
    assert rows["p2/dist32769", 0]["maxdist"] <= 32768                      # ... one byte further it is not (zlib refuses a longer distance, too)
    assert rows["p3/abc", 0]["maxlen"] == 258 and rows["p3/abc", 0]["stored"] == 0 and rows["p3/abc", 0]["out"] < 600
    assert rows["p3/run", 0]["maxlen"] == 258 and rows["p3/run", 0]["nmatch"] >= 3
    assert total("p3/zeros200k") < 200000 // 100
    assert rows["p4/fib", 0]["stored"] == 0 and rows["p4/fib", 0]["out"] < 46367 // 2
    fq = bp.p5_fastq()
    fixed, huff = bp.zlib_total(fq, level=6, strategy=bu.zlib.Z_FIXED), bp.zlib_total(fq, level=6, strategy=bu.zlib.Z_HUFFMAN_ONLY)
    print("p5/fastq: encoder %d, zlib fixed %d, huffman-only %d, level 1 %d, level 6 %d" % (total("p5/fastq"), fixed, huff, bp.zlib_total(fq, level=1), bp.zlib_total(fq, level=6)))
    assert total("p5/fastq") < min(fixed, huff)


def test_deflate_host_build_seeded_sweep(host_exe):
    """300 seeded payloads of 0..70 000 bytes, alphabets of 1, 2, 4, 16 and 256 symbols, planted repeats: zlib inflates each member to the input"""
    lines, checked = run_host(host_exe, "sweep", 300)
    assert checked >= 300
    m = re.match(r"sweep: (\d+) bytes in, (\d+) out", lines[-2])
    assert m and int(m.group(2)) < int(m.group(1))


def test_code_length_builder(host_exe):
    """def_code_lengths alone on Fibonacci frequencies (286 and 30 symbols with limit 15, 19 with limit 7): every length within the limit, the Kraft sum exactly
    1, a zero frequency a zero length, one used symbol still a complete code"""
    lines, checked = run_host(host_exe, "lengths")
    assert checked == 21


def compile_test(tmp, name):
    out = str(tmp / name)
    lib = os.path.join(ROOT, "seqlib_amd")
    subprocess.check_call(["g++", "-std=c++17", "-O2", "-Wall", "-Werror", "-I" + os.path.join(ROOT, "include"), os.path.join(ROOT, "tests", "cpp", name + ".cpp"), "-o", out,
                           "-L" + lib, "-lseqlib_amd", "-Wl,-rpath," + lib, "-lz", "-lpthread"])
    return out


def test_cpp_writer_refuses_without_gpu(ffi, tmp_path):
    import torch
    if torch.cuda.is_available():
        pytest.skip("GPU present")
    r = subprocess.run([compile_test(tmp_path, "bam_writer_host_test"), "refuse", str(tmp_path)], capture_output=True, text=True)
    assert r.returncode == 0 and r.stdout.strip() == "refuse OK", r.stdout + r.stderr
    assert "no HIP device" in r.stderr and "BamWriter::UseGpu - call it before Open()" in r.stderr and r.stderr.count("only BAM output") == 2
    assert not (tmp_path / "gpu.bam").exists()
    assert len(bu.parse_bam((tmp_path / "late.bam").read_bytes())[2]) == 1


def test_cpp_host_writer_is_unchanged(ffi, tmp_path):
    """without UseGpu the writer's bytes are zlib level 6 of the stream cut at 0xff00, the header in members of its own: rebuilt here with Python's zlib"""
    r = subprocess.run([compile_test(tmp_path, "bam_writer_host_test"), "host", str(tmp_path)], capture_output=True, text=True)
    assert r.returncode == 0 and r.stdout.startswith("host OK 1500"), r.stdout + r.stderr
    raw = (tmp_path / "one.bam").read_bytes()
    text, refs, recs = bu.parse_bam(raw)
    assert len(recs) == 1500 and refs == bu.REFS
    stream = bu.inflate_all(raw)
    n_head = len(stream) - sum(len(x["raw"]) for x in recs)
    assert raw == bu.bgzf_bytes(stream[:n_head], eof=False, level=6) + bu.bgzf_bytes(stream[n_head:], eof=True, level=6)
    assert (tmp_path / "many.bam").read_bytes() == raw
