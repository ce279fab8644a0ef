"""The FASTQ reader without a GPU: the serial parser of the slow path (seqlib_amd/csrc/fq_host.h) and the fast path's per-record test (dev_fastq.h) as a
stand-alone program under ASan + UBSan, the Python statement of the grammar (tests/fastq_util.py) against the GetNextSequence loop, and the C-ABI's surface."""
import os
import re
import subprocess

import pytest

from tests import fastq_util

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CASES = fastq_util.cases()


def test_host_parser_and_record_test_under_sanitizers(tmp_path):
    """fqh_parse over every case, whole and fed chunks cut at every byte position of the small ones, and fq_check over the line table of every such prefix:
    the records of the Python statement, no sanitizer report"""
    exe = str(tmp_path / "fastq_host_test")
    subprocess.check_call(["g++", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-fno-omit-frame-pointer", "-g", "-O1", "-Wall", "-Werror",
                           "-I" + os.path.join(ROOT, "seqlib_amd", "csrc"), os.path.join(ROOT, "tests", "cpp", "fastq_host_test.cpp"), "-o", exe])
    exp = str(tmp_path / "expect.bin")
    fastq_util.dump_expectations(exp, CASES)
    r = subprocess.run([exe, exp], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "fastq_host_test OK: %d cases" % len(CASES) in r.stdout


def test_case_list_covers_what_it_names():
    by = {n: (t, s) for n, t, s in CASES}
    assert len(by) == len(CASES)
    lens = sorted({len(r[2]) for r in fastq_util.parse(by["lengths"][0])[0]})
    assert lens == [1, 15, 16, 17, 2047, 2048, 2049, 5000]
    assert [len(by["size%+d" % d][0]) % 64 for d in (-1, 0, 1)] == [63, 0, 1]
    assert [by["line_end%+d" % d][0].index(b"\n") for d in (-1, 0, 1)] == [63, 64, 65]
    assert not by["no_final_newline"][0].endswith(b"\n")
    for n in ("truncated_qual", "long_qual_mid", "truncated_qual_crlf", "long_qual_mid_crlf"):
        recs, bad = fastq_util.parse(by[n][0])
        assert bad and len(recs) == 2
    assert len(fastq_util.parse(by["one_multiline_mid"][0])[0]) == fastq_util.ONE_MULTILINE_MID_BEFORE + 6
    for n, (t, strict) in by.items():
        if strict and t:
            assert all(r[4] & 2 and len(r[2]) >= 1 for r in fastq_util.parse(t)[0]), n


@pytest.fixture(scope="module")
def api_exe(tmp_path_factory):
    import __graft_entry__ as g
    if not os.path.exists(os.path.join(ROOT, "seqlib_amd", "libseqlib_amd.so")):
        g.build()
    out = str(tmp_path_factory.mktemp("fq") / "seqlib_api_test")
    lib = os.path.join(ROOT, "seqlib_amd")
    subprocess.check_call(["g++", "-std=c++17", "-O2", "-I" + os.path.join(ROOT, "include"), os.path.join(ROOT, "tests", "cpp", "seqlib_api_test.cpp"), "-o", out,
                           "-L" + lib, "-lseqlib_amd", "-Wl,-rpath," + lib, "-lz", "-lpthread"])
    return out


@pytest.mark.parametrize("form", ["plain", "gzip"])
def test_python_statement_matches_getnextsequence(api_exe, tmp_path, form):
    """record for record the dump of the `while (r.GetNextSequence(s))` loop, which stops at the same record on the error cases.  The dump reuses one
    UnalignedSequence, but parse_record() clears its comment and quality per record and GetNextSequence assigns them from the first record on that has one,
    so a line is name, comment, sequence, quality of that record -- an empty quality for a read without a '+' block."""
    for name, text, _ in CASES:
        p = tmp_path / (name + ".fq")
        p.write_bytes(fastq_util.gzip_(text) if form == "gzip" else text)
        r = subprocess.run([api_exe, "fastq", str(p)], capture_output=True)
        assert r.returncode == 0, (name, r.stderr)
        recs, _ = fastq_util.parse(text)
        exp = b"".join(b"\t".join((nm, com, seq, qual if flag & 2 else b"")) + b"\n" for nm, com, seq, qual, flag in recs)
        assert r.stdout == exp, name


def test_golden_file_is_strict(golden_dir):
    text = open(os.path.join(golden_dir, "sim1_bcr.head3000.fq"), "rb").read()
    recs, bad = fastq_util.parse(text)
    assert len(recs) == 3000 and not bad and text.count(b"\n") == 12000


def test_abi_surface():
    """every function the header declares is exported and bound; a missing file is SLX_EIO before any device is asked for"""
    import ctypes as C
    from seqlib_amd import _ffi, fastqio
    hdr = open(os.path.join(ROOT, "include", "seqlib_amd_fastq.h")).read()
    declared = sorted(set(re.findall(r"\b(slx_fastq_[a-z_]+)\s*\(", hdr[hdr.index("extern \"C\""):])))
    assert declared == sorted(fastqio.FASTQ_EXPORTS)
    L = fastqio.lib()
    for s in declared:
        assert hasattr(L, s), s
    h = C.c_void_p()
    assert L.slx_fastq_open(b"/nonexistent/dir/x.fq", -1, C.byref(h)) == _ffi.SLX_EIO and not h
    assert b"missing" in L.slx_last_error()
    assert L.slx_fastq_counter(None, b"reads") == -1
