"""The host side of the SAM reader, without a GPU: the header's names, slx_sam_sniff, slx_sam_parse_line against the Python statement of the grammar
(tests/sam_util.py), and sam_host.h / dev_sam.h's per-line body under sanitizers in a stand-alone program (tests/cpp/sam_host_test.cpp)."""
import os
import re
import subprocess

import pytest

import seqlib_amd  # noqa: F401  (the package must import)
from seqlib_amd import _ffi, samio
from tests import bam_util as bu
from tests import fastq_util
from tests import sam_util as su

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
REF_NAMES = [n for n, _ in bu.REFS]


def test_header_declares_exactly_the_exports():
    text = open(os.path.join(ROOT, "include", "seqlib_amd_sam.h")).read()
    body = text[text.index("#ifndef SEQLIB_AMD_SAM_H"):]
    declared = re.findall(r"^\s*(?:int|void|int64_t|const char \*)\s+\*?(slx_\w+)\s*\(", body, re.M)
    assert sorted(declared) == sorted(samio.SAM_EXPORTS)
    assert all(n.startswith("slx_sam_") for n in declared)
    L = samio.lib()
    for n in samio.SAM_EXPORTS:
        assert hasattr(L, n), n


def test_open_without_a_gpu_is_enodevice(tmp_path):
    import torch
    if torch.cuda.is_available():
        pytest.skip("a GPU is present: tests/test_gpu_sam.py opens SAM files")
    p = tmp_path / "a.sam"
    p.write_bytes(su.sam_text(bu.TEXT, su.canonical(3)[0]))
    with pytest.raises(_ffi.SlxError) as e:
        samio.Reader(p)
    assert e.value.code == _ffi.SLX_ENODEVICE


def test_sniff(tmp_path):
    lines, _ = su.canonical(20)
    sam = su.sam_text(bu.TEXT, lines)
    files = {
        "a.bam": (bu.bam_bytes(bu.TEXT, bu.REFS, bu.sample_records(20)), 0),
        "a.sam": (sam, 1),
        "a.sam.gz": (fastq_util.gzip_(sam), 1),
        "a.sam.bgz": (bu.bgzf_bytes(sam, 300), 1),
        "headerless.sam": (su.sam_text("", lines), 1),
        "header_only.sam": (bu.TEXT.encode(), 1),
        "junk.bin": (bytes(range(256)) * 4, None),
        "junk.txt": (b"just some words\nand more\n", None),
        "junk.gz": (fastq_util.gzip_(b"\x00\x01\x02 not a SAM"), None),
        "cram.cram": (b"CRAM\x03\x00" + bytes(40), None),
        "empty": (b"", None),
    }
    for name, (data, want) in files.items():
        p = tmp_path / name
        p.write_bytes(data)
        if want is None:
            with pytest.raises(_ffi.SlxError) as e:
                samio.sniff(p)
            assert e.value.code == _ffi.SLX_EIO, name
        else:
            assert samio.sniff(p) == want, name
    with pytest.raises(_ffi.SlxError) as e:
        samio.sniff(tmp_path / "missing.sam")
    assert e.value.code == _ffi.SLX_EIO


@pytest.mark.parametrize("name,line,ok", su.CASES, ids=[c[0] for c in su.CASES])
def test_parse_line_equals_python(name, line, ok):
    if ok:
        assert samio.parse_line(line, REF_NAMES) == su.line_to_record(line, bu.REFS)
    else:
        with pytest.raises(su.SamError):
            su.line_to_record(line, bu.REFS)
        with pytest.raises(_ffi.SlxError) as e:
            samio.parse_line(line, REF_NAMES)
        assert e.value.code == _ffi.SLX_EIO


def test_parse_line_on_the_canonical_fixture():
    lines, recs = su.canonical(400)
    assert [samio.parse_line(l, REF_NAMES) for l in lines] == recs
    # integer aux come back in the smallest type: the expectation is the Python parser's, not the input's bytes
    assert recs != bu.sample_records(400)
    assert [su.record_to_line(r, bu.REFS) for r in recs] == lines


def test_long_cigar_message_and_small_buffer():
    line = su._l(cigar=b"1M" * 65536, seq=b"A" * 65536, qual=b"*")
    with pytest.raises(su.SamError, match="CG:B"):
        su.line_to_record(line, bu.REFS)
    with pytest.raises(_ffi.SlxError, match="CG:B"):
        samio.parse_line(line, REF_NAMES)
    ok = su._l(cigar=b"1M" * 65535, seq=b"A" * 65535, qual=b"*")
    assert samio.parse_line(ok, REF_NAMES) == su.line_to_record(ok, bu.REFS)
    import ctypes as C
    n = C.c_int64(0)
    buf = C.create_string_buffer(8)
    arr = (C.c_char_p * 3)(*[x.encode() for x in REF_NAMES])
    assert samio.lib().slx_sam_parse_line(su._l(), len(su._l()), arr, 3, buf, 8, C.byref(n)) == _ffi.SLX_EINVAL
    assert n.value == len(su.line_to_record(su._l(), bu.REFS))


def test_text_level_rules_in_python():
    lines, recs = su.canonical(5)
    for eol, last in ((b"\n", True), (b"\r\n", True), (b"\n", False), (b"\r\n", False)):
        text, refs, got, bad = su.parse_text(su.sam_text(bu.TEXT.replace("\n", eol.decode()), lines, eol, last))
        assert (text, refs, got, bad) == (bu.TEXT.encode(), bu.REFS, recs, None)
    hdr_lines = bu.TEXT.count("\n")
    for where in (0, 2, 4):
        for badline in (b"", b"@CO\tlate", su._l(rname=b"chrZ")):
            if where == 0 and badline[:1] == b"@":          # (before the first record it is one more header line)
                continue
            body = lines[:where] + [badline] + lines[where + 1:]
            text, refs, got, bad = su.parse_text(su.sam_text(bu.TEXT, body))
            assert got == recs[:where] and bad[0] == hdr_lines + where + 1


def test_host_parser_and_kernel_body_under_sanitizers(tmp_path):
    """sam_host.h and the host build of dev_sam.h's per-line body over the case list, whole, truncated at every byte and with every byte replaced by tab, LF, NUL and
    0xff: the records of the Python statement, FAST only where the record equals the host parser's, no sanitizer report"""
    exe = str(tmp_path / "sam_host_test")
    subprocess.check_call(["g++", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-fno-omit-frame-pointer", "-g", "-O1", "-Wall", "-Werror",
                           "-I" + os.path.join(ROOT, "seqlib_amd", "csrc"), os.path.join(ROOT, "tests", "cpp", "sam_host_test.cpp"), "-o", exe])
    exp = str(tmp_path / "expect.bin")
    su.dump_expectations(exp)
    r = subprocess.run([exe, exp], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "sam_host_test OK: %d cases" % len(su.CASES) in r.stdout
