"""The host side of the SAM writer, without a GPU: the exports, slx_samw_format_record against the Python statement of the rules (tests/samw_util.py), and
samw_host.h / dev_samw.h's per-record body under sanitizers in a stand-alone program (tests/cpp/samw_host_test.cpp)."""
import ctypes as C
import os
import re
import subprocess

import pytest

import seqlib_amd  # noqa: F401  (the package must import)
from seqlib_amd import _ffi, samwio
from tests import bam_util as bu
from tests import samw_util as wu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
REF_NAMES = [n for n, _ in bu.REFS]


def test_header_declares_exactly_the_exports():
    text = open(os.path.join(ROOT, "include", "seqlib_amd_samw.h")).read()
    body = text[text.index("#ifndef SEQLIB_AMD_SAMW_H"):]
    declared = re.findall(r"^\s*(?:int|void|int64_t|const char \*)\s+\*?(slx_\w+)\s*\(", body, re.M)
    assert sorted(declared) == sorted(samwio.SAMW_EXPORTS)
    assert all(n.startswith("slx_samw_") for n in declared)
    L = samwio.lib()
    for n in samwio.SAMW_EXPORTS:
        assert hasattr(L, n), n


def test_open_without_a_gpu_is_enodevice(tmp_path):
    import torch
    if torch.cuda.is_available():
        pytest.skip("a GPU is present: tests/test_gpu_samw.py opens writers")
    p = tmp_path / "a.sam"
    with pytest.raises(_ffi.SlxError) as e:
        samwio.Writer(p)
    assert e.value.code == _ffi.SLX_ENODEVICE and not p.exists()


def test_the_case_list_covers_what_it_claims():
    names = [c[0] for c in wu.CASES]
    assert len(set(names)) == len(names)
    lines = {n: wu.record_to_line(r, bu.REFS) for n, r, ok in wu.CASES if ok}
    assert lines["unmapped"] == b"r\t4\t*\t0\t0\t*\t*\t0\t0\tACGT\tIIII\n"
    assert lines["l_seq_0"].split(b"\t")[9:] == [b"*", b"*\n"]
    assert lines["mate_same"].split(b"\t")[6:9] == [b"=", b"2147483647", b"-1"]
    assert lines["cigar_op_codes_9_to_15"].split(b"\t")[5] == b"5B6?7M"
    assert lines["aux_f_1"].endswith(b"XF:f:-0\n") and lines["aux_f_4"].endswith(b"XF:f:inf\n") and lines["aux_f_5"].endswith(b"XF:f:nan\n")
    assert lines["aux_f_2"].endswith(b"XF:f:0.001\n") and lines["aux_f_3"].endswith(b"XF:f:3.4e+38\n")
    assert lines["stray_3"] == lines["stray_1"] == wu.record_to_line(wu.make(aux=b"NMC\x05"), bu.REFS)
    assert set("".join(l.split(b"\t")[9].decode() for l in lines.values())) >= set(bu.SEQ_CODES)
    assert sum(not ok for _, _, ok in wu.CASES) >= 20


@pytest.mark.parametrize("name,rec,ok", wu.CASES, ids=[c[0] for c in wu.CASES])
def test_format_record_equals_python(name, rec, ok):
    if ok:
        assert samwio.format_record(rec, REF_NAMES) == wu.record_to_line(rec, bu.REFS)
    else:
        with pytest.raises(wu.SamwError):
            wu.record_to_line(rec, bu.REFS)
        with pytest.raises(_ffi.SlxError) as e:
            samwio.format_record(rec, REF_NAMES)
        assert e.value.code == _ffi.SLX_EIO


def test_format_record_on_the_sample_records():
    recs = bu.sample_records(400)
    got = [samwio.format_record(r, REF_NAMES) for r in recs]
    assert got == [wu.record_to_line(r, bu.REFS) for r in recs]
    # no floating-point fields there: the line is sam_util's, which the SAM reader's tests read back
    from tests import sam_util as su
    assert got == [su.record_to_line(r, bu.REFS) + b"\n" for r in recs]


def test_small_buffer_returns_the_size_needed():
    rec = wu.make(aux=b"XZZhello\0")
    want = wu.record_to_line(rec, bu.REFS)
    arr = (C.c_char_p * 3)(*[x.encode() for x in REF_NAMES])
    n = C.c_int64(0)
    buf = C.create_string_buffer(8)
    assert samwio.lib().slx_samw_format_record(rec, len(rec), arr, 3, buf, 8, C.byref(n)) == _ffi.SLX_EINVAL
    assert n.value == len(want)
    buf = C.create_string_buffer(len(want))
    assert samwio.lib().slx_samw_format_record(rec, len(rec), arr, 3, buf, len(want), C.byref(n)) == _ffi.SLX_OK and buf.raw == want


def test_host_formatter_and_kernel_body_under_sanitizers(tmp_path):
    """samw_host.h and the host build of dev_samw.h's per-record body (size, then fill) over the case list, whole and truncated at every byte with block_size
    adjusted: the lines of the Python statement or a refusal, no sanitizer report"""
    exe = str(tmp_path / "samw_host_test")
    subprocess.check_call(["g++", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-fno-omit-frame-pointer", "-g", "-O1", "-Wall", "-Werror",
                           "-I" + os.path.join(ROOT, "seqlib_amd", "csrc"), os.path.join(ROOT, "tests", "cpp", "samw_host_test.cpp"), "-o", exe])
    exp = str(tmp_path / "expect.bin")
    wu.dump_expectations(exp)
    r = subprocess.run([exe, exp], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    assert "samw_host_test OK: %d cases" % len(wu.CASES) in r.stdout
