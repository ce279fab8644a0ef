"""The host side of the reference genome unit, without a GPU: the exports, slx_ref_fai_of_text against the recorded samtools index of tests/golden/tiny.fa and
against the Python statement of the rules (tests/ref_util.py) over the FASTA cases, every failing case with its message, slx_ref_record_nm_md over the record cases
and generated records, damaged records, and dev_ref.h's and ref_host.h's bodies under sanitizers in a stand-alone program (tests/cpp/ref_host_test.cpp)."""
import os
import re
import subprocess

import pytest

import seqlib_amd  # noqa: F401  (the package must import)
from seqlib_amd import _ffi, refio
from tests import ref_util as ru

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    """tests/cpp/ref_host_test.cpp under ASan and UBSan: a program of its own, nothing is loaded into Python"""
    out = str(tmp_path_factory.mktemp("ref") / "ref_host_test")
    subprocess.check_call(["g++", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-fno-omit-frame-pointer", "-g", "-O1", "-Wall", "-Werror",
                           "-I" + os.path.join(ROOT, "seqlib_amd", "csrc"), "-I" + os.path.join(ROOT, "include"), os.path.join(ROOT, "tests", "cpp", "ref_host_test.cpp"), "-o", out])
    return out


@pytest.fixture(scope="module")
def bulk():
    contigs = ru.bulk_contigs()
    recs = ru.bulk_records(contigs)
    return contigs, recs, [ru.nm_md(r, contigs) for r in recs]


def test_header_declares_exactly_the_exports():
    text = open(os.path.join(ROOT, "include", "seqlib_amd_ref.h")).read()
    body = text[text.index("#ifndef SEQLIB_AMD_REF_H"):]
    declared = re.findall(r"^\s*(?:int|void|int64_t|const char)\s+\*?(slx_\w+)\s*\(", body, re.M)
    assert sorted(declared) == sorted(refio.REF_EXPORTS)
    assert all(n.startswith("slx_ref_") for n in declared)
    L = refio.lib()
    for n in refio.REF_EXPORTS:
        assert hasattr(L, n), n
    rules = text[:text.index("#ifndef SEQLIB_AMD_REF_H")]
    for word in ("restates", "htslib and samtools are not part of this tree", "NOT pinned", "stale index", "LINEBASES", "33..126", "2^31 - 1", "multiple of 16", "SLX_EIO", "SLX_EINVAL",
                 "ACMGRSVTWYHKDBN", "l_seq", "No CPU fallback"):
        assert word in rules, word
    for what in ru.WHAT.values():          # the sentences of the errors are the library's
        assert what.encode() in open(os.path.join(ROOT, "seqlib_amd", "csrc", "ref_host.h"), "rb").read(), what


def test_tiny_fa_gives_the_recorded_samtools_index():
    text = open(os.path.join(GOLDEN, "tiny.fa"), "rb").read()
    want = open(os.path.join(GOLDEN, "tiny.fa.fai"), "rb").read()
    assert want.split(b"\n")[0] == b"bcr\t141530\t5\t100\t101" and want.count(b"\n") == 4
    assert refio.fai_of_text(text) == want == ru.fai_text(text)


@pytest.mark.parametrize("name", sorted(ru.GOOD))
def test_fasta_case_equals_python(name):
    text = ru.GOOD[name]
    assert len(text) < 700
    assert refio.fai_of_text(text) == ru.fai_text(text)


def test_the_fasta_cases_cover_what_they_claim():
    f = lambda n: [c[:5] for c in ru.contigs_of(ru.GOOD[n])]
    assert f("lf") == [(b"one", 150, 5, 60, 61), (b"two", 47, 163, 47, 48), (b"three", 120, 218, 60, 61)]
    assert f("crlf") == [(b"one", 150, 6, 60, 62), (b"two", 47, 168, 47, 49), (b"three", 120, 225, 60, 62)]
    assert f("no_final_eol") == f("lf") and not ru.GOOD["no_final_eol"].endswith(b"\n")
    assert f("last_line_full")[1] == (b"y", 60, 128, 60, 61)
    assert f("zero_between")[1] == (b"empty", 0, 165, 0, 0) and f("zero_last")[1] == (b"empty", 0, 165, 0, 0) and f("zero_last_no_eol")[1][2] == 164
    assert f("zero_only") == [(b"nothing", 0, 9, 0, 0)]
    assert f("trailing_blank") == f("lf") and f("blank_before_header")[1][:2] == (b"two", 47)
    assert [c[0] for c in f("description")] == [b"chr1", b"chr2"]
    assert f("width_1") == [(b"w1", 9, 4, 1, 2)] and f("cr_at_end_unterminated") == [(b"x", 6, 3, 4, 5)]
    assert ru.contigs_of(ru.GOOD["lower_and_iupac"])[0][5] == b"acgtnACGTNRYKMSWBDHVryk" * 5


@pytest.mark.parametrize("name", sorted(ru.BAD))
def test_failing_fasta_case(name):
    text, what, contig, byte = ru.BAD[name]
    with pytest.raises(ru.FastaError) as pe:
        ru.contigs_of(text)
    assert str(pe.value) == ru.bad_message(name)
    with pytest.raises(_ffi.SlxError) as e:
        refio.fai_of_text(text)
    assert e.value.code == _ffi.SLX_EIO and ru.bad_message(name) in str(e.value)


@pytest.mark.parametrize("name,r", ru.REC_CASES, ids=[n for n, _ in ru.REC_CASES])
def test_record_equals_python(name, r):
    p = ru.parse(r)
    want = ru.nm_md(r, ru.REC_CONTIGS)
    if 0 <= p["tid"] < len(ru.REC_CONTIGS):
        assert refio.record_nm_md(r, ru.REC_CONTIGS[p["tid"]]) == want
    else:
        assert want == (-1, b"")
        if p["tid"] < 0:
            assert refio.record_nm_md(r, ru.REC_CONTIGS[0]) == want


def test_the_record_cases_cover_what_they_claim():
    by = dict(ru.REC_CASES)
    g = lambda n: ru.nm_md(by[n], ru.REC_CONTIGS)
    assert {op for op, _ in ru.parse(by["every_op"])["cig"]} == set(range(16))
    assert g("perfect") == (0, b"20") and g("one_mismatch") == (1, b"9T10") and g("mismatch_first_and_last") == (2, b"0A10G0") and g("all_mismatch")[0] == 6
    assert g("ops_9_to_15_only") == (0, b"0")
    assert g("lead_soft") == g("trail_soft") == g("lead_hard") == g("trail_hard") == g("hard_and_soft_both_ends") == (0, b"10")
    assert g("ins_next_to_mismatch") == (4, b"4T0A4") and g("del_next_to_mismatch") == (4, b"4T0^AC0G4") and g("del_at_start") == (3, b"0^GTA8")
    assert g("del_after_del") == (3, b"2^A0^CG4")
    assert g("n_in_read") == (1, b"4A5") and g("n_in_reference") == (2, b"5N0N5") and g("n_in_both") == (3, b"0T2N0N3")
    assert g("iupac_read") == (3, b"0A3A2T0") and g("eq_in_read") == (0, b"8")
    assert g("lower_case_reference") == (1, b"4N15") and g("lower_case_mismatch_and_del") == (11, b"2G1^ACGT0K0M0S0W0B0D0")
    assert g("off_end_in_m") == (0, b"4") and g("off_end_in_m_with_mismatch") == (1, b"2T0") and g("off_end_in_d") == (3, b"3^CGT0")
    assert g("d_at_the_end_exactly") == (3, b"3^CGT0") and g("d_past_the_end") == (0, b"2^0") and g("pos_at_the_end") == (0, b"0") and g("n_skip_past_the_end") == (0, b"2")
    assert g("cigar_longer_than_read") == (0, b"6") and g("insert_longer_than_read") == (9, b"2") and g("run_of_ten") == (1, b"10G0")
    for n in ("unmapped_flag", "tid_minus_one", "tid_out_of_range", "pos_negative", "no_cigar", "l_seq_0"):
        assert g(n) == (-1, b""), n
    assert len(ru.parse(by["cigar_70_ops"])["cig"]) == 69 and g("cigar_70_ops")[0] >= 34


def test_bulk_records_equal_python(bulk):
    contigs, recs, want = bulk
    lens = [ru.parse(r)["l_seq"] for r in recs]
    assert len(recs) == 2000 and min(lens) == 1 and max(lens) == 20000 and max(len(ru.parse(r)["cig"]) for r in recs) > 64
    assert sum(nm < 0 for nm, _ in want) > 50 and sum(nm > 0 for nm, _ in want) > 1000 and sum(b"^" in md for _, md in want) > 200
    for r, w in zip(recs, want):
        tid = ru.parse(r)["tid"]
        if 0 <= tid < len(contigs):
            assert refio.record_nm_md(r, contigs[tid]) == w


def test_damaged_records_are_eio():
    good = dict(ru.REC_CASES)["every_op"]
    for bad in ru.truncated(good):
        with pytest.raises(_ffi.SlxError) as e:
            refio.record_nm_md(bad, ru.REC_CONTIGS[0])
        assert e.value.code == _ffi.SLX_EIO


def test_without_a_gpu_opening_is_enodevice():
    import torch
    if torch.cuda.is_available():
        pytest.skip("a GPU is present: tests/test_gpu_ref.py opens references")
    with pytest.raises(_ffi.SlxError) as e:
        refio.Ref(os.path.join(GOLDEN, "tiny.fa"))
    assert e.value.code == _ffi.SLX_ENODEVICE
    with pytest.raises(_ffi.SlxError) as e:
        refio.Ref(os.path.join(GOLDEN, "no_such.fa"))
    assert e.value.code == _ffi.SLX_EIO


def test_bodies_under_sanitizers(exe, tmp_path, bulk):
    """dev_ref.h and ref_host.h over the FASTA cases, the record cases and 300 generated records, every text and record in a heap block of exactly its size: Python's
    index text, messages, NM and MD, with no sanitizer report"""
    lines = []
    for name in sorted(ru.GOOD):
        lines.append("F %s %s 1 %s" % (name, ru.GOOD[name].hex(), ru.fai_text(ru.GOOD[name]).hex()))
    for name in sorted(ru.BAD):
        lines.append("F %s %s 0 %s" % (name, ru.BAD[name][0].hex() or "-", ru.bad_message(name).encode().hex()))
    n_fa = len(lines)
    for i, c in enumerate(ru.REC_CONTIGS):
        lines.append("G %d %s" % (i, c.hex()))
    n_rec = 0
    for name, r in ru.REC_CASES:
        tid = ru.parse(r)["tid"]
        nm, md = ru.nm_md(r, ru.REC_CONTIGS)
        if tid < 3:          # (one record against one contig: no range to be outside of)
            lines.append("R %s %s %d 0 %d %s" % (name, r.hex(), max(tid, 0), nm, md.hex() or "-"))
            n_rec += 1
    for k, bad in enumerate(ru.truncated(dict(ru.REC_CASES)["every_op"])):
        lines.append("R damaged_%d %s 0 1 0 -" % (k, bad.hex()))
        n_rec += 1
    contigs, recs, want = bulk
    for i, c in enumerate(contigs):
        lines.append("G %d %s" % (10 + i, c.hex()))
    for i, (r, (nm, md)) in enumerate(zip(recs[:300], want)):
        tid = ru.parse(r)["tid"]
        if 0 <= tid < 3:
            lines.append("R bulk_%d %s %d 0 %d %s" % (i, r.hex(), 10 + tid, nm, md.hex() or "-"))
            n_rec += 1
    p = tmp_path / "expect.txt"
    p.write_text("\n".join(lines) + "\n")
    r = subprocess.run([exe, "cases", str(p)], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    assert "ref_host_test OK: %d texts, %d records" % (n_fa, n_rec) in r.stdout
