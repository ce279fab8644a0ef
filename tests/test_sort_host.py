"""CPU tests of the coordinate sort (include/seqlib_amd_sort.h, seqlib_amd/csrc/slx_sort.hip, dev_recsort.h): the exports, the refusal without a GPU, the
header rule, and the host-compiled key and tile-gather bodies under ASan + UBSan against a plain memcpy model (tests/cpp/sort_host_test.cpp, a program of its
own).  No test here needs a GPU."""
import os
import re
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def ffi():
    import __graft_entry__ as g
    if not os.path.exists(os.path.join(ROOT, "seqlib_amd", "libseqlib_amd.so")):
        g.build()
    from seqlib_amd import _ffi
    _ffi.lib()
    return _ffi


def test_sort_exports_match_header(ffi):
    from seqlib_amd import sortio
    hdr = open(os.path.join(ROOT, "include", "seqlib_amd_sort.h")).read()
    body = hdr[hdr.index("extern \"C\""):]
    declared = set(re.findall(r"\b(slx_[a-z0-9_]+)\s*\(", body))
    assert declared == set(sortio.SORT_EXPORTS), declared ^ set(sortio.SORT_EXPORTS)
    assert all(name.startswith("slx_sort_") for name in declared)
    L = sortio.lib()
    for name in declared:
        assert hasattr(L, name), name
    head = hdr[:hdr.index("#ifndef")]
    for name in sortio.SORT_EXPORTS:
        assert name in head, name
    for words in ("Not carried", "No CPU fallback", "SeqLib/BamRecord.h:681-699", "HALF of the HBM"):
        assert words in head, words


def test_sort_names_stay_out_of_the_other_headers_and_bindings(ffi):
    from seqlib_amd import bamio, fml, recio
    for other in ("seqlib_amd.h", "seqlib_amd_bam.h", "seqlib_amd_rec.h", "seqlib_amd_fml.h"):
        assert "slx_sort_" not in open(os.path.join(ROOT, "include", other)).read(), other
    assert not any(e.startswith("slx_sort_") for e in ffi.EXPORTS + bamio.EXPORTS + bamio.BAI_EXPORTS + bamio.BGZF_EXPORTS + recio.REC_EXPORTS + list(fml.EXPORTS))


def test_sort_no_gpu_fails_loudly(ffi, tmp_path):
    import torch
    if torch.cuda.is_available():
        pytest.skip("GPU present")
    from seqlib_amd import sortio
    from tests import bam_util as bu
    with pytest.raises(ffi.SlxError) as e:
        sortio.Sorter()
    assert e.value.code == ffi.SLX_ENODEVICE and "no CPU fallback" in str(e.value)
    src, out = tmp_path / "in.bam", tmp_path / "out.bam"
    src.write_bytes(bu.bam_bytes(bu.TEXT, bu.REFS, bu.sample_records(20)))
    with pytest.raises(ffi.SlxError) as e:
        sortio.sort_file(src, out)
    assert e.value.code == ffi.SLX_ENODEVICE and "no CPU fallback" in str(e.value)
    assert not out.exists()


SQ = "@SQ\tSN:chrA\tLN:200000\n@PG\tID:x\tSO:unsorted\n"


@pytest.mark.parametrize("text, want", [
    ("@HD\tVN:1.6\tSO:unsorted\n" + SQ, "@HD\tVN:1.6\tSO:coordinate\n" + SQ),                          # the value is replaced
    ("@HD\tVN:1.6\tGO:query\n" + SQ, "@HD\tVN:1.6\tGO:query\tSO:coordinate\n" + SQ),                   # appended, GO: kept
    ("@HD\tSO:queryname\tVN:1.6\tGO:query\n" + SQ, "@HD\tSO:coordinate\tVN:1.6\tGO:query\n" + SQ),     # the field order is kept
    (SQ, "@HD\tVN:1.6\tSO:coordinate\n" + SQ),                                                          # no @HD: the line goes in front
    ("", "@HD\tVN:1.6\tSO:coordinate\n"),
    ("@HD\tVN:1.6\tSO:coordinate\n" + SQ, "@HD\tVN:1.6\tSO:coordinate\n" + SQ),                        # unchanged
    ("@HD\tVN:1.4", "@HD\tVN:1.4\tSO:coordinate"),                                                      # no newline at the end
])
def test_sort_header_rule(ffi, text, want):
    from seqlib_amd import sortio
    assert sortio.header_so(text) == want
    assert sortio.header_so(want) == want


def test_sort_header_is_one_copy():
    """the C-ABI and the C++ class share the rule: BamWriter.h calls slx_sort_header, and the text "SO:coordinate" is written down once in the sources"""
    hits = []
    for base, exts in (("include", (".h",)), (os.path.join("seqlib_amd", "csrc"), (".h", ".hip", ".cpp"))):
        for dp, _, fns in os.walk(os.path.join(ROOT, base)):
            for fn in fns:
                if fn.endswith(exts):
                    code = [ln.split("//")[0] for ln in open(os.path.join(dp, fn), errors="replace") if not ln.lstrip().startswith(("*", "/*", "//"))]
                    if any('SO:coordinate' in ln for ln in code):
                        hits.append(fn)
    assert hits == ["recsort_host.h"], hits
    assert "slx_sort_header(" in open(os.path.join(ROOT, "include", "SeqLib", "BamWriter.h")).read()


def test_sort_host_bodies_under_asan_ubsan(tmp_path):
    """dev_recsort.h on the host, one lane, in a stand-alone program: rs_key and every tile of rs_gather_tile against a memcpy model, with slabs of one tile, of
    three and of the whole stream, zero records and one record, every allocation exactly sized; the program asserts the edges its record list is built for"""
    exe = str(tmp_path / "sort_host_test")
    subprocess.check_call(["g++", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-fno-omit-frame-pointer", "-g", "-O1", "-Wall", "-Werror",
                           "-Wno-unknown-pragmas", "-o", exe, os.path.join(ROOT, "tests", "cpp", "sort_host_test.cpp")])
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1")
    r = subprocess.run([exe], capture_output=True, text=True, env=env, timeout=300)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    assert "runtime error" not in r.stderr and "AddressSanitizer" not in r.stderr and "LeakSanitizer" not in r.stderr, r.stderr[-3000:]
    words = r.stdout.split()
    assert words[:2] == ["sort_host", "OK"] and int(words[2]) > 60 and int(words[3]) % 16 != 0 and int(words[4]) >= 9, r.stdout
