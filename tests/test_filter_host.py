"""CPU tests of the read filter (include/seqlib_amd_filter.h, seqlib_amd/csrc/slx_filter.hip, dev_rfilter.h, rfilter_host.h): the exports, the refusal
without a GPU, the host-compiled per-record body against the Python statement of the rules (tests/filter_util.py) on every record and every rule set, the
refusal of damaged records, and the bodies under ASan + UBSan in a program of their own (tests/cpp/filter_host_test.cpp).  No test here needs a GPU."""
import os
import re
import subprocess

import pytest

from tests import filter_util as fu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def ffi():
    import __graft_entry__ as g
    if not os.path.exists(os.path.join(ROOT, "seqlib_amd", "libseqlib_amd.so")):
        g.build()
    from seqlib_amd import _ffi
    _ffi.lib()
    return _ffi


@pytest.fixture(scope="module")
def data():
    recs = fu.records()
    parsed = fu.parsed(recs)
    return recs, parsed, fu.coverage(parsed)          # the model asserts that every rule set keeps and drops and that every clause decides somewhere


def test_filter_exports_match_header(ffi):
    from seqlib_amd import filterio
    hdr = open(os.path.join(ROOT, "include", "seqlib_amd_filter.h")).read()
    body = hdr[hdr.index("extern \"C\""):]
    declared = set(re.findall(r"\b(slx_[a-z0-9_]+)\s*\(", body))
    assert declared == set(filterio.FILTER_EXPORTS), declared ^ set(filterio.FILTER_EXPORTS)
    assert all(name.startswith("slx_filter_") for name in declared)
    L = filterio.lib()
    for name in declared:
        assert hasattr(L, name), name
    head = hdr[:hdr.index("#ifndef")]
    for name in filterio.FILTER_EXPORTS:
        assert name in head, name
    for words in ("Not carried", "No CPU fallback", "src/ReadFilter.cpp:22-136, 457-658", "0x100"):
        assert words in head, words


def test_filter_names_stay_out_of_the_other_headers_and_bindings(ffi):
    from seqlib_amd import bamio, fml, recio, sortio
    for other in ("seqlib_amd.h", "seqlib_amd_bam.h", "seqlib_amd_rec.h", "seqlib_amd_fml.h", "seqlib_amd_sort.h"):
        assert "slx_filter_" not in open(os.path.join(ROOT, "include", other)).read(), other
    assert not any(e.startswith("slx_filter_") for e in ffi.EXPORTS + bamio.EXPORTS + bamio.BAI_EXPORTS + bamio.BGZF_EXPORTS + recio.REC_EXPORTS + sortio.SORT_EXPORTS + list(fml.EXPORTS))


def test_filter_no_gpu_fails_loudly(ffi, tmp_path):
    import torch
    if torch.cuda.is_available():
        pytest.skip("GPU present")
    from seqlib_amd import bamio, filterio
    from tests import bam_util as bu
    flt = filterio.Filter(fu.RULE_SETS["everything"])          # building one needs no GPU
    assert flt.counter("seen") == 0
    with pytest.raises(ffi.SlxError) as e:
        flt.apply_device(0x1000, 0x2000, 3, 0x3000)
    assert e.value.code == ffi.SLX_ENODEVICE and "no CPU fallback" in str(e.value)
    src = tmp_path / "in.bam"
    src.write_bytes(bu.bam_bytes(bu.TEXT, bu.REFS, bu.sample_records(20)))
    with pytest.raises(ffi.SlxError) as e:                      # attach-then-next: there is no reader to attach to without a GPU
        rd = bamio.Reader(src)
        flt.attach(rd)
        rd.next()
    assert e.value.code == ffi.SLX_ENODEVICE and "no CPU fallback" in str(e.value)
    flt.close()


def test_record_test_equals_the_model(ffi, data):
    from seqlib_amd import filterio
    recs, parsed, masks = data
    assert len(recs) > 780
    for name, filters in fu.RULE_SETS.items():
        flt = filterio.Filter(filters)
        got = [flt.test_record(x) for x in recs]
        bad = [i for i, (a, b) in enumerate(zip(got, masks[name])) if a != b]
        assert not bad, (name, bad[:10], [parsed[i]["name"] for i in bad[:10]])
        assert flt.counter("seen") == len(recs) and flt.counter("passed") == sum(masks[name])
        flt.close()
    empty = filterio.Filter([])
    assert all(empty.test_record(x) for x in recs[:50])


def test_features_equal_the_model(ffi, data):
    from seqlib_amd import filterio
    recs, parsed, _ = data
    for raw, p in zip(recs, parsed):
        got, want = filterio.features(raw), fu.features(p)
        assert {k: got[k] for k in want} == want, p["name"]


@pytest.mark.parametrize("case", list(fu.damaged()))
def test_damaged_records_are_refused(ffi, case):
    from seqlib_amd import filterio
    rec = fu.damaged()[case]
    flt = filterio.Filter(fu.RULE_SETS["nm"])
    with pytest.raises(ffi.SlxError) as e:
        flt.test_record(rec)
    assert e.value.code == ffi.SLX_EIO and "pass its block_size" in str(e.value)
    with pytest.raises(ffi.SlxError) as e:
        flt.test_record(rec[:-1])                                # a span that is not block_size + 4
    assert e.value.code == ffi.SLX_EIO
    flt.close()


def test_filter_host_bodies_under_asan_ubsan(tmp_path):
    """dev_rfilter.h and rfilter_host.h on the host, one lane, in a stand-alone program: the DFA builder against naive search, the window evaluator and the
    long-record evaluator (several windows, lanes and chunks) against the one-lane evaluation of every record from an allocation of exactly its size, and the
    damaged records; every buffer exactly sized"""
    exe = str(tmp_path / "filter_host_test")
    subprocess.check_call(["g++", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-fno-omit-frame-pointer", "-g", "-O1", "-Wall", "-Werror",
                           "-Wno-unknown-pragmas", "-I" + os.path.join(ROOT, "include"), "-o", exe, os.path.join(ROOT, "tests", "cpp", "filter_host_test.cpp")])
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1")
    r = subprocess.run([exe], capture_output=True, text=True, env=env, timeout=300)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    assert "runtime error" not in r.stderr and "AddressSanitizer" not in r.stderr and "LeakSanitizer" not in r.stderr, r.stderr[-3000:]
    words = r.stdout.split()
    assert words[:2] == ["filter_host", "OK"] and int(words[2]) >= 400 and int(words[3]) > 100 and int(words[4]) > 300, r.stdout
