"""The host side of the interval unit, without a GPU: the exports, the host-only object's sorted arrays, merge and slx_grc_query_host against the Python statement of
the rules (tests/grc_util.py) on every case, the error codes, and csrc/grc_host.h's bodies under sanitizers in a stand-alone program (tests/cpp/grc_host_test.cpp)."""
import os
import re
import subprocess

import pytest

import seqlib_amd  # noqa: F401  (the package must import)
from seqlib_amd import _ffi, grcio
from tests import cov_util as cu
from tests import grc_util as gu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MODES = [(True, False), (False, False), (True, True), (False, True)]          # (ignore_strand, contained)


def host_collection(subjects):
    """a host-only object wherever the test runs"""
    c = grcio.Collection(subjects, device=grcio.SLX_GRC_HOST)
    assert c.counter("device") == -1
    return c


def test_header_declares_exactly_the_exports():
    text = open(os.path.join(ROOT, "include", "seqlib_amd_grc.h")).read()
    body = text[text.index("#ifndef SEQLIB_AMD_GRC_H"):]
    declared = re.findall(r"^\s*(?:int|void|int64_t)\s+(slx_\w+)\s*\(", body, re.M)
    assert sorted(declared) == sorted(grcio.GRC_EXPORTS)
    assert all(n.startswith("slx_grc_") for n in declared)
    L = grcio.lib()
    for n in grcio.GRC_EXPORTS:
        assert hasattr(L, n), n
    assert "SeqLib/GenomicRegionCollection.cpp:267-306" in text and "SeqLib/IntervalTree.h:198, 224" in text


def test_the_case_list_covers_what_it_claims():
    assert len(set(gu.CASE_IDS)) == len(gu.CASE_IDS)
    _, s, q = gu.case("container_200")
    counts = gu.join(s, q, True)[1]
    assert counts[0] == 202 and 64 < counts[1] <= 128 and counts[2] > 128 and counts[3] == 1
    assert gu.join(s, q, False)[1][3] == 0          # a long candidate range without a hit: the container is on the other strand
    assert gu.merge(gu.case("merge_shape")[1]) == [(2, 10, 110, "*"), (2, 200, 310, "*"), (23, 10, 110, "*")]
    assert gu.merge(gu.case("touch_merge")[1]) == [(0, 1, 50, "*"), (0, 51, 61, "*"), (1, 4, 5, "*"), (1, 6, 7, "*")]
    assert gu.merge([(0, 4, 6, "-"), (0, 6, 8, "+")]) == [(0, 4, 8, "-")]
    _, s, q = gu.case("extremes")
    assert gu.join(s, q, True)[2][0] == 2 ** 32 and gu.join(s, q, True)[1][0] == 5
    assert gu.width([(1, 3), (2, 2), (5, 6), (6, 9)]) == 8
    assert [len(c[1]) for c in gu.CASES if c[0].startswith("subjects_")] == [0, 1, 63, 64, 65, 300]
    assert [len(c[2]) for c in gu.CASES if c[0].startswith("queries_")] == [0, 1, 63, 64, 65, 1000]
    assert gu.record_iv(dict(cu.CASES)["plain"]) == (2, 100, 150) and gu.record_iv(dict(cu.CASES)["n_cigar_0"])[2] == 301


@pytest.mark.parametrize("name,subjects,queries", gu.CASES, ids=gu.CASE_IDS)
def test_sorted_merged_and_single_queries_equal_python(name, subjects, queries):
    c = host_collection(subjects)
    srt, perm, run, ends = c.sorted()
    assert (srt, perm, run, ends) == gu.sorted_index(subjects)
    assert c.merged() == gu.merge(subjects)
    assert c.counter("merged") == len(gu.merge(subjects)) and c.counter("subjects") == len(subjects)
    for q in queries[:70]:
        for ignore_strand, contained in MODES:
            want = gu.hits(subjects, q, ignore_strand, contained)
            got, w = c.query_host(q, ignore_strand, contained)
            assert got == want, (q, ignore_strand, contained)
            if not contained:
                assert w == gu.width([(a, b) for _, a, b in want])
    c.close()


def test_merging_a_merged_collection_changes_nothing():
    for _, subjects, _q in gu.CASES:
        m = gu.merge(subjects)
        c = host_collection(m)
        assert c.merged() == m
        c.close()


def test_einval_for_an_interval_that_ends_before_it_starts():
    with pytest.raises(_ffi.SlxError) as e:
        grcio.Collection([(0, 1, 5), (0, 6, 5)])
    assert e.value.code == _ffi.SLX_EINVAL
    c = host_collection([(0, 1, 5)])
    with pytest.raises(_ffi.SlxError) as e:
        c.query_host((0, 3, 2))
    assert e.value.code == _ffi.SLX_EINVAL
    with pytest.raises(_ffi.SlxError) as e:
        c.set("wave_range", (1 << 20) + 1)
    assert e.value.code == _ffi.SLX_EINVAL
    with pytest.raises(_ffi.SlxError) as e:
        c.set("nonsense", 1)
    assert e.value.code == _ffi.SLX_EINVAL and c.counter("nonsense") == -1
    for k in grcio.KNOBS:
        c.set(k, 64)
    assert all(c.counter(n) >= 0 for n in grcio.COUNTERS if n != "device")
    c.close()


def test_query_host_reports_the_number_when_the_arrays_are_short():
    import ctypes as C
    import numpy as np
    c = host_collection([(0, 1, 5), (0, 2, 6), (0, 3, 7)])
    ids, n = np.zeros(2, dtype=np.int32), C.c_int64(0)
    rc = grcio.lib().slx_grc_query_host(c.h, grcio.ivs([(0, 4, 4)]), 1, 0, ids.ctypes.data, None, None, 2, C.byref(n), None)
    assert rc == _ffi.SLX_EINVAL and n.value == 3 and ids.tolist() == [0, 1]
    rc = grcio.lib().slx_grc_query_host(c.h, grcio.ivs([(0, 4, 4)]), 1, 0, None, None, None, 0, C.byref(n), None)          # the number alone
    assert rc == 0 and n.value == 3
    c.close()


def test_on_a_host_only_object_every_batch_entry_is_enodevice():
    c = host_collection(gu.case("points")[1])
    stream, off = cu.stream_of(gu.case_records())
    for call in (lambda: c.overlaps([(0, 1, 2)]), lambda: c.count([(0, 1, 2)]), lambda: c.overlaps_host(stream, off), lambda: c.overlaps_device(None, 0, None, 0),
                 lambda: c.subject_counts(), lambda: c.clear_counts()):
        with pytest.raises(_ffi.SlxError) as e:
            call()
        assert e.value.code == _ffi.SLX_ENODEVICE
    c.close()
    with pytest.raises(_ffi.SlxError) as e:
        grcio.Collection([(0, 1, 2)], device=-3)
    assert e.value.code == _ffi.SLX_EINVAL


def test_without_a_gpu_a_device_object_is_enodevice_and_auto_is_host_only():
    import torch
    if torch.cuda.is_available():
        pytest.skip("a GPU is present: tests/test_gpu_grc.py builds on it")
    with pytest.raises(_ffi.SlxError) as e:
        grcio.Collection([(0, 1, 2)], device=0)
    assert e.value.code == _ffi.SLX_ENODEVICE
    c = grcio.Collection([(0, 1, 2)])
    assert c.counter("device") == -1 and c.query_host((0, 2, 2))[0] == [(0, 2, 2)]
    c.close()


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    """tests/cpp/grc_host_test.cpp under ASan and UBSan: a program of its own, nothing is loaded into Python"""
    out = str(tmp_path_factory.mktemp("grc") / "grc_host_test")
    subprocess.check_call(["g++", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-fno-omit-frame-pointer", "-g", "-O1", "-Wall", "-Werror",
                           "-I" + os.path.join(ROOT, "seqlib_amd", "csrc"), "-I" + os.path.join(ROOT, "include"), os.path.join(ROOT, "tests", "cpp", "grc_host_test.cpp"), "-o", out])
    return out


def iv_text(iv):
    return "%d %d %d %s" % gu.norm(iv)


def test_bodies_under_sanitizers(exe, tmp_path):
    """grc_host.h over the case list, every array in a heap block of exactly its size: the host build's arrays, the merge, and for every query and mode the
    candidate range, the count, the hits in order and the width -- Python's, with no sanitizer report"""
    lines, n_q = [], 0
    for _, subjects, queries in gu.CASES:
        lines.append("S %d %s" % (len(subjects), " ".join(iv_text(s) for s in subjects)))
        srt, perm, run, ends = gu.sorted_index(subjects)
        lines.append("X " + " ".join("%s %d %d %d" % (iv_text(s), p, r, e) for s, p, r, e in zip(srt, perm, run, ends)))
        m = gu.merge(subjects)
        lines.append("M %d %s" % (len(m), " ".join(iv_text(s) for s in m)))
        for q in queries[:70]:
            for ignore_strand, contained in MODES:
                h = gu.hits(subjects, q, ignore_strand, contained)
                lines.append("Q %s %d %d %d %s" % (iv_text(q), (1 if ignore_strand else 0) | (2 if contained else 0), gu.width([(a, b) for _, a, b in h]), len(h),
                                                   " ".join("%d %d %d" % x for x in h)))
                n_q += 1
    p = tmp_path / "expect.txt"
    p.write_text("\n".join(lines) + "\n")
    r = subprocess.run([exe, "cases", str(p)], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    assert "grc_host_test OK: %d sets, %d merges, %d queries" % (len(gu.CASES), len(gu.CASES), n_q) in r.stdout
