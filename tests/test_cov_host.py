"""The host side of the coverage unit, without a GPU: the exports, slx_cov_record_intervals against the Python statement of the rules (tests/cov_util.py), the array
layout and the decimal formatter of csrc/cov_host.h, and cov_host.h's per-record and per-position bodies under sanitizers in a stand-alone program
(tests/cpp/cov_host_test.cpp)."""
import os
import re
import subprocess

import pytest

import seqlib_amd  # noqa: F401  (the package must import)
from seqlib_amd import _ffi, covio
from tests import cov_util as cu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GRCH38 = [248956422, 242193529, 198295559, 190214555, 181538259, 170805979, 159345973, 145138636, 138394717, 133797422, 135086622, 133275309, 114364328, 107043718,
          101991189, 90338345, 83257441, 80373285, 58617616, 64444167, 46709983, 50818468, 156040895, 57227415]
CLIPS = [(0, 1 << 40), (0, 5000), (100, 300), (4990, 5000), (0, 1)]


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    """tests/cpp/cov_host_test.cpp under ASan and UBSan: a program of its own, nothing is loaded into Python"""
    out = str(tmp_path_factory.mktemp("cov") / "cov_host_test")
    subprocess.check_call(["g++", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-fno-omit-frame-pointer", "-g", "-O1", "-Wall", "-Werror", "-pthread",
                           "-I" + os.path.join(ROOT, "seqlib_amd", "csrc"), "-I" + os.path.join(ROOT, "include"), os.path.join(ROOT, "tests", "cpp", "cov_host_test.cpp"), "-o", out])
    return out


def test_header_declares_exactly_the_exports():
    text = open(os.path.join(ROOT, "include", "seqlib_amd_cov.h")).read()
    body = text[text.index("#ifndef SEQLIB_AMD_COV_H"):]
    declared = re.findall(r"^\s*(?:int|void|int64_t|const char \*)\s+\*?(slx_\w+)\s*\(", body, re.M)
    assert sorted(declared) == sorted(covio.COV_EXPORTS)
    assert all(n.startswith("slx_cov_") for n in declared)
    L = covio.lib()
    for n in covio.COV_EXPORTS:
        assert hasattr(L, n), n
    assert "src/non_api/STCoverage.cpp:44-109" in text and "116-176" in text


def test_the_case_list_covers_what_it_claims():
    names = [n for n, _ in cu.CASES]
    assert len(set(names)) == len(names)
    by = dict(cu.CASES)
    assert cu.intervals(by["plain"], cu.SPAN) == [(100, 151)] and cu.intervals(by["plain"], cu.ALIGNED) == [(100, 150)]          # the kept quirk: e is included
    assert cu.intervals(by["plain"], cu.SPAN, 3) == [(103, 148)] and cu.intervals(by["plain"], cu.SPAN, -2) == [(98, 153)]
    assert cu.intervals(by["5S10M"], cu.FULL) == [(395, 411)] and cu.intervals(by["10M5S"], cu.FULL) == [(420, 436)]
    assert cu.intervals(by["2H5S10M"], cu.FULL) == [(440, 451)] and cu.intervals(by["7S"], cu.FULL) == [(453, 469)]
    assert cu.intervals(by["5S10M_at_2"], cu.FULL) == [(0, 13)]
    assert cu.intervals(by["unmapped_placed"], cu.SPAN) == [(200, 202)] and cu.intervals(by["n_cigar_0"], cu.SPAN) == [(300, 302)]
    assert cu.intervals(by["n_cigar_0"], cu.SPAN, 3) == [] and cu.intervals(by["n_cigar_0"], cu.ALIGNED) == []
    assert cu.intervals(by["10M100N10M"], cu.ALIGNED) == [(500, 510), (610, 620)]
    assert cu.intervals(by["10M3D10M2I5M"], cu.ALIGNED) == [(700, 710), (713, 723), (723, 728)]
    assert cu.intervals(by["10M3D10M2I5M"], cu.ALIGNED, 0, 1) == [(700, 710), (710, 713), (713, 723), (723, 728)]
    for k in range(16):
        r = by["op_code_%d" % k]
        assert cu.intervals(r, cu.ALIGNED) == ([(900 + 4 * k, 907 + 4 * k)] if k in (0, 7, 8) else [])
        assert cu.intervals(r, cu.SPAN) == [(900 + 4 * k, 900 + 4 * k + (8 if k in cu.REF_OPS else 2))]
    assert [len(cu.parse(by["ops_%d" % n])[4]) for n in (64, 65, 200)] == [64, 65, 200]
    assert not any(cu.eligible(by[n], 4) for n in ("tid_-1", "tid_n_ref", "pos_-1", "unmapped_placed", "dup", "secondary", "qcfail")) and cu.eligible(by["supplementary"], 4)
    assert cu.eligible(by["low_mapq"], 4) and not cu.eligible(by["low_mapq"], 4, min_mapq=4) and cu.eligible(by["dup"], 4, exclude_flags=0)
    d = cu.depth([r for _, r in cu.CASES], cu.SPAN)
    assert d[2][4999] == 5 and d[0][0] == 2 and d[3][-1] == 1          # the extra position past a contig's end is dropped


@pytest.mark.parametrize("name,r", cu.CASES, ids=[n for n, _ in cu.CASES])
def test_record_intervals_equal_python(name, r):
    for mode, buff, count_del in cu.CONFIGS:
        for clip in CLIPS:
            assert covio.record_intervals(r, mode, buff, count_del, clip) == cu.clipped(cu.intervals(r, mode, buff, count_del), *clip), (mode, buff, count_del, clip)


def test_record_intervals_refuse_a_broken_record():
    r = bytearray(dict(cu.CASES)["10M3D10M2I5M"])
    for bad in (bytes(r[:-1]), bytes(r[:20]), bytes(r[:16] + b"\xff\xff" + r[18:])):          # cut, cut inside the fixed part, n_cigar past block_size
        with pytest.raises(_ffi.SlxError) as e:
            covio.record_intervals(bad, cu.ALIGNED)
        assert e.value.code == _ffi.SLX_EIO


def py_layout(lens):
    """len + 1 entries per contig, each contig on a 16-byte boundary"""
    off, at = [], 0
    for ln in lens:
        off.append(at)
        at += (ln + 1 + 3) // 4 * 4
    return off, at


@pytest.mark.parametrize("lens", [GRCH38, [2 ** 31 - 1, 5], [0, 1, 2, 3, 4, 70, 5000, 10000001]], ids=["grch38", "2^31-1", "small"])
def test_layout_is_64_bit(exe, lens):
    got = [int(x) for x in subprocess.run([exe, "layout"] + [str(x) for x in lens], capture_output=True, text=True, check=True).stdout.split()]
    off, total = py_layout(lens)
    assert got == off + [total]
    if lens is GRCH38:
        assert 4 * total > 2 ** 32 and abs(4 * total - 12.4e9) < 0.1e9 and got[23] == sum((x + 4) // 4 * 4 for x in GRCH38[:23]) > 2 ** 31
    if lens[0] == 2 ** 31 - 1:
        assert got[1] == 2 ** 31 and total == 2 ** 31 + 8


def test_decimal_formatter_is_exact(exe):
    vals = [0, 9, 10, 99999, 2147483647, 100000, 10000001, 4294967296, -1, -2147483648]
    r = subprocess.run([exe, "dec"] + [str(v) for v in vals], capture_output=True, text=True, check=True)
    assert r.stdout.split() == [str(v) for v in vals]


def test_without_a_gpu_adding_is_enodevice():
    import torch
    if torch.cuda.is_available():
        pytest.skip("a GPU is present: tests/test_gpu_cov.py adds records")
    c = covio.Coverage(cu.REFS)          # host only
    stream, off = cu.stream_of([r for _, r in cu.CASES])
    for call in (lambda: c.add_host(stream, off), lambda: c.add_device(None, 0, None, 0), lambda: c.depth(1), lambda: c.max(), lambda: c.at(1, 3), lambda: c.clear(),
                 lambda: c.regions([(1, 0, 5)]), lambda: c.bedgraph("/dev/null"), lambda: c.depth_device(1)):
        with pytest.raises(_ffi.SlxError) as e:
            call()
        assert e.value.code == _ffi.SLX_ENODEVICE
    c.set("mode", cu.SPAN)
    with pytest.raises(_ffi.SlxError) as e:
        c.set("mode", 3)
    assert e.value.code == _ffi.SLX_EINVAL and c.counter("records_seen") == 0 and c.counter("nonsense") == -1
    c.close()
    with pytest.raises(_ffi.SlxError) as e:
        covio.Coverage(cu.REFS, device=0)
    assert e.value.code == _ffi.SLX_ENODEVICE


def test_bodies_under_sanitizers(exe, tmp_path):
    """cov_host.h over the case list, every record in a heap block of exactly its size: cov_head's verdict, cov_record's intervals for every setting and clip, and the
    bedGraph text of all cases together through the layout, a prefix sum and cov_bg_piece -- Python's, with no sanitizer report"""
    recs = [r for _, r in cu.CASES]
    lines = ["R %d %s" % (len(cu.REFS), " ".join("%s %d" % x for x in cu.REFS))]
    n = 0
    for name, r in cu.CASES:
        for mode, buff, count_del in cu.CONFIGS:
            for clip in CLIPS:
                iv = cu.clipped(cu.intervals(r, mode, buff, count_del), *clip)
                lines.append("C %s %s %d %d %d %d %d %d %d %s" % (name, r.hex(), cu.eligible(r, len(cu.REFS)), mode, buff, count_del, clip[0], clip[1], len(iv), " ".join("%d %d" % x for x in iv)))
                n += 1
    n_texts = 0
    for mode, buff, count_del in cu.CONFIGS:
        d = cu.depth(recs, mode, buff, count_del)
        for iz in (0, 1):
            lines.append("B %d %d %d %d %s" % (mode, buff, count_del, iz, cu.bedgraph(d, iz).hex() or "-"))
            n_texts += 1
    p = tmp_path / "expect.txt"
    p.write_text("\n".join(lines) + "\n")
    r = subprocess.run([exe, "cases", str(p)], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    assert "cov_host_test OK: %d cases, %d texts" % (n, n_texts) in r.stdout
