"""The host side of the read statistics, without a GPU: the exports, the bin layouts, slx_stats_record against the Python statement of the rules
(tests/stats_util.py), damaged records, dev_stats.h's and stats_host.h's bodies under sanitizers in a stand-alone program (tests/cpp/stats_host_test.cpp), and
SeqLib::Histogram through a program that links nothing (tests/cpp/histogram_test.cpp)."""
import os
import re
import subprocess

import pytest

import seqlib_amd  # noqa: F401  (the package must import)
from seqlib_amd import _ffi, statsio
from tests import filter_util as fu
from tests import stats_util as su

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    """tests/cpp/stats_host_test.cpp under ASan and UBSan: a program of its own, nothing is loaded into Python"""
    out = str(tmp_path_factory.mktemp("stats") / "stats_host_test")
    subprocess.check_call(["g++", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-fno-omit-frame-pointer", "-g", "-O1", "-Wall", "-Werror",
                           "-I" + os.path.join(ROOT, "seqlib_amd", "csrc"), "-I" + os.path.join(ROOT, "include"), os.path.join(ROOT, "tests", "cpp", "stats_host_test.cpp"), "-o", out])
    return out


@pytest.fixture(scope="module")
def hist_exe(tmp_path_factory):
    out = str(tmp_path_factory.mktemp("hist") / "histogram_test")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-Werror", "-I" + os.path.join(ROOT, "include"), os.path.join(ROOT, "tests", "cpp", "histogram_test.cpp"), "-o", out])
    return out


def test_header_declares_exactly_the_exports():
    text = open(os.path.join(ROOT, "include", "seqlib_amd_stats.h")).read()
    body = text[text.index("#ifndef SEQLIB_AMD_STATS_H"):]
    declared = re.findall(r"^\s*(?:int|void|int64_t|const char)\s+\*?(slx_\w+)\s*\(", body, re.M)
    assert sorted(declared) == sorted(statsio.STATS_EXPORTS)
    assert all(n.startswith("slx_stats_") for n in declared)
    L = statsio.lib()
    for n in statsio.STATS_EXPORTS:
        assert hasattr(L, n), n
    rules = text[:text.index("#ifndef SEQLIB_AMD_STATS_H")]
    for word in ("src/non_api/BamStats.cpp:45-109", "src/non_api/Histogram.cpp:14-48", "QNAMED_", "first appearance", "0x100", "nm_missing", "below", "above", "SLX_EUNSUPPORTED", "SLX_EIO"):
        assert word in rules, word


def test_the_case_list_covers_what_it_claims():
    names = [n for n, _ in su.CASES]
    assert len(set(names)) == len(names)
    by = {n: su.parse(r) for n, r in su.CASES}
    g = lambda n: su.group(by[n])
    v = lambda n, h: su.values(by[n])[0][h]
    assert g("rg_z") == b"g1" and g("rg_z_empty") == b"QNAMED_lane7" and g("rg_type_a") == b"QNAMED_lane8" and g("rg_second_of_two") == b"first" and g("rg_i_then_z") == b"QNAMED_NA"
    assert g("name_colon") == b"QNAMED_flow" and g("name_no_colon") == b"QNAMED_NA" and g("name_colon_first") == b"QNAMED_"
    assert [len(g(n)) for n in ("key_255", "key_256", "qnamed_255", "qnamed_256")] == [255, 256, 255, 256]
    assert [(v("nm_" + t, "nm"), su.values(by["nm_" + t])[1]) for t in "cCsSiI"] == [(7, True), (200, True), (30, True), (99, True), (5, True), (6, True)]
    assert [su.values(by[n])[1] for n in ("nm_z", "nm_z_then_int", "nm_absent", "nm_negative")] == [False, False, False, True] and v("nm_negative", "nm") == -3
    assert [v(n, "isize") for n in ("isize_not_paired", "isize_mate_unmapped", "isize_read_unmapped", "isize_other_contig", "isize_-150", "isize_-2147483648")] == [-2, -2, -2, -1, 150, 2 ** 31]
    assert [v("clip_%d" % n, "clip") for n in (0, 4, 5, 99, 100, 101)] == [0, 4, 5, 99, 100, 101] and v("clip_hs_both_ends", "clip") == 15
    assert v("qual_all_ff", "phred") == 255 and v("qual_all_0", "phred") == 0 and v("l_seq_0", "phred") == -1 and v("qual_mixed_floor", "phred") == 39
    assert [by["ops_%d" % n]["n_cigar"] for n in (64, 65, 200)] == [64, 65, 200]
    # the QUAL starts at each of the four byte alignments of its record
    starts = {(36 + by["qual_align_%d_len_7" % k]["l_name"] + 4 + 4) % 4 for k in range(4)}
    assert starts == {0, 1, 2, 3}
    acc = dict((k, (c, h)) for k, c, h in su.accumulate([su.parse(r) for r in su.GOOD]))
    c, h = acc[b"g1"]
    assert h["isize"][1] == 0 and h["isize"][2] == 4 and h["nm"][1] == 1 and h["nm"][2] == 2 and h["mapq"][2] == 2 and h["clip"][2] == 2 and h["len"][2] == 1          # below, above (clip: 101, and the 200 ops)
    assert h["phred"][1] == 1 and h["phred"][2] == 2 and c["nm_missing"] == 3 and h["isize"][0][-1] == 2 and h["isize"][0][-2] == 1


@pytest.mark.parametrize("which,n,last", [("mapq", 101, (100, 100)), ("nm", 101, (100, 100)), ("isize", 201, (1998, 2000)), ("clip", 21, (100, 100)), ("phred", 101, (100, 100)),
                                          ("len", 251, (250, 250))])
def test_bin_layouts(which, n, last):
    s = statsio.Stats()
    b = s.bins(which)
    assert b == su.bins(which) and len(b) == n and b[-1] == last
    assert all(b[k][1] + 1 == b[k + 1][0] for k in range(n - 1))
    s.close()


def test_len_max_and_isize_max_move_the_last_bin():
    s = statsio.Stats(len_max=300, isize_max=1005)
    assert s.bins("len") == su.bins("len", len_max=300) and len(s.bins("len")) == 301
    assert s.bins("isize") == su.bins("isize", isize_max=1005) and s.bins("isize")[-1] == (998, 1005)
    assert sum(len(s.bins(h)) for h in statsio.HISTS) == 776 + 50 - 100
    s.close()
    assert sum(len(su.bins(h)) for h in su.HISTS) == 776


@pytest.mark.parametrize("name,r", su.CASES, ids=[n for n, _ in su.CASES])
def test_record_equals_python(name, r):
    p = su.parse(r)
    if name in su.FAILING:
        with pytest.raises(_ffi.SlxError) as e:
            statsio.record(r)
        assert e.value.code == _ffi.SLX_EUNSUPPORTED and len(su.group(p)) > su.MAX_KEY
        return
    group, values, has_nm, flag = statsio.record(r)
    assert group == su.group(p) and (values, has_nm) == su.values(p) and flag == p["flag"]


def test_bulk_records_equal_python():
    recs = su.bulk()
    for r, p in zip(recs, fu.parsed(recs)):
        group, values, has_nm, flag = statsio.record(r)
        assert group == su.group(p) and (values, has_nm) == su.values(p) and flag == p["flag"]


def test_damaged_records_are_eio():
    for name, r in fu.damaged().items():
        with pytest.raises(_ffi.SlxError) as e:
            statsio.record(r)
        assert e.value.code == _ffi.SLX_EIO, name
    good = dict(su.CASES)["clip_hs_both_ends"]
    for bad in (good[:-1], good[:20], good[:16] + b"\xff\xff" + good[18:]):          # cut, cut inside the fixed part, n_cigar past block_size
        with pytest.raises(_ffi.SlxError) as e:
            statsio.record(bad)
        assert e.value.code == _ffi.SLX_EIO


def test_knob_ranges():
    s = statsio.Stats()
    for key, bad in (("len_max", 0), ("isize_max", (1 << 20) + 1), ("exclude_flags", 0x10000), ("min_mapq", 256), ("lds_groups", 17), ("window_bytes", 48), ("window_bytes", 100),
                     ("window_bytes", 32784), ("group_slots", 1), ("long_record", 0), ("max_groups", 0), ("max_groups", (1 << 20) + 1), ("no such knob", 1)):
        with pytest.raises(_ffi.SlxError) as e:
            s.set(key, bad)
        assert e.value.code == _ffi.SLX_EINVAL, key
    for key, ok in (("len_max", 1), ("isize_max", 1 << 20), ("exclude_flags", 0xffff), ("min_mapq", 255), ("lds_groups", 0), ("lds_groups", 16), ("window_bytes", 64), ("window_bytes", 32768),
                    ("group_slots", 2), ("group_slots", 1000), ("max_groups", 1), ("max_groups", 1 << 20), ("long_record", 1), ("long_record", 2 ** 31 - 1)):
        s.set(key, ok)
    assert s.counter("nonsense") == -1 and all(s.counter(c) == 0 for c in statsio.COUNTERS)
    s.close()


def test_without_a_gpu_adding_is_enodevice():
    import torch
    if torch.cuda.is_available():
        pytest.skip("a GPU is present: tests/test_gpu_stats.py adds records")
    s = statsio.Stats()          # host only
    stream, off = su.stream_of(su.GOOD)
    for call in (lambda: s.add_host(stream, off), lambda: s.add_device(None, 0, None, 0)):
        with pytest.raises(_ffi.SlxError) as e:
            call()
        assert e.value.code == _ffi.SLX_ENODEVICE
    assert s.n_groups() == 0 and s.text() == su.HEADER.encode() and s.group_name(0) is None
    s.clear()
    s.close()
    with pytest.raises(_ffi.SlxError) as e:
        statsio.Stats(device=0)
    assert e.value.code == _ffi.SLX_ENODEVICE


def test_bodies_under_sanitizers(exe, tmp_path):
    """dev_stats.h over the case list, every record in a heap block of exactly its size: st_record's values and key, the lane-of-nlanes split for 1, 2, 7 and 64
    lanes, every truncated copy, then the adds, the group registry and the text -- Python's, with no sanitizer report"""
    lines = []
    for i, h in enumerate(su.HISTS):
        b = su.bins(h)
        lines.append("B %d %d %s" % (i, len(b), " ".join("%d %d" % x for x in b)))
    good = []
    for name, r in su.CASES + [("dmg_" + n, r) for n, r in fu.damaged().items()] + [("bulk_%d" % i, r) for i, r in enumerate(su.bulk()[:60]) if len(r) < 3000]:
        p = su.parse(r)
        if name.startswith("dmg_"):
            lines.append("C %s %s 1 - 0 0 0 0 0 0 0 0" % (name, r.hex()))
            continue
        if name in su.FAILING:
            lines.append("C %s %s 2 - 0 0 0 0 0 0 0 0" % (name, r.hex()))
            continue
        v, has_nm = su.values(p)
        lines.append("C %s %s 0 %s %d %d %s" % (name, r.hex(), su.group(p).hex(), has_nm, p["flag"], " ".join(str(v[h]) for h in su.HISTS)))
        good.append(p)
    lines.append("T %s" % su.text(su.accumulate(good)).hex())
    p = tmp_path / "expect.txt"
    p.write_text("\n".join(lines) + "\n")
    r = subprocess.run([exe, "cases", str(p)], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    assert "stats_host_test OK: %d cases, 6 histograms, 1 texts" % (len(lines) - 7) in r.stdout


def test_histogram_class(hist_exe):
    r = subprocess.run([hist_exe, "self"], capture_output=True, text=True)
    assert r.returncode == 0 and r.stdout == "histogram self OK\n", r.stdout + r.stderr
    for (start, end, width), which in (((0, 100, 1), "mapq"), ((-2, 2000, 10), "isize"), ((0, 100, 5), "clip"), ((0, 250, 1), "len")):
        vals = [start - 1, start, start + width - 1, start + width, end - 1, end, end, end + 1, 300]
        out = subprocess.run([hist_exe, "bins", str(start), str(end), str(width)] + [str(v) for v in vals], capture_output=True, text=True, check=True).stdout.split("\n")
        b = su.bins(which)
        cnt = [sum(lo <= v <= hi for v in vals) for lo, hi in b]
        assert out[:len(b)] == ["%d %d %d" % (lo, hi, n) for (lo, hi), n in zip(b, cnt)]
        assert out[len(b)] == "%d %d" % (sum(v < start for v in vals), sum(v > end for v in vals))
        assert out[len(b) + 1] == ",".join("%d_%d_%d" % (lo, hi, n) for (lo, hi), n in zip(b, cnt) if n)
