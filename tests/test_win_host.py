"""The host side of the assembly-window collector, without a GPU: the exports, the host-only handle, the knobs, slx_win_quality_trim against the Python
statement of the rules (tests/win_util.py), and win_host.h's and dev_win.h's bodies under sanitizers in a stand-alone program (tests/cpp/win_host_test.cpp)."""
import os
import random
import re
import struct
import subprocess

import pytest

import seqlib_amd  # noqa: F401  (the package must import)
from seqlib_amd import _ffi, winio
from tests import ref_util as ru
from tests import win_util as wu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
THRESHOLDS = (0, 4, 41, 93)
LENGTHS = (0, 1, 2, 63, 64, 65)
WINDOWS = [(0, 0, 5000), (0, 100, 200), (1, 0, 10)]


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    """tests/cpp/win_host_test.cpp under ASan and UBSan: a program of its own, nothing is loaded into Python"""
    out = str(tmp_path_factory.mktemp("win") / "win_host_test")
    subprocess.check_call(["g++", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-fno-omit-frame-pointer", "-g", "-O1", "-Wall", "-Werror",
                           "-I" + os.path.join(ROOT, "seqlib_amd", "csrc"), "-I" + os.path.join(ROOT, "include"), os.path.join(ROOT, "tests", "cpp", "win_host_test.cpp"), "-o", out])
    return out


def test_header_declares_exactly_the_exports():
    text = open(os.path.join(ROOT, "include", "seqlib_amd_win.h")).read()
    body = text[text.index("#ifndef SEQLIB_AMD_WIN_H"):]
    declared = re.findall(r"^\s*(?:int|void|int64_t|const char)\s+\*?(slx_\w+)\s*\(", body, re.M)
    assert sorted(declared) == sorted(winio.WIN_EXPORTS)
    assert all(n.startswith("slx_win_") for n in declared)
    L = winio.lib()
    for n in winio.WIN_EXPORTS:
        assert hasattr(L, n), n
    rules = text[:text.index("#ifndef SEQLIB_AMD_WIN_H")]
    for word in ("slx_grc_overlaps_device", "skip_flags", "l_read_name <= 1", "=ACMGRSVTWYHKDBN", "original_strand", "wraps to 0x20", "QUIRK", "qual_trim", "QualityTrimmedSequence",
                 "before the strand flip", "ascending global record ordinal", "caller's order", "two records", "SLX_EIO", "LOWEST", "as it was before the call", "SLX_EUNSUPPORTED",
                 "arena_bytes", "2^32", "wave_len", "No CPU fallback", "Not carried"):
        assert word in rules, word
    fml = open(os.path.join(ROOT, "include", "seqlib_amd_fml.h")).read()
    assert re.search(r"^int\s+slx_fml_stage_device\(slx_fml \*f, const void \*d_bases, const void \*d_quals, const void \*d_offs, int64_t n_reads\);", fml, re.M)
    assert hasattr(L, "slx_fml_stage_device")


def test_host_only_handle_answers_enodevice():
    c = winio.Collector(WINDOWS, winio.HOST)
    assert c.counter("device") == -1 and c.counter("windows") == 3
    stream, off = ru.stream_of(wu.edge_records()[:3])
    for call, args in ((c.add_host, (stream, off)), (c.add_device, (None, 0, None, 0)), (c.finish, ()), (c.view, ()), (c.download, ()), (c.clear, ())):
        with pytest.raises(_ffi.SlxError) as e:
            call(*args)
        assert e.value.code == _ffi.SLX_ENODEVICE and "assembly windows are collected on MI355X only" in str(e.value), call
    c.close()
    for bad in ((winio.Collector, ([(0, 5, 4)], winio.HOST)), (winio.Collector, (WINDOWS, -3))):          # pos2 < pos1; no such device value
        with pytest.raises(_ffi.SlxError) as e:
            bad[0](*bad[1])
        assert e.value.code == _ffi.SLX_EINVAL


def test_knobs_and_counters():
    c = winio.Collector([], winio.HOST)
    assert (c.counter("skip_flags"), c.counter("qual_trim"), c.counter("original_strand"), c.counter("wave_len"), c.counter("arena_bytes")) == (0, -1, 0, 512, 2 ** 34)
    for key, good, bad in (("skip_flags", (0, 0xffff), (-1, 0x10000)), ("qual_trim", (-1, 0, 93), (-2, 94)), ("original_strand", (0, 1), (-1, 2)), ("wave_len", (0, 2 ** 20), (-1, 2 ** 20 + 1)),
                           ("arena_bytes", (0, 2 ** 40), (-1,))):
        for v in good:
            c.set(key, v)
            assert c.counter(key) == v
        for v in bad:
            with pytest.raises(_ffi.SlxError) as e:
                c.set(key, v)
            assert e.value.code == _ffi.SLX_EINVAL
    with pytest.raises(_ffi.SlxError):
        c.set("no_such_knob", 1)
    assert c.counter("no_such_counter") == -1
    for name in winio.COUNTERS:
        assert c.counter(name) >= -1 and (name == "device" or name == "qual_trim" or c.counter(name) >= 0), name
    c.close()


def _profiles():
    for t in THRESHOLDS:
        for n in LENGTHS:
            for name, q in sorted(wu.profile_quals(n, t).items()):
                yield t, n, name, q


def test_quality_trim_gives_the_reference_pairs():
    seen = set()
    for t, n, name, q in _profiles():
        want = wu.quality_trim(q, t)
        assert winio.quality_trim(q, t) == want, (t, n, name)
        seen.add((want[0] == 0, want[1] == -1, want[0] == n))
    assert winio.quality_trim(b"", 4) == (0, -1)
    assert winio.quality_trim(bytes([3, 3, 30, 3, 30, 3]), 4) == (2, 5) and winio.quality_trim(bytes([3] * 6), 4) == (6, -1) and winio.quality_trim(b"\xff\x03\x03", 4) == (0, -1)
    assert len(seen) >= 4


def _hexs(b):
    return bytes(b).hex() or "-"


def _batch_line(recs, rules, stream=None, off=None):
    if stream is None:
        stream, off = ru.stream_of(recs)
    bad = wu.first_bad(stream, off)
    offs = ",".join(map(str, off))
    if bad is not None:
        return "B %d %s %s 1 %d - - -" % (len(off) - 1, _hexs(stream), offs, bad)
    got = [wu.read_of(r, rules) for r in recs]
    return "B %d %s %s 0 -1 %s %s %s" % (len(recs), _hexs(stream), offs, ",".join(str(s) for s, _, _ in got) or "-", _hexs(b"".join(b for _, b, _ in got)), _hexs(b"".join(q for _, _, q in got)))


def _profile_records(t):
    recs = []
    for n in LENGTHS:
        for k, (name, q) in enumerate(sorted(wu.profile_quals(n, t).items())):
            seq = wu.rand_seq(random.Random(n * 10 + k), n, wu.SEQ_CODES)
            recs.append(wu.record("%s%d" % (name, n), 0, 100 + n, seq, q, flag=0x10 if k % 2 else 0))
    return recs


def broken_records():
    good = wu.record("good", 0, 100, "ACGTACGTAC", bytes(range(10)))
    past = bytearray(good)
    struct.pack_into("<i", past, 20, 10 ** 6)                      # l_seq past the block
    no_nul = bytearray(good)
    no_nul[36 + good[12] - 1] = ord("x")                            # no NUL in the name
    short = struct.pack("<I", 20) + bytes(20)                       # block_size below the fixed part
    return [("l_seq_past_block", bytes(past)), ("name_without_nul", bytes(no_nul)), ("block_size_below_fixed", short)]


def test_the_cases_cover_what_they_claim():
    sts = set()
    for t in THRESHOLDS:
        for r in _profile_records(t):
            sts.add(wu.read_of(r, wu.Rules(qual_trim=t))[0])
    assert sts == {wu.KEEP, wu.NO_SEQ, wu.TRIMMED}
    assert wu.read_of(wu.record("", 0, 1, "ACGT", bytes(4)), wu.Rules())[0] == wu.NO_NAME
    r = wu.record("r", 0, 1, "ACMGN", None, flag=0x10)
    assert wu.read_of(r, wu.Rules()) == (wu.KEEP, b"ACMGN", b"\x20" * 5)          # the 0xff filler wraps to a space
    assert wu.read_of(r, wu.Rules(original_strand=1))[1] == b"NCKGT"
    r = wu.record("r", 0, 1, "ACGTA", bytes([1, 30, 2, 30, 3]), flag=0x10)
    assert wu.read_of(r, wu.Rules(qual_trim=4, original_strand=1))[1:] == (b"ACG", bytes([63, 35, 63]))          # trimmed to CGT first, then flipped
    for name, bad in broken_records():
        with pytest.raises(wu.BadRecord):
            wu.fields(bad)
    lens = {struct.unpack_from("<i", r, 20)[0] for r in wu.edge_records()}
    assert lens == set(wu.EDGE_LENGTHS)


def test_bodies_under_sanitizers(exe, tmp_path):
    """the measure step, the extract and the tile gather over the trim profiles at every threshold and length, the edge lengths (reads that span tiles among
    them), every skip-flag bit, the empty name, batches of 0 and 1, and refused batches -- every block exactly sized: Python's statuses and bytes, with no
    sanitizer report"""
    lines, n_batches, n_records, n_trims = [], 0, 0, 0
    for t, n, name, q in _profiles():
        lines.append("T %d %s %d %d" % ((t, _hexs(q)) + wu.quality_trim(q, t)))
        n_trims += 1
    for n in (511, 512, 513, 2049):          # what the wave form scans in more than one ballot
        for at in (0, 63, 64, n - 1):
            q = bytearray([3] * n)
            q[at] = 40
            lines.append("T 4 %s %d %d" % ((_hexs(q),) + wu.quality_trim(q, 4)))
            n_trims += 1

    def batch(recs, rules, stream=None, off=None):
        nonlocal n_batches, n_records
        line = _batch_line(recs, rules, stream, off)
        lines.append(line)
        n_batches += 1
        if " 0 -1 " in line:
            n_records += len(recs)

    edge = wu.edge_records()
    empty_name = wu.record("", 0, 100, "ACGT", bytes(4))
    for strand in (0, 1):
        for t in (-1,) + THRESHOLDS:
            rules = wu.Rules(qual_trim=t, original_strand=strand)
            lines.append("R 0 %d %d" % (t, strand))
            batch(_profile_records(max(t, 0)) + [empty_name], rules)
            batch(edge, rules)
            batch([], rules)
            batch(edge[4:5], rules)
    flagged = [wu.record("f%x" % (1 << b), 0, 100, "ACGTAC", bytes(6), flag=1 << b) for b in range(12)] + [wu.record("f0", 0, 100, "ACGTAC", bytes(6))]
    for b in range(12):
        lines.append("R %d -1 0" % (1 << b))
        batch(flagged, wu.Rules(skip_flags=1 << b))
    lines.append("R 0 4 1")
    rules = wu.Rules(qual_trim=4, original_strand=1)
    good = edge[:6]
    for name, bad_rec in broken_records():          # a broken record in the middle
        recs = good[:3] + [bad_rec] + good[3:]
        stream, off = ru.stream_of(recs)
        assert wu.first_bad(stream, off) == 3, name
        batch(recs, rules, stream, off)
    stream, off = ru.stream_of(good)
    for k, delta in ((0, 4), (3, 4), (3, -4), (6, -1), (6, 1), (2, 10 ** 6)):          # a wrong entry of the offset table
        o2 = list(off)
        o2[k] += delta
        assert wu.first_bad(stream, o2) is not None
        batch(good, rules, stream, o2)
    for k in (1, 5):          # the tail of a batch: the table from entry k on as it stands, the stream from record k on
        batch(good[k:], rules, stream[off[k]:], off[k:])
    p = tmp_path / "expect.txt"
    p.write_text("\n".join(lines) + "\n")
    r = subprocess.run([exe, "cases", str(p)], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    assert "win_host_test OK: %d trims, %d batches, %d records" % (n_trims, n_batches, n_records) in r.stdout
