"""The host side of the duplicate marker, without a GPU: the exports, SLX_ENODEVICE, slx_dup_signature_host (the kernels' per-record body on the CPU) against
the Python statement of the rules (tests/dup_util.py) over the edge list, slx_dup_library_of against the Python parse, and the rules' own worked examples."""
import os
import re
import struct
import subprocess

import pytest

import seqlib_amd  # noqa: F401  (the package must import)
from seqlib_amd import _ffi, dupio
from tests import dup_util as du

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_header_declares_exactly_the_exports():
    text = open(os.path.join(ROOT, "include", "seqlib_amd_dup.h")).read()
    body = text[text.index("#ifndef SEQLIB_AMD_DUP_H"):]
    declared = re.findall(r"^\s*(?:int|void|int64_t|const char)\s+\*?(slx_\w+)\s*\(", body, re.M)
    assert sorted(declared) == sorted(dupio.DUP_EXPORTS)
    assert all(n.startswith("slx_dup_") for n in declared)
    L = dupio.lib()
    for n in dupio.DUP_EXPORTS:
        assert hasattr(L, n), n
    rules = text[:text.index("#ifndef SEQLIB_AMD_DUP_H")]
    for word in ("0x4 | 0x100 | 0x800", "refID < 0", "ELIGIBLE", "is cleared", "first appearance", "a library of its own", "Library 0", "byte for byte", "pos - lead",
                 "pos + ref_len - 1 + trail", "EMPTY CIGAR", "pos - 1", "15 <= q <= 0xfe", "2^31 - 1", "0x8 clear", "PAIR", "ORPHANS", "E(a) <= E(b)", "lower ordinal is lowest",
                 "An orphan never is", "LOWEST", "as it was", "SLX_EIO", "SLX_EUNSUPPORTED", "max_bytes", "65 535", "run_max", "SLX_EINVAL", "wave_len", "long_records", "hash_bits",
                 "hash_runs_mixed", "No CPU fallback", "Not carried", "optical duplicates", "UMIs", "CG:B", "ReadFilter"):
        assert word in rules, word
    assert open(os.path.join(ROOT, "include", "seqlib_amd_sort.h")).read().count("slx_dup") == 0          # the sorter's header is as it was


def test_no_device_answers_enodevice():
    if dupio.lib().slx_device_count() > 0:
        return          # (a GPU is visible: tests/test_gpu_dup.py runs the marker)
    with pytest.raises(_ffi.SlxError) as e:
        dupio.Marker()
    assert e.value.code == _ffi.SLX_ENODEVICE and "duplicates are marked on MI355X only" in str(e.value)


def test_signatures_of_the_edge_list():
    edge = du.edge_records()
    recs = [r for _, r in edge]
    for header in (None, du.HEADER):
        got = dupio.signature_host(*du.stream_of(recs), header_text=header)
        for (label, r), g in zip(edge, got):
            assert g == du.signature(r, header), (label, header is not None)
    one_by_one = [dupio.signature_host(*du.stream_of([r]), header_text=du.HEADER)[0] for r in recs]          # other alignments of the same records
    assert one_by_one == [du.signature(r, du.HEADER) for r in recs]
    assert dupio.signature_host(b"", [0]) == []


def test_the_edge_list_covers_what_it_claims():
    sig = {label: du.signature(r, du.HEADER) for label, r in du.edge_records()}
    assert {s[0] for s in sig.values()} == {du.IGNORED, du.FRAGMENT, du.PAIRED}
    assert sig["noclip_f"][3] == 1000 and sig["hs_lead_f"][3] == 1000 - 12 and sig["s_trail_f"][3] == 1000
    assert sig["noclip_r"][3] == 1049 and sig["sh_trail_r"][3] == 1000 + 45 - 1 + 14 and sig["hs_lead_r"][3] == 1044
    assert sig["empty_cigar_r"][3] == 999 and sig["empty_cigar_f"][3] == 1000
    assert sig["clips_only_f"][3] == 1000 - 23 and sig["clips_only_r"][3] == 1000 - 1 + 23
    assert sig["inner_clip_f"][3] == 998 and sig["inner_clip_r"][3] == 1000 + 20 - 1 + 4
    assert sig["op_D_r"][3] == 1000 + 43 - 1 and sig["op_I_r"][3] == 1000 + 40 - 1 and sig["op_P_r"][3] == 1039 and sig["op_N_r"][3] == sig["op_=_r"][3] == sig["op_X_r"][3] == 1042
    assert sig["ops129_lead_run_66_f"][3] == 5000 - 66 and sig["ops129_lead_run_66_r"][3] == 5000 + 120 - 1 + 6
    assert (sig["q14"][5], sig["q15"][5], sig["q254"][5], sig["q255"][5], sig["no_qual"][5]) == (0, 135, 9 * 254, 0, 0)
    assert [sig[k][0] for k in ("flag4", "flag100", "flag800", "no_ref")] == [du.IGNORED] * 4
    assert [sig[k][0] for k in ("flag1", "flag9", "flag41", "flag91", "flag400")] == [du.PAIRED, du.FRAGMENT, du.PAIRED, du.PAIRED, du.FRAGMENT]
    libs = [sig[k][1] for k in ("rg_a1", "rg_a2", "rg_b", "rg_solo", "rg_a", "rg_unknown", "rg_empty", "rg_type_A", "rg_type_A_then_Z", "rg_behind_others", "rg_twice", "rg_noid",
                                "rg_comment", "aux_broken_before_rg", "aux_cut_short", "noclip_f")]
    assert libs == [1, 1, 2, 3, 4, 0, 0, 0, 0, 2, 2, 0, 0, 0, 0, 0]
    big = du.record("big", 0, 1, qual=bytes([0xfe]) * 5)
    assert du.signature(big)[5] == 5 * 254


@pytest.mark.parametrize("name", sorted(du.HEADERS))
def test_library_of_equals_the_python_parse(name):
    text = du.HEADERS[name]
    for rg in du.RG_PROBES:
        assert dupio.library_of(text, rg) == du.library_of(text, rg), rg
    want = {"no_rg": {}, "shared_lb": {b"x": 1, b"y": 2, b"z": 1}, "without_lb": {b"x": 1, b"y": 2, b"z": 3}, "prefix_id": {b"grp": 1, b"grp1": 2, b"g": 3},
            "mixed": {b"a1": 1, b"a2": 1, b"b": 2, b"solo": 3, b"a": 4}, "nul_padded": {b"x": 1}, "empty": {}}[name]
    assert du.libraries(text) == want


def test_too_many_libraries_are_refused():
    text = "".join("@RG\tID:g%d\n" % i for i in range(65536))
    with pytest.raises(_ffi.SlxError) as e:
        dupio.library_of(text, b"g1")
    assert e.value.code == _ffi.SLX_EUNSUPPORTED
    assert dupio.library_of("".join("@RG\tID:g%d\n" % i for i in range(65535)), b"g65534") == 65535


def broken_batches():
    """[(label, records, stream, offsets, lowest bad index)]"""
    good = [r for _, r in du.edge_records()[:6]]
    past = bytearray(good[3])
    struct.pack_into("<i", past, 20, 10 ** 6)                      # l_seq past the block
    no_nul = bytearray(good[3])
    no_nul[36 + good[3][12] - 1] = ord("x")                         # no NUL in the name
    out = []
    for label, bad in (("l_seq_past_block", bytes(past)), ("name_without_nul", bytes(no_nul))):
        recs = good[:3] + [bad] + good[4:]
        out.append((label, recs) + du.stream_of(recs) + (3,))
    stream, off = du.stream_of(good)
    # record 3 cut to 40 bytes: by the editor's test the record named is the one that does not start where the block_size before it ends
    out.append(("truncated_in_the_middle", good, stream[:off[3] + 40] + stream[off[4]:], off[:4] + [o - (off[4] - off[3] - 40) for o in off[4:]], 4))
    return out


def test_a_broken_record_is_named_by_its_lowest_index():
    for label, recs, stream, off, bad in broken_batches():
        with pytest.raises(_ffi.SlxError) as e:
            dupio.signature_host(stream, off)
        assert e.value.code == _ffi.SLX_EIO and "record %d of the batch" % bad in str(e.value), label


def test_body_under_sanitizers(tmp_path):
    """dup_host.h in a program of its own under ASan + UBSan, every block exactly sized: the edge list in one batch and record by record, with and without a
    header, a batch of none, the broken batches, and the tail of a batch -- Python's signatures, the lowest broken index, and no sanitizer report"""
    exe = str(tmp_path / "dup_host_test")
    subprocess.check_call(["g++", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-fno-omit-frame-pointer", "-g", "-O1", "-Wall", "-Werror",
                           "-I" + os.path.join(ROOT, "seqlib_amd", "csrc"), "-I" + os.path.join(ROOT, "include"), os.path.join(ROOT, "tests", "cpp", "dup_host_test.cpp"), "-o", exe])
    hexs = lambda b: bytes(b).hex() or "-"
    lines, want = [], []
    recs = [r for _, r in du.edge_records()]

    def batch(rs, header, stream=None, off=None, bad=None):
        if stream is None:
            stream, off = du.stream_of(rs)
        lines.append("B %d %s %s" % (len(off) - 1, hexs(stream), ",".join(map(str, off))))
        want.extend(["E %d" % bad] if bad is not None else ["S"] + ["%d %d %d %d %d %d" % du.signature(r, header) for r in rs])

    for header in ("", du.HEADER, du.HEADERS["nul_padded"]):
        lines.append("H %s" % hexs(header.encode()))
        batch(recs, header)
        batch([], header)
        for r in recs[::7]:
            batch([r], header)
    stream, off = du.stream_of(recs)
    batch(recs[5:], du.HEADERS["nul_padded"], stream[off[5]:], off[5:])          # the tail of a batch: the table from entry 5 on as it stands
    for label, rs, stream, off, bad in broken_batches():
        batch(rs, None, stream, off, bad)
    p = tmp_path / "cases.txt"
    p.write_text("\n".join(lines) + "\n")
    r = subprocess.run([exe, str(p)], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-3000:]
    got = r.stdout.splitlines()
    assert got[:-1] == want and got[-1].startswith("dup_host_test OK: %d batches" % len([ln for ln in lines if ln[0] == "B"]))


def test_the_rules_worked_examples():
    """mark() on cases whose answer is written down here by hand"""
    D, N, U = du.DUP, du.NOT_DUP, du.UNTOUCHED
    q = lambda v: bytes([v]) * 50
    # two pairs at the same ends: the better one stays; a tie goes to the lower ordinal
    assert du.mark([du.pair("a", 0, 100, 300, q(20)) + du.pair("b", 0, 100, 300, q(30))])[0] == [D, D, N, N]
    assert du.mark([du.pair("a", 0, 100, 300) + du.pair("b", 0, 100, 300)])[0] == [N, N, D, D]
    # one base, the strand or the contig apart: no duplicates
    assert du.mark([du.pair("a", 0, 100, 300) + du.pair("b", 0, 100, 301) + du.pair("c", 0, 100, 300, flag1=0x10) + du.pair("d", 0, 100, 300, refid2=1)])[0] == [N] * 8
    # a fragment beside a paired record is a duplicate; fragments alone keep their best; an orphan never is one
    frag = du.record("f", 0, 100, qual=q(40))
    assert du.mark([[frag] + du.pair("a", 0, 100, 300)])[0] == [D, N, N]
    assert du.mark([[frag, du.pair("a", 0, 100, 300)[0]]])[0] == [D, N]
    assert du.mark([[du.record("f1", 0, 100, qual=q(20)), frag, du.record("f3", 0, 100, qual=q(40))]])[0] == [D, N, D]
    # three records of one name, and two first reads, are orphans
    three = du.pair("t", 0, 100, 300) + [du.pair("t", 0, 100, 300)[0]]
    assert du.mark([three + three])[0] == [N] * 6 and du.mark([three])[1]["orphans"] == 3
    two_first = [du.pair("u", 0, 100, 300)[0], du.pair("u", 0, 100, 300)[0]]
    assert du.mark([two_first + du.pair("v", 0, 100, 300) + du.pair("w", 0, 100, 300)])[0] == [N, N, N, N, D, D]
    # an ignored record is untouched; a set bit on an eligible record that is no duplicate goes
    sec = du.record("s", 0, 100, flag=0x100 | 0x400)
    old = du.record("o", 0, 100, flag=0x400)
    ver = du.mark([[sec, old]])[0]
    assert ver == [U, N] and du.marked(sec, ver[0]) == sec and struct.unpack_from("<H", du.marked(old, ver[1]), 18)[0] == 0
