"""The host side of the record editor, without a GPU: the exports, every SLX_EINVAL of the plan, slx_edit_record against the Python statement of the rules
(tests/edit_util.py) over the record cases and 2 000 generated records, damaged records and malformed aux areas, the host-only handle, and dev_edit.h's and
edit_host.h's bodies under sanitizers in a stand-alone program (tests/cpp/edit_host_test.cpp)."""
import os
import re
import struct
import subprocess

import pytest

import seqlib_amd  # noqa: F401  (the package must import)
from seqlib_amd import _ffi, editio
from tests import edit_util as eu
from tests import ref_util as ru

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    """tests/cpp/edit_host_test.cpp under ASan and UBSan: a program of its own, nothing is loaded into Python"""
    out = str(tmp_path_factory.mktemp("edit") / "edit_host_test")
    subprocess.check_call(["g++", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-fno-omit-frame-pointer", "-g", "-O1", "-Wall", "-Werror",
                           "-I" + os.path.join(ROOT, "seqlib_amd", "csrc"), "-I" + os.path.join(ROOT, "include"), os.path.join(ROOT, "tests", "cpp", "edit_host_test.cpp"), "-o", out])
    return out


@pytest.fixture(scope="module")
def bulk():
    return eu.bulk_records()


@pytest.fixture()
def ed():
    e = editio.Editor(editio.HOST)
    yield e
    e.close()


def _record(ed, plan, rec, cols):
    """slx_edit_record with the column values of one record"""
    ci = {k: v for k, v in cols.items() if plan.adds[k][1] == "ic"}
    cz = {k: v for k, v in cols.items() if plan.adds[k][1] == "Zc"}
    return ed.record(rec, ci, cz)


def test_header_declares_exactly_the_exports():
    text = open(os.path.join(ROOT, "include", "seqlib_amd_edit.h")).read()
    body = text[text.index("#ifndef SEQLIB_AMD_EDIT_H"):]
    declared = re.findall(r"^\s*(?:int|void|int64_t|const char)\s+\*?(slx_\w+)\s*\(", body, re.M)
    assert sorted(declared) == sorted(editio.EDIT_EXPORTS)
    assert all(n.startswith("slx_edit_") for n in declared)
    L = editio.lib()
    for n in editio.EDIT_EXPORTS:
        assert hasattr(L, n), n
    rules = text[:text.index("#ifndef SEQLIB_AMD_EDIT_H")]
    for word in ("FIRST occurrence", "EMPTY value does nothing", "STRICTER than bam_aux_skip", "no test reaches it", "valid until the next apply", "block_size is rewritten", "ClearSeqQualAndTags",
                 "RemoveAllTags", "AddZTag", "AddIntTag", "SLX_EIO", "SLX_EINVAL", "SLX_EUNSUPPORTED", "4096", "No CPU fallback"):
        assert word in rules, word


def test_every_einval_of_the_plan(ed):
    def refused(call, *a):
        with pytest.raises(_ffi.SlxError) as e:
            call(*a)
        assert e.value.code == _ffi.SLX_EINVAL
    for bad in (b"", b"X", b"XAB", b"1A", b"X_", b"X ", b"\xc3\xa4"):
        assert not eu.tag_ok(bad)
        refused(ed.drop_tag, bad)
        refused(ed.add_int, bad, 1)
        refused(ed.add_z, bad, b"v")
        refused(ed.add_int_column, bad, None, -1)
        refused(ed.add_z_column, bad, None, 0, None)
    for good in (b"XA", b"x9", b"Zz", b"a0"):
        assert eu.tag_ok(good)
    ed.add_int(b"NM", 1)
    refused(ed.add_int, b"NM", 2)          # a name twice among the adds, whatever the kinds
    refused(ed.add_z, b"NM", b"v")
    refused(ed.add_int_column, b"NM", None, -1)
    refused(ed.add_z_column, b"NM", None, 0, None)
    ed.add_z_column(b"MD", None, 0, None)
    ed.add_z_column(b"MD", None, 0, None)          # the same column again binds in place
    refused(ed.add_int_column, b"MD", None, -1)
    refused(ed.drop_column, b"NM")         # a constant add is no column; neither is a tag the plan lacks, or one that is no tag
    refused(ed.drop_column, b"XX")
    refused(ed.drop_column, b"X")
    ed.drop_column(b"MD")                  # the column leaves the plan: the name is free again, and the adds behind it moved up
    refused(ed.drop_column, b"MD")
    ed.add_int(b"XQ", 4)
    ed.add_int_column(b"MD", None, -1)
    ed.drop_column(b"MD")
    assert ed.record(dict(eu.REC_CASES)["no_aux"]) == eu.apply(dict(eu.REC_CASES)["no_aux"], eu.Plan(adds=[(b"NM", "i", 1, False), (b"XQ", "i", 4, False)]))
    refused(ed.add_z, b"RG", b"")          # a constant Z value that is empty, or holds a NUL
    refused(ed.add_z, b"RG", b"a\0b")
    ed.plan_clear()
    for k in range(8):
        ed.drop_tag(b"D%d" % k)
        ed.add_int(b"A%d" % k, k)
    refused(ed.drop_tag, b"D9")            # more than 8
    refused(ed.add_int, b"A9", 9)
    refused(ed.add_z, b"Z9", b"v")
    ed.plan_clear()
    ed.add_z(b"Z1", b"v" * 2000)
    ed.add_z(b"Z2", b"v" * 2000)          # 4002 bytes with the NULs
    refused(ed.add_z, b"Z3", b"v" * 94)   # 4097
    ed.add_z(b"Z3", b"v" * 93)            # 4096 exactly
    assert eu.plan_error(eu.Plan(adds=[(b"Z1", "Z", b"v" * 2000, False), (b"Z2", "Z", b"v" * 2000, False), (b"Z3", "Z", b"v" * 94, False)])) == "constants"
    assert eu.plan_error(eu.Plan(adds=[(b"Z1", "Z", b"v" * 2000, False), (b"Z2", "Z", b"v" * 2000, False), (b"Z3", "Z", b"v" * 93, False)])) is None
    refused(ed.set, "long_aux", 0)
    refused(ed.set, "long_aux", 2 ** 31)
    refused(ed.set, "no_such_knob", 1)
    assert ed.counter("no_such_counter") == -1 and ed.counter("long_aux") == 256 and ed.counter("device") == -1


@pytest.mark.parametrize("plan_name", sorted(eu.PLANS))
def test_record_cases_equal_python(ed, plan_name):
    plan = eu.PLANS[plan_name]
    assert eu.plan_error(plan) is None
    eu.configure(ed, plan)
    recs = [r for _, r in eu.REC_CASES]
    cols = eu.column_values(plan, len(recs))
    want = eu.apply_batch(recs, plan, cols)
    for i, (name, r) in enumerate(eu.REC_CASES):
        assert _record(ed, plan, r, {k: v[i] for k, v in cols.items()}) == want[i], name


def test_the_cases_cover_what_they_claim():
    by = dict(eu.REC_CASES)
    f = lambda n: [x[:3] for x in eu.aux_fields(by[n][eu.layout(by[n])[0]:])]
    assert {t[2:3] for t in f("every_type")} == {bytes([c]) for c in b"AcCsSiIfdZHB"} and len(f("every_type")) == 20
    assert {x[3:4] for x in eu.aux_fields(eu.EVERY_TYPE) if x[2:3] == b"B"} == {bytes([c]) for c in b"cCsSiIf"}
    assert f("no_aux") == [] and f("z_only_nul") == [b"MDZ"]
    assert [t[:2] for t in f("cut_first")].index(b"XA") == 0 and [t[:2] for t in f("cut_middle")].index(b"XA") == 1 and [t[:2] for t in f("cut_last")].index(b"XA") == 2
    assert b"XA" not in [t[:2] for t in f("cut_absent")] and [t[:2] for t in f("cut_twice_present")].count(b"XA") == 3
    assert all(t in [x[:2] for x in f("all_8_drops")] for t in eu.DROP8)
    ls = lambda n: struct.unpack_from("<i", by[n], 20)[0]
    nc = lambda n: struct.unpack_from("<H", by[n], 16)[0]
    assert ls("l_seq_0") == 0 and nc("n_cigar_0") == 0 and by["name_1_byte"][12] == 1 and by["name_254_bytes"][12] == 254 and ls("odd_l_seq") == 5
    # only the first of two goes; an add whose name is dropped; INT with and without replace over an existing tag
    drop = eu.apply(by["cut_twice_present"], eu.PLANS["drop_names"])
    assert drop.count(b"XAZ") == 2 and b"first;" not in drop and b"second;" in drop
    two = eu.apply(by["cut_twice_present"], eu.PLANS["drop_xa_twice"])
    assert two.count(b"XAZ") == 1 and b"third;" in two
    assert eu.apply(by["cut_first"], eu.PLANS["add_dropped_name"]).endswith(b"XAZnew\0NMi\x05\0\0\0")
    assert eu.apply(by["has_rg_and_nm"], eu.PLANS["int_no_replace"]).count(b"NMi") == 2 and eu.apply(by["has_rg_and_nm"], eu.PLANS["int_replace"]).count(b"NMi") == 1
    assert eu.apply(by["nm_twice"], eu.PLANS["int_replace"]).count(b"NMi") == 2
    # an empty Z column value and an int equal to `absent` do nothing at all: the old tags stay
    assert eu.apply(by["has_rg_and_nm"], eu.PLANS["columns"], {0: -1, 1: b""}) == by["has_rg_and_nm"]
    got = eu.apply(by["has_rg_and_nm"], eu.PLANS["columns"], {0: 3, 1: b"4A5"})
    assert got.endswith(b"RGZold\0NMi\x03\0\0\0MDZ4A5\0") and len(got) == len(by["has_rg_and_nm"]) + 1
    clear = eu.apply(by["every_type"], eu.PLANS["clear"])
    assert len(clear) == 36 + by["every_type"][12] + 4 and struct.unpack_from("<i", clear, 20)[0] == 0 and struct.unpack_from("<I", clear)[0] == len(clear) - 4
    cols = eu.column_values(eu.PLANS["columns"], 12)
    assert -1 in cols[0] and b"" in cols[1] and {len(v) for v in cols[1]} >= {0, 1, 15, 16, 17}
    for name, r in eu.REC_CASES:
        assert eu.apply(r, eu.PLANS["identity"]) == r, name


def test_bulk_records_equal_python(ed, bulk):
    lens = [len(r) for r in bulk]
    assert len(bulk) == 2000 and max(lens) > 30000 and min(lens) < 60
    for plan_name in ("drop_names", "columns", "adds_8"):
        plan = eu.PLANS[plan_name]
        eu.configure(ed, plan)
        cols = eu.column_values(plan, len(bulk), seed=5)
        want = eu.apply_batch(bulk, plan, cols)
        changed = 0
        for i, r in enumerate(bulk):
            assert _record(ed, plan, r, {k: v[i] for k, v in cols.items()}) == want[i], (plan_name, i)
            changed += want[i] != r
        assert changed > 500


def test_damaged_records_are_eio(ed):
    good = dict(eu.REC_CASES)["every_type"]
    for plan_name in ("identity", "drop_all", "clear", "add_consts"):          # the aux area is parsed whatever the plan does with it
        eu.configure(ed, eu.PLANS[plan_name])
        for bad in ru.truncated(good) + [r for _, r in eu.malformed_aux()]:
            with pytest.raises(eu.BadRecord):
                eu.apply(bad, eu.PLANS[plan_name])
            with pytest.raises(_ffi.SlxError) as e:
                ed.record(bad)
            assert e.value.code == _ffi.SLX_EIO and "record 0 of the batch" in str(e.value)


def test_host_only_handle_answers_enodevice(ed):
    stream, off = ru.stream_of([r for _, r in eu.REC_CASES])
    with pytest.raises(_ffi.SlxError) as e:
        ed.apply_host(stream, off)
    assert e.value.code == _ffi.SLX_ENODEVICE and "batches of records are edited on MI355X only" in str(e.value)
    with pytest.raises(_ffi.SlxError) as e:
        ed.apply_device(None, 0, None, 0)
    assert e.value.code == _ffi.SLX_ENODEVICE and "slx_edit_apply_device" in str(e.value) and "edited on MI355X only" in str(e.value)
    with pytest.raises(_ffi.SlxError) as e:
        ed.to_host(editio.Batch())
    assert e.value.code == _ffi.SLX_ENODEVICE
    with pytest.raises(_ffi.SlxError) as e:
        editio.Editor(-3)
    assert e.value.code == _ffi.SLX_EINVAL


def test_live_bytes_return_after_free():
    L = _ffi.lib()
    before = (L.slx_hip_live_bytes(0), L.slx_hip_live_bytes(1))
    e = editio.Editor(editio.AUTO)
    eu.configure(e, eu.PLANS["add_consts"])
    if e.counter("device") >= 0:
        stream, off = ru.stream_of([r for _, r in eu.REC_CASES])
        b = e.apply_host(stream, off)
        assert b.n_records == len(eu.REC_CASES)
        assert L.slx_hip_live_bytes(0) > before[0]
    e.close()
    assert (L.slx_hip_live_bytes(0), L.slx_hip_live_bytes(1)) == before


def _hexs(b):
    return bytes(b).hex() or "-"


def _plan_lines(plan):
    lines = ["P"] + ["D %s" % t.decode() for t in plan.drops] + (["DA"] if plan.drop_all else []) + (["CL"] if plan.clear else [])
    for tag, kind, value, replace in plan.adds:
        t = tag.decode()
        lines.append("CZ %s" % t if kind == "Zc" else "AZ %s %s" % (t, _hexs(value)) if kind == "Z" else "%s %s %d %d" % ("AI" if kind == "i" else "CI", t, value, replace))
    return lines


def _batch_lines(plan, recs, cols, stream=None, off=None):
    lines = []
    for k, vals in cols.items():
        if plan.adds[k][1] == "ic":
            lines.append("V %d %s" % (k, ",".join(map(str, vals)) or "-"))
        else:
            text, toff = eu.z_column(vals)
            lines.append("T %d %s %s" % (k, _hexs(text), ",".join(map(str, toff))))
    if stream is None:
        stream, off = ru.stream_of(recs)
    bad = eu.first_bad(stream, off)
    if bad is None:
        out, noff = ru.stream_of(eu.apply_batch(recs, plan, cols))
        lines.append("B %d %s %s 0 -1 %s %s" % (len(off) - 1, _hexs(stream), ",".join(map(str, off)), _hexs(out), ",".join(map(str, noff))))
    else:
        lines.append("B %d %s %s 1 %d - -" % (len(off) - 1, _hexs(stream), ",".join(map(str, off)), bad))
    return lines


def test_bodies_under_sanitizers(exe, tmp_path, bulk):
    """the size pass and the tile gather over the record cases under every plan, generated records (long ones that span tiles among them), batches of 0 and 1,
    and refused batches -- every stream, table and column in a heap block of exactly its size: Python's bytes and offsets, with no sanitizer report"""
    cases = [r for _, r in eu.REC_CASES]
    few = sorted(bulk[:400], key=len)[:150] + sorted(bulk, key=len)[-3:]
    lines, n_batches, n_records = [], 0, 0
    for name in sorted(eu.PLANS):
        plan = eu.PLANS[name]
        lines += _plan_lines(plan)
        for recs in (cases, [], cases[:1], few if name in ("drop_names", "columns", "adds_8", "identity", "clear") else cases[3:9]):
            lines += _batch_lines(plan, recs, eu.column_values(plan, len(recs), seed=3))
            n_batches, n_records = n_batches + 1, n_records + len(recs)
    plan = eu.PLANS["drop_names"]
    lines += _plan_lines(plan)
    stream, off = ru.stream_of(cases)
    for k in (1, 5, len(cases) - 1):          # the tail of a batch: the table from entry k on as it stands, the stream from record k on
        lines += _batch_lines(plan, cases[k:], {}, stream[off[k]:], off[k:])
        n_batches, n_records = n_batches + 1, n_records + len(cases) - k
    good = cases[:6]
    for bad_rec in ru.truncated(cases[1]) + [r for _, r in eu.malformed_aux()]:          # a broken record in the middle
        recs = good[:3] + [bad_rec] + good[3:]
        stream, off = ru.stream_of(recs)
        assert eu.first_bad(stream, off) == (4 if len(bad_rec) >= 36 and struct.unpack_from("<I", bad_rec)[0] + 4 != len(bad_rec) else 3)          # (a block_size that passes its span is blamed on the record that starts inside it, as the sorter does)
        lines += _batch_lines(plan, recs, {}, stream, off)
        n_batches += 1
    stream, off = ru.stream_of(good)
    for k, delta in ((0, 4), (3, 4), (3, -4), (6, -1), (6, 1), (2, 10 ** 6), (0, 100), (0, 10 ** 6)):          # a wrong entry of the offset table
        o2 = list(off)
        o2[k] += delta
        assert eu.first_bad(stream, o2) is not None
        lines += _batch_lines(plan, good, {}, stream, o2)
        n_batches += 1
    p = tmp_path / "expect.txt"
    p.write_text("\n".join(lines) + "\n")
    r = subprocess.run([exe, "cases", str(p)], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    assert "edit_host_test OK: %d plans, %d batches, %d records" % (len(eu.PLANS) + 1, n_batches, n_records) in r.stdout
