"""GPU tests of the record editor at the C-ABI (include/seqlib_amd_edit.h through seqlib_amd/editio.py) against the Python statement of the rules in
tests/edit_util.py: the record cases under every kind of plan, batches of 0, 1, 64 and 65, the identity, the knob that must not change a result, record
boundaries, cut boundaries and added tags at the tile edges, every source alignment of a piece, Z column values around the word and the tile size, NM and MD
written back (calmd without leaving HBM), the edited batch taken by the sorter and the BGZF writer, and a broken record in the middle of a batch.  Equality is
exact everywhere."""
import ctypes as C
import os
import struct

import pytest

from tests import bam_util as bu
from tests import edit_util as eu
from tests import ref_util as ru

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")
TILE = 2048


@pytest.fixture(scope="module")
def io(sl):
    import torch
    from seqlib_amd import _ffi, bamio, editio, recio, refio, sortio
    editio.lib()

    class F:
        pass
    f = F()
    f.ffi, f.bamio, f.editio, f.recio, f.refio, f.sortio, f.torch = _ffi, bamio, editio, recio, refio, sortio, torch
    return f


@pytest.fixture(scope="module")
def ed(io):
    e = io.editio.Editor()
    assert e.counter("device") >= 0
    yield e
    e.close()


@pytest.fixture(scope="module")
def bulk():
    return eu.bulk_records()


def upload(io, plan, cols):
    """the columns in HBM: ({add index: pointers to bind}, the tensors that own them)"""
    t, bind, keep = io.torch, {}, []
    for k, vals in cols.items():
        if plan.adds[k][1] == "ic":
            d = t.tensor(vals if vals else [0], dtype=t.int32).cuda()
            keep.append(d)
            bind[k] = (d.data_ptr(),)
        else:
            text, off = eu.z_column(vals)
            dt = t.frombuffer(bytearray(text or b"\0"), dtype=t.uint8).cuda()
            do = t.tensor(off, dtype=t.int64).cuda()
            keep += [dt, do]
            bind[k] = (dt.data_ptr(), len(text), do.data_ptr())
    t.cuda.synchronize()          # (torch copies on its own stream, the editor reads on its own)
    return bind, keep


def run(io, ed, plan, recs, cols=None, stream_off=None):
    """-> (edited stream, offsets) of a host batch under the plan"""
    cols = cols or {}
    bind, keep = upload(io, plan, cols)
    eu.configure(ed, plan, bind)
    stream, off = stream_off or ru.stream_of(recs)
    b = ed.apply_host(stream, off)
    io.torch.cuda.synchronize()
    del keep
    return ed.to_host(b)


def check(io, ed, plan, recs, cols=None):
    want, woff = ru.stream_of(eu.apply_batch(recs, plan, cols))
    got, off = run(io, ed, plan, recs, cols)
    assert off == woff
    if got != want:
        k = next(i for i in range(len(recs)) if got[off[i]:off[i + 1]] != want[off[i]:off[i + 1]])
        at = next(j for j in range(len(want)) if got[j] != want[j])
        raise AssertionError("record %d differs, first at stream byte %d (tile %d + %d)" % (k, at, at // TILE, at % TILE))
    assert ed.counter("records") == len(recs) and ed.counter("bytes_in") == sum(map(len, recs)) and ed.counter("bytes_out") == len(want)
    return got, off


def padded(name, pad, aux_front=b"", aux_back=b""):
    """a record with a Z tag PD of `pad` value bytes between aux_front and aux_back"""
    return ru.raw_record(name, 0, 0, 4, [(0, 4)], "ACGT", aux=aux_front + b"PDZ" + b"p" * pad + b"\0" + aux_back)


# ---------------------------------------------------------------- the cases, the batch sizes, the identity, the knob
@pytest.mark.parametrize("plan_name", sorted(eu.PLANS))
def test_record_cases_under_every_plan(io, ed, plan_name):
    plan = eu.PLANS[plan_name]
    recs = [r for _, r in eu.REC_CASES]
    check(io, ed, plan, recs, eu.column_values(plan, len(recs)))


@pytest.mark.parametrize("n", [0, 1, 64, 65])
def test_batches_of(io, ed, bulk, n):
    short = [r for r in bulk if len(r) < 300]
    for plan_name in ("columns", "drop_names", "clear_then_add"):
        plan = eu.PLANS[plan_name]
        got, off = check(io, ed, plan, short[:n], eu.column_values(plan, n, seed=n))
        assert len(off) == n + 1 and off[0] == 0


def test_identity_returns_the_input(io, ed, bulk):
    recs = [r for _, r in eu.REC_CASES] + bulk[:300]
    stream, off = ru.stream_of(recs)
    assert run(io, ed, eu.PLANS["identity"], recs) == (stream, off)
    assert ed.counter("us_size") > 0 and ed.counter("us_scan") > 0 and ed.counter("us_gather") > 0


def test_long_aux_changes_nothing(io, bulk):
    recs = [r for _, r in eu.REC_CASES] + bulk[:600]
    plan = eu.PLANS["columns_no_replace"]
    cols = eu.column_values(plan, len(recs), seed=9)
    aux_len = [len(r) - eu.layout(r)[0] for r in recs]
    e = io.editio.Editor()
    default = e.counter("long_aux")
    want_long = {1: sum(a >= 1 for a in aux_len), default: sum(a >= default for a in aux_len), 2 ** 31 - 1: 0}
    assert 0 < want_long[default] < want_long[1] < len(recs)          # by default both forms run
    for knob in (1, default, 2 ** 31 - 1):
        e.set("long_aux", knob)
        check(io, e, plan, recs, cols)
        assert e.counter("long_records") == want_long[knob]
        check(io, e, eu.PLANS["drop_xa_twice"], recs)
    e.close()


def test_device_batch_and_refusals_of_the_call(io, ed):
    t = io.torch
    recs = [r for _, r in eu.REC_CASES]
    stream, off = ru.stream_of(recs)
    plan = eu.PLANS["add_dropped_name"]
    eu.configure(ed, plan)
    d_s, d_o = t.frombuffer(bytearray(stream), dtype=t.uint8).cuda(), t.tensor(off, dtype=t.int64).cuda()
    t.cuda.synchronize()
    b = ed.apply_device(d_s.data_ptr(), len(stream), d_o.data_ptr(), len(recs))
    assert ed.to_host(b) == ru.stream_of(eu.apply_batch(recs, plan))
    with pytest.raises(io.ffi.SlxError) as e:          # the handle's own last result
        ed.apply_device(b.d_stream, b.n_bytes, b.d_rec_off, b.n_records)
    assert e.value.code == io.ffi.SLX_EINVAL and "own last result" in str(e.value)
    other = io.editio.Editor()                            # ... is another handle's input without a host copy
    eu.configure(other, eu.PLANS["drop_all"])
    b = ed.apply_device(d_s.data_ptr(), len(stream), d_o.data_ptr(), len(recs))
    b2 = other.apply_device(b.d_stream, b.n_bytes, b.d_rec_off, b.n_records)
    assert other.to_host(b2) == ru.stream_of(eu.apply_batch(eu.apply_batch(recs, plan), eu.PLANS["drop_all"]))
    other.close()
    with pytest.raises(io.ffi.SlxError) as e:          # not the last result any more
        ed.to_host(io.editio.Batch(1, 40, b.d_stream, b.d_rec_off))
    assert e.value.code == io.ffi.SLX_EINVAL
    plan = eu.PLANS["columns"]
    cols = eu.column_values(plan, len(recs))
    check(io, ed, plan, recs, cols)
    with pytest.raises(io.ffi.SlxError) as e:          # columns are bound for one apply
        ed.apply_host(stream, off)
    assert e.value.code == io.ffi.SLX_EINVAL and "not bound" in str(e.value)
    bind, keep = upload(io, plan, {0: cols[0], 1: cols[1]})
    eu.configure(ed, plan, {0: bind[0], 1: (bind[1][0], bind[1][1] - 1, bind[1][2])})          # offsets that pass n_text
    with pytest.raises(io.ffi.SlxError) as e:
        ed.apply_host(stream, off)
    assert e.value.code == io.ffi.SLX_EINVAL and "Z column" in str(e.value)


# ---------------------------------------------------------------- tile edges
@pytest.mark.parametrize("target", [2047, 2048, 2049])
def test_features_at_a_tile_edge(io, ed, target):
    """a record boundary, the byte behind a cut, and an added tag's header byte, each placed at output offset `target`; then the same one tile further on"""
    plan = eu.Plan(drops=[b"XA"], adds=[(b"RG", "Z", b"grp", False), (b"NM", "ic", -1, True), (b"MD", "Zc", None, False)])
    back = b"ASi\x07\0\0\0" + b"XAZchr9,+1,4M,0;\0" + b"KPZkept behind the cut\0"
    tail = [padded("t%d" % i, 3 * i, aux_back=back) for i in range(4)]
    for extra in (0, TILE):
        for feature in ("record", "cut", "add", "value"):
            def batch(pad):
                recs = [padded("first", pad)] + ([padded("filler", extra - 60)] if extra else []) + [padded("second", 5, aux_back=back)] + tail
                k = len(recs) - 5          # "second"
                cols = {1: [3, -1, 7, 9, -1, 2, 4][:len(recs)], 2: [b"10", b"", b"9", b"7", b"1^AC3", b"", b"2"][:len(recs)]}
                cols[1][k], cols[2][k] = 8, b"4A5"
                out = eu.apply_batch(recs, plan, cols)
                start = sum(map(len, out[:k]))
                at = {"record": start, "cut": start + out[k].index(b"KPZ"), "add": start + out[k].index(b"RGZgrp"), "value": start + out[k].index(b"MDZ") + 3}[feature]
                return recs, cols, at
            _, _, at0 = batch(0)
            assert at0 < target + extra
            recs, cols, at = batch(target + extra - at0)          # (a byte more in the first record moves everything behind it by one)
            assert at == target + extra, (feature, at)
            check(io, ed, plan, recs, cols)


@pytest.mark.parametrize("total", [1000, 2048, 2049, 4096])
def test_total_output_sizes(io, ed, total):
    plan = eu.Plan(drops=[b"XA"], adds=[(b"RG", "Z", b"grp", False)])
    mk = lambda pad: [padded("one", pad, aux_back=b"XAZgone\0"), padded("two", 0)]
    base = sum(map(len, eu.apply_batch(mk(0), plan)))
    recs = mk(total - base)
    assert sum(map(len, eu.apply_batch(recs, plan))) == total
    check(io, ed, plan, recs)


def test_a_record_and_a_value_that_span_tiles(io, ed, bulk):
    long_rec = max(bulk, key=len)
    assert struct.unpack_from("<i", long_rec, 20)[0] == 20000 and len(long_rec) > 10 * TILE
    recs = [padded("before", 7), long_rec, padded("after", 9, aux_back=b"MDZold\0")]
    plan = eu.PLANS["columns"]
    cols = {0: [1, 2, 3], 1: [b"5", b"M" * 5000, b"6"]}
    check(io, ed, plan, recs, cols)
    cols = {0: [1, -1, 3], 1: [b"T" * 5000, b"", b"V" * 2500]}
    check(io, ed, plan, recs, cols)
    check(io, ed, eu.PLANS["clear"], recs)


# ---------------------------------------------------------------- source alignment
def test_every_source_alignment_of_a_kept_piece(io, ed):
    """the kept range between two cuts starts at all 16 residues mod 16 with lengths 0 and 4..40 (an aux field has 4 bytes at least): head bytes, whole words and
    tail bytes of the gather.  apply_host stages the stream at the front of an allocation, so a stream offset's residue is the address's."""
    plan = eu.Plan(drops=[b"XA", b"SA"])
    recs, seen = [], set()
    at = 0
    for length in [0] + list(range(4, 41)):
        for res in range(16):
            mid = b"" if length == 0 else b"KPZ" + b"k" * (length - 4) + b"\0"
            name = "r"
            while True:          # the name's length moves the piece to the residue wanted
                r = ru.raw_record(name, 0, 0, 4, [(0, 4)], "ACGT", aux=b"XAZcut one\0" + mid + b"SAZcut two\0")
                start = at + r.index(b"XAZcut one\0") + 11
                if start % 16 == res:
                    break
                name += "r"
            recs.append(r)
            seen.add((start % 16, length))
            at += len(r)
    assert seen == {(res, length) for res in range(16) for length in [0] + list(range(4, 41))}
    check(io, ed, plan, recs)


@pytest.mark.parametrize("lengths", [list(range(0, 41)) * 2 + [3], [0, 1, 15, 16, 17, 2047, 2048, 0, 5]], ids=["0_to_40", "word_and_tile"])
def test_z_column_value_lengths(io, ed, lengths):
    """values of every length 0..40 at changing residues of the text offset, and the lengths around the word and the tile size; an int column with `absent`"""
    plan = eu.Plan(adds=[(b"NM", "ic", -1, True), (b"MD", "Zc", None, False)])
    vals = [bytes(65 + (i + j) % 26 for j in range(n)) for i, n in enumerate(lengths)]
    off = eu.z_column(vals)[1]
    if len(lengths) > 50:
        assert {(o % 16) for o in off} == set(range(16)) and len({(o % 16, n) for o, n in zip(off, lengths)}) >= 75
    recs = [padded("z%d" % i, i % 23, aux_front=b"NMi\x63\0\0\0", aux_back=b"MDZold\0") for i in range(len(lengths))]
    ints = [-1 if i % 3 == 1 else i for i in range(len(lengths))]
    got, goff = check(io, ed, plan, recs, {0: ints, 1: vals})
    assert got[goff[1]:goff[2]].count(b"NMi\x63") == 1 and got[goff[2]:goff[3]].count(b"NMi\x63") == 0          # absent: nothing at all
    assert b"MDZold\0" in got[goff[0]:goff[1]] and b"MDZold\0" not in got[goff[1]:goff[2]]                      # an empty value: nothing at all


# ---------------------------------------------------------------- calmd end to end
def test_nm_md_written_back(io, sl, tiny_gpu, ed):
    """the golden reads aligned, built into records in HBM, NM and MD computed there and written back there: every record equals the Python statement applied
    to the builder's record; on forward-strand records the NM written is the one the aligner wrote (the independence argument of test_nm_equals_the_aligners)"""
    ref = io.refio.Ref(os.path.join(GOLDEN, "tiny.fa"))
    al = sl.BWAAligner(tiny_gpu)
    L = open(os.path.join(GOLDEN, "sim1_bcr.head3000.fq")).read().split("\n")
    names, seqs = [L[i][1:].split()[0].encode() for i in range(0, len(L) - 3, 4)], [L[i + 1].encode() for i in range(0, len(L) - 3, 4)]
    rb = io.recio.Builder(al._handle())
    d_bases, d_offs, d_names, d_name_offs = rb.upload(seqs, names)
    hits = al.align_device(d_bases, d_offs, len(seqs), 0, False, 0.9, 10)
    b = rb.build(hits, d_bases, d_offs, d_names, d_name_offs, False)
    m = io.refio.Md()
    io.ffi.check(io.refio.lib().slx_ref_nm_md_device(ref.h, b.d_stream, b.n_bytes, b.d_rec_off, b.n_records, None, 0, C.byref(m)))
    nm, md = ref._down(m)
    plan = eu.Plan(drops=[b"XS"], adds=[(b"NM", "ic", -1, True), (b"MD", "Zc", None, False), (b"RG", "Z", b"sim1", False)])
    eu.configure(ed, plan, {0: (m.d_nm,), 1: (m.d_md, m.md_bytes, m.d_md_off)})
    out = ed.apply_device(b.d_stream, b.n_bytes, b.d_rec_off, b.n_records)
    got, off = ed.to_host(out)
    stream, soff = rb.to_host(b)
    recs = [stream[soff[i]:soff[i + 1]] for i in range(b.n_records)]
    want = eu.apply_batch(recs, plan, {0: nm, 1: md})
    n_fwd = n_unmapped = 0
    for i, w in enumerate(want):
        g = got[off[i]:off[i + 1]]
        assert g == w, i
        flag = struct.unpack_from("<H", recs[i], 18)[0]
        fields = eu.aux_fields(g[eu.layout(g)[0]:])
        if nm[i] < 0:
            n_unmapped += 1
            assert g == eu.apply(recs[i], eu.Plan(drops=[b"XS"], adds=[(b"RG", "Z", b"sim1", False)]))          # the old tags are left alone
            continue
        assert [f[:3] for f in fields[-3:]] == [b"NMi", b"MDZ", b"RGZ"] and sum(f[:2] == b"NM" for f in fields) == 1 and fields[-2] == b"MDZ" + md[i] + b"\0"
        if not flag & 16:
            old = [f for f in eu.aux_fields(recs[i][eu.layout(recs[i])[0]:]) if f[:2] == b"NM"]
            assert len(old) == 1 and old[0][3:] == fields[-3][3:] == struct.pack("<i", nm[i])
            n_fwd += 1
    assert n_fwd >= 1400 and len(want) == b.n_records >= n_fwd + n_unmapped
    rb.close()
    ref.close()


# ---------------------------------------------------------------- downstream
def test_the_edited_batch_is_accepted_downstream(io, ed, tmp_path):
    recs = list(bu.sample_records(400))
    plan = eu.Plan(drops=[b"NM", b"XA"], adds=[(b"RG", "Z", b"lane.7", False), (b"XI", "ic", 0, False)])
    cols = {1: [i % 4 for i in range(len(recs))]}
    want = eu.apply_batch(recs, plan, cols)
    assert sum(w != r for w, r in zip(want, recs)) == len(recs)
    bind, keep = upload(io, plan, cols)
    eu.configure(ed, plan, bind)
    b = ed.apply_host(*ru.stream_of(recs))
    s = io.sortio.Sorter()
    s.add_device(b.d_stream, b.n_bytes, b.d_rec_off, b.n_records)
    got, off, perm = s.to_host()
    key = lambda r: (struct.unpack_from("<i", r, 4)[0] & 0xffffffff, struct.unpack_from("<i", r, 8)[0])
    assert [got[off[i]:off[i + 1]] for i in range(len(recs))] == sorted(want, key=key)
    s.close()
    path = tmp_path / "edited.bam"
    w = io.bamio.Writer(path)
    w.write(bu.bam_header(bu.TEXT, bu.REFS))
    w.write_device(b.d_stream, b.n_bytes)
    w.close()
    text, refs, back = bu.parse_bam(path.read_bytes())
    assert [r["raw"] for r in back] == want and refs == list(bu.REFS)
    rd = io.bamio.Reader(path)          # ... and the reader reads it back record for record
    served = []
    while True:
        got, _ = rd.next(0x6000)
        if not got:
            break
        served += got
    rd.close()
    assert served == want


# ---------------------------------------------------------------- a broken record
def test_a_broken_record_fails_the_call_and_the_next_succeeds(io, ed, bulk):
    """every such input lies inside its allocation: the offsets stay inside the stream, the record without a NUL ends where its block_size says"""
    good = [r for r in bulk if len(r) < 400][:200]
    plan = eu.PLANS["add_consts"]
    no_nul = ru.raw_record("no_nul", 0, 0, 4, [(0, 4)], "ACGT", aux=b"NMi\x01\0\0\0XAZchr1,+5,4M,0;")
    batch = good[:117] + [no_nul] + good[118:]
    stream, off = ru.stream_of(batch)
    wrong = off[:117] + [off[117] + 4] + off[118:]
    gstream, goff = ru.stream_of(good)
    for s, o in ((stream, off), (gstream, wrong)):
        assert eu.first_bad(s, o) == 117
        eu.configure(ed, plan)
        with pytest.raises(io.ffi.SlxError) as e:
            ed.apply_host(s, o)
        assert e.value.code == io.ffi.SLX_EIO and "record 117 of the batch" in str(e.value)
        check(io, ed, plan, good)
    for knob in (1, 2 ** 31 - 1):          # the wave form finds the missing NUL too
        e2 = io.editio.Editor(long_aux=knob)
        eu.configure(e2, plan)
        with pytest.raises(io.ffi.SlxError) as e:
            e2.apply_host(stream, off)
        assert e.value.code == io.ffi.SLX_EIO and "record 117 of the batch" in str(e.value)
        e2.close()


@pytest.mark.parametrize("long_aux", [1, None, 2 ** 31 - 1], ids=["all_waves", "default", "all_lanes"])
def test_the_first_of_two_broken_records_is_named(io, bulk, long_aux):
    """the earlier broken record has a long aux area (a wave walks it by default, after the lanes have walked the short ones), the later one a short one: the
    call names the earlier one whichever form walks which, so the knob changes no error either"""
    good = [r for r in bulk if len(r) < 400][:200]
    long_bad = ru.raw_record("long_no_nul", 0, 0, 4, [(0, 4)], "ACGT", aux=b"NMi\x01\0\0\0XAZ" + b"chr1,+5,4M,0;" * 40)
    short_bad = ru.raw_record("short_bad", 0, 0, 4, [(0, 4)], "ACGT", aux=b"XAQ\x01")
    assert len(long_bad) - eu.layout(long_bad)[0] > 256 > len(short_bad)
    e = io.editio.Editor()
    if long_aux:
        e.set("long_aux", long_aux)
    eu.configure(e, eu.PLANS["drop_names"])
    for first, second in ((long_bad, short_bad), (short_bad, long_bad)):
        batch = good[:100] + [first] + good[101:150] + [second] + good[151:]
        stream, off = ru.stream_of(batch)
        assert eu.first_bad(stream, off) == 100
        with pytest.raises(io.ffi.SlxError) as err:
            e.apply_host(stream, off)
        assert err.value.code == io.ffi.SLX_EIO and "record 100 of the batch" in str(err.value)
    check(io, e, eu.PLANS["drop_names"], good)
    e.close()


def test_the_tail_of_a_batch(io, ed):
    """the offsets count from the first entry given: record k on of a batch in HBM is the stream pointer moved up, the table from entry k on as it stands"""
    t = io.torch
    recs = [r for _, r in eu.REC_CASES]
    stream, off = ru.stream_of(recs)
    plan = eu.PLANS["add_dropped_name"]
    d_s, d_o = t.frombuffer(bytearray(stream), dtype=t.uint8).cuda(), t.tensor(off, dtype=t.int64).cuda()
    t.cuda.synchronize()
    for k in (0, 1, 7, len(recs) - 1):
        eu.configure(ed, plan)
        b = ed.apply_device(d_s.data_ptr() + off[k], len(stream) - off[k], d_o.data_ptr() + 8 * k, len(recs) - k)
        got, goff = ed.to_host(b)
        assert (got, goff) == ru.stream_of(eu.apply_batch(recs[k:], plan)) and goff[0] == 0
    with pytest.raises(io.ffi.SlxError) as e:          # the whole stream under the tail's table: the last record no longer ends at n_bytes
        ed.apply_device(d_s.data_ptr(), len(stream), d_o.data_ptr() + 8, len(recs) - 1)
    assert e.value.code == io.ffi.SLX_EIO
