"""GPU tests of the read statistics at the C-ABI (include/seqlib_amd_stats.h through seqlib_amd/statsio.py) against the Python statement of the rules in
tests/stats_util.py: every case and the bulk records counter for counter and bin for bin, the knobs that must not change a result, the group table (no group,
one, as many as LDS holds and one more, more than one round of registration, a group first seen in a later batch, first-appearance order), the entries
(host and device, merge, clear, text, the two eligibility knobs, failures), and batches that come from the BAM reader with a filter and with regions.  Equality is
exact everywhere.  The C++ classes are driven in tests/test_cpp_stats.py."""
import struct

import pytest

from tests import bam_util as bu
from tests import filter_util as fu
from tests import stats_util as su

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def io(sl):
    from seqlib_amd import _ffi, bamio, filterio, recio, statsio
    statsio.lib()

    class F:
        pass
    f = F()
    f.ffi, f.bamio, f.filterio, f.recio, f.statsio = _ffi, bamio, filterio, recio, statsio
    return f


@pytest.fixture(scope="module")
def data():
    """the cases and the bulk records, parsed once, and what they must give"""
    recs = su.GOOD + su.bulk()
    parsed = [su.parse(r) for r in recs]
    return recs, parsed, su.accumulate(parsed)


def make(io, recs, pieces=1, **knobs):
    s = io.statsio.Stats(**knobs)
    step = max(1, -(-len(recs) // pieces))
    for i in range(0, len(recs), step):
        s.add_host(*su.stream_of(recs[i:i + step]))
    return s


def same(got, want):
    assert [g[0] for g in got] == [w[0] for w in want]
    for (name, gc, gh), (_, wc, wh) in zip(got, want):
        assert gc == wc, (name, {k: (gc[k], wc[k]) for k in gc if gc[k] != wc[k]})
        for h in su.HISTS:
            assert tuple(gh[h]) == tuple(wh[h]), (name, h, gh[h][1:], wh[h][1:], [(k, a, b) for k, (a, b) in enumerate(zip(gh[h][0], wh[h][0])) if a != b][:5])


def rec_of(group, i=0, flag=0, mapq=60):
    return bu.bam_record("r%d" % i, flag, 0, 100 + i, mapq, [("M", 8)], "ACGTACGT", bytes([30 + i % 5]) * 8, b"NMC\1RGZ" + group + b"\0")


def test_counts(io, data):
    recs, parsed, want = data
    s = make(io, recs)
    same(s.groups(), want)
    n_long = sum(len(r) > 4096 for r in recs)
    assert s.counter("records_seen") == s.counter("records_counted") == len(recs) and s.counter("long_records") >= n_long >= 2
    assert s.counter("group_misses") == len(recs) and s.counter("adds_lds") > 0 and s.counter("us_add") > 0
    assert len(want) > 12 and sum(c["reads"] for _, c, _ in want) == len(recs)
    s.close()


@pytest.mark.parametrize("knobs", [dict(lds_groups=0), dict(lds_groups=1), dict(lds_groups=2), dict(lds_groups=16), dict(window_bytes=64), dict(window_bytes=64, lds_groups=0),
                                   dict(window_bytes=32768), dict(long_record=1), dict(long_record=1, lds_groups=0), dict(group_slots=2), dict(group_slots=2, window_bytes=80, lds_groups=1, long_record=300)],
                         ids=lambda k: "-".join("%s=%d" % x for x in k.items()))
def test_knobs_never_change_a_result(io, data, knobs):
    recs, parsed, want = data
    s = make(io, recs, pieces=3, **knobs)
    same(s.groups(), want)
    assert s.text() == su.text(want)
    assert s.counter("records_counted") == len(recs)
    if knobs.get("lds_groups", 1) == 0:
        assert s.counter("adds_lds") == 0 and s.counter("adds_global") > 0
    if knobs.get("long_record") == 1:
        assert s.counter("long_records") == len(recs)          # a wave for every record
    if knobs.get("window_bytes") == 64:
        assert s.counter("long_records") >= sum(len(r) > 64 + 2048 for r in recs) >= 2          # records that exceed the stage: the two of 30001 bases at least
    s.close()


def test_no_group_and_an_empty_batch(io):
    s = io.statsio.Stats()
    assert s.n_groups() == 0 and s.groups() == [] and s.text() == su.HEADER.encode() and s.group_name(0) is None
    s.add_host(b"", [0])
    s.add_device(None, 0, None, 0)
    assert s.n_groups() == 0 and s.counter("records_seen") == 0
    with pytest.raises(io.ffi.SlxError) as e:
        s.counter_of(0, "reads")
    assert e.value.code == io.ffi.SLX_EINVAL
    s.close()


@pytest.mark.parametrize("n_groups", [1, 2, 3, 67])
def test_as_many_groups_as_lds_holds_and_one_more(io, n_groups):
    """lds_groups = 2: one group, as many as LDS holds, one more, and many"""
    recs = [rec_of(b"grp%03d" % ((i * 7) % n_groups), i, flag=(0x400 if i % 3 == 0 else 0)) for i in range(400)]
    want = su.accumulate([su.parse(r) for r in recs])
    s = make(io, recs, lds_groups=2)
    same(s.groups(), want)
    assert len(want) == n_groups and s.counter("adds_lds") > 0 and (s.counter("adds_global") > 0) == (n_groups > 2)
    s.close()


def test_one_add_per_wave_where_the_wave_agrees(io):
    """one group, equal records: a wave of 64 adds once per counter, not 64 times"""
    recs = [rec_of(b"only", 0)] * 640
    s = make(io, recs)
    s.add_host(*su.stream_of(recs))          # the group is known now: one launch
    same(s.groups(), su.accumulate([su.parse(r) for r in recs] * 2))
    assert s.counter("adds_lds") < 2 * 640 * 9 / 16 and s.counter("adds_global") == 0 and s.counter("group_misses") == 640
    s.close()


def test_more_groups_than_one_round_registers(io):
    """4500 groups in one batch: the host registers 4096 lowest marked records a round; the order is that of first appearance"""
    recs = [rec_of(b"g%05d" % (i if i < 4500 else i % 97), i) for i in range(4700)]
    want = su.accumulate([su.parse(r) for r in recs])
    s = make(io, recs, group_slots=2)
    assert s.n_groups() == 4500 and [s.group_name(i) for i in (0, 1, 4095, 4096, 4499)] == [b"g00000", b"g00001", b"g04095", b"g04096", b"g04499"]
    pick = list(range(100)) + list(range(4400, 4500))
    same([s.group(i) for i in pick], [want[i] for i in pick])
    assert [s.counter_of(i, "reads") for i in range(4500)] == [c["reads"] for _, c, _ in want]
    s.close()


def test_a_group_first_seen_in_the_second_batch_and_a_repeated_batch(io):
    a = [rec_of(b"beta", 0), rec_of(b"alpha", 1), rec_of(b"beta", 2)]
    b = [rec_of(b"alpha", 3), rec_of(b"gamma", 4), rec_of(b"", 5), rec_of(b"beta", 6)]
    s = make(io, a)
    assert [s.group_name(i) for i in range(s.n_groups())] == [b"beta", b"alpha"] and s.counter("group_misses") == 3
    s.add_host(*su.stream_of(b))
    assert [s.group_name(i) for i in range(s.n_groups())] == [b"beta", b"alpha", b"gamma", b"QNAMED_NA"] and s.counter("group_misses") == 5
    s.add_host(*su.stream_of(b))
    s.add_host(*su.stream_of(a))
    assert s.counter("group_misses") == 5          # nothing new: one launch per batch
    same(s.groups(), su.accumulate([su.parse(r) for r in a + b + b + a]))
    s.close()


def test_add_host_equals_add_device(io, data):
    import torch
    recs, parsed, want = data
    stream, off = su.stream_of(recs)
    d_stream = torch.frombuffer(bytearray(stream), dtype=torch.uint8).cuda()
    d_off = torch.tensor(off, dtype=torch.int64).cuda()
    torch.cuda.synchronize()
    s = io.statsio.Stats()
    s.add_device(d_stream.data_ptr(), len(stream), d_off.data_ptr(), len(recs))
    same(s.groups(), want)
    # from an odd address: the stage keeps the source's alignment
    d_odd = torch.zeros(len(stream) + 3, dtype=torch.uint8).cuda()
    d_odd[3:] = d_stream
    torch.cuda.synchronize()
    t = io.statsio.Stats()
    t.add_device(d_odd.data_ptr() + 3, len(stream), d_off.data_ptr(), len(recs))
    same(t.groups(), want)
    s.close()
    t.close()


def test_merge_clear_and_text(io, data):
    recs, parsed, want = data
    half = len(recs) // 2
    a, b = make(io, recs[:half]), make(io, recs[half:], lds_groups=0)
    a.merge(b)
    same(a.groups(), want)
    assert a.text() == su.text(want) and a.text().count(b"\n") == len(want) + 1
    same(b.groups(), su.accumulate(parsed[half:]))          # the source stands as it was
    a.add_host(*su.stream_of(recs[:50]))                    # and the merged object goes on counting
    same(a.groups(), su.accumulate(parsed + parsed[:50]))
    a.clear()
    assert a.n_groups() == 0 and a.text() == su.HEADER.encode() and a.counter("records_seen") == 0
    a.add_host(*su.stream_of(recs[half:]))
    same(a.groups(), su.accumulate(parsed[half:]))
    c = io.statsio.Stats(len_max=300)
    with pytest.raises(io.ffi.SlxError) as e:
        c.merge(a)
    assert e.value.code == io.ffi.SLX_EINVAL
    with pytest.raises(io.ffi.SlxError) as e:
        a.set("len_max", 300)          # after the first add
    assert e.value.code == io.ffi.SLX_EINVAL
    for x in (a, b, c):
        x.close()


def test_len_max_and_isize_max(io, data):
    recs, parsed, _ = data
    s = make(io, recs, len_max=300, isize_max=1005)
    same(s.groups(), su.accumulate(parsed, len_max=300, isize_max=1005))
    assert s.text() == su.text(su.accumulate(parsed, len_max=300, isize_max=1005), len_max=300, isize_max=1005)
    s.close()


@pytest.mark.parametrize("exclude_flags,min_mapq", [(0x400, 0), (0, 30), (0x704, 17)])
def test_exclude_flags_and_min_mapq(io, data, exclude_flags, min_mapq):
    recs, parsed, _ = data
    want = su.accumulate(parsed, exclude_flags=exclude_flags, min_mapq=min_mapq)
    for knobs in (dict(), dict(long_record=1)):
        s = make(io, recs, exclude_flags=exclude_flags, min_mapq=min_mapq, **knobs)
        same(s.groups(), want)
        n = sum(c["reads"] for _, c, _ in want)
        assert s.counter("records_seen") == len(recs) and s.counter("records_counted") == n < len(recs)
        s.close()


def test_a_damaged_record_fails_the_call(io):
    good = su.GOOD[:10]
    for name, bad in fu.damaged().items():
        for knobs in (dict(), dict(long_record=1)):
            s = io.statsio.Stats(**knobs)
            with pytest.raises(io.ffi.SlxError, match="record 3 of the batch") as e:
                s.add_host(*su.stream_of(good[:3] + [bad] + good[3:]))
            assert e.value.code == io.ffi.SLX_EIO, name
            s.close()
    s = io.statsio.Stats()
    stream, off = su.stream_of(good)
    for bad_off in (off[:-1] + [off[-1] + 4], [0, off[2], off[1]] + off[3:]):          # an offset past the stream; offsets that run backwards
        with pytest.raises(io.ffi.SlxError, match="of the batch") as e:
            s.add_host(stream, bad_off)
        assert e.value.code == io.ffi.SLX_EIO
    s.clear()
    s.add_host(stream, off)
    same(s.groups(), su.accumulate([su.parse(r) for r in good]))
    s.close()


def test_a_key_of_256_bytes_fails_the_call(io):
    by = dict(su.CASES)
    for name in su.FAILING:
        for knobs in (dict(), dict(long_record=1)):
            s = io.statsio.Stats(**knobs)
            with pytest.raises(io.ffi.SlxError, match="record 2 of the batch") as e:
                s.add_host(*su.stream_of(su.GOOD[:2] + [by[name]] + su.GOOD[2:5]))
            assert e.value.code == io.ffi.SLX_EUNSUPPORTED, name
            s.close()


def test_max_groups_stops_a_group_per_read(io):
    recs = [rec_of(b"g%02d" % (i % 11), i) for i in range(60)]
    s = make(io, recs[:10], max_groups=10)          # ten groups: as many as allowed
    assert s.n_groups() == 10
    s.add_host(*su.stream_of(recs[:10]))
    with pytest.raises(io.ffi.SlxError, match="record 0 of the batch opens one read group more than max_groups = 10") as e:
        s.add_host(*su.stream_of(recs[10:]))
    assert e.value.code == io.ffi.SLX_EUNSUPPORTED and s.n_groups() == 10
    s.clear()          # (the object holds an unspecified part of the refused batch)
    s.add_host(*su.stream_of(recs[:10] * 2))
    t = make(io, recs[10:12])          # g10, g00
    with pytest.raises(io.ffi.SlxError, match="nothing was merged") as e:
        s.merge(t)
    assert e.value.code == io.ffi.SLX_EUNSUPPORTED
    same(s.groups(), su.accumulate([su.parse(r) for r in recs[:10] * 2]))
    s.set("max_groups", 11)
    s.merge(t)
    same(s.groups(), su.accumulate([su.parse(r) for r in recs[:10] * 2 + recs[10:12]]))
    s.close()
    t.close()


def test_more_records_than_the_stream_can_hold(io):
    s = io.statsio.Stats()
    for stream, off in ((b"", [0, 0]), (b"x" * 40, [0, 20, 40])):
        with pytest.raises(io.ffi.SlxError) as e:
            s.add_host(stream, off)
        assert e.value.code == io.ffi.SLX_EIO
    s.close()


def drain(rd, s, max_bytes):
    """-> the records the reader served, in order, all of them added from HBM"""
    served, n_batches = [], 0
    while True:
        recs, b = rd.next(max_bytes)
        if not b.n_records:
            return served, n_batches
        s.add_device(b.d_stream, b.n_bytes, b.d_rec_off, b.n_records)
        served += recs
        n_batches += 1


def test_through_the_bam_reader(io, tmp_path):
    recs = [r for r in su.bulk() if len(r) < 3000]
    key = lambda r: (struct.unpack_from("<i", r, 4)[0] & 0xffffffff, struct.unpack_from("<i", r, 8)[0])
    placed = lambda r: 0 <= struct.unpack_from("<i", r, 4)[0] < 3 and struct.unpack_from("<i", r, 8)[0] >= 0
    recs = sorted((r for r in recs if placed(r) or struct.unpack_from("<i", r, 4)[0] < 0), key=key)          # the unplaced ones sort last
    p = tmp_path / "sorted.bam"
    p.write_bytes(bu.bam_bytes(bu.TEXT, bu.REFS, recs, member_size=4000))
    io.bamio.index_build(p)
    rd = io.bamio.Reader(p)
    s = io.statsio.Stats()
    served, n_batches = drain(rd, s, 8000)
    assert served == recs and n_batches >= 3
    same(s.groups(), su.accumulate([su.parse(r) for r in recs]))
    s.close()
    # a mapq filter attached to the reader: the batches hold the kept records only
    flt = io.filterio.Filter([dict(rules=[dict(mapq=(30, 255, False))])])
    flt.attach(rd)
    rd.rewind()
    s = io.statsio.Stats()
    served, n_batches = drain(rd, s, 8000)
    assert served == [r for r in recs if r[13] >= 30] and 0 < len(served) < len(recs) and n_batches >= 3
    same(s.groups(), su.accumulate([su.parse(r) for r in served]))
    s.close()
    io.filterio.Filter.detach(rd)
    # two regions that overlap: a record is served, and counted, once per region it overlaps
    rd.index_load()
    rd.set_regions([(0, 1000, 2000), (0, 1990, 2600)])
    s = io.statsio.Stats()
    served, n_batches = drain(rd, s, 8000)
    assert len(served) > len(set(served)) > 20 and all(r in recs for r in served)
    same(s.groups(), su.accumulate([su.parse(r) for r in served]))
    assert s.counter("records_counted") == len(served)
    s.close()
    rd.close()
