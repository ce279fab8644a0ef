"""GPU tests of the assembly-window collector at the C-ABI (include/seqlib_amd_win.h through seqlib_amd/winio.py) and of slx_fml_stage_device, against the
Python statement of the rules in tests/win_util.py: batch sizes, the read lengths at the nibble, store, ballot, knob and tile edges (in one batch, and first and
last of a tile), the window shapes, three interleaving adds, a real reader with and without regions, trim, strand and skip flags, the knob that must not change
a result, the arena bound, a broken record, and the whole route to contigs.  Equality is exact everywhere."""
import random
import struct

import numpy as np
import pytest

from tests import bam_util as bu
from tests import fml_util as fu
from tests import ref_util as ru
from tests import win_util as wu

pytestmark = pytest.mark.gpu

TILE = 2048
ONE = [(0, 0, 10 ** 6)]


@pytest.fixture(scope="module")
def io(sl):
    import torch
    from seqlib_amd import _ffi, bamio, fml, winio
    winio.lib()

    class F:
        pass
    f = F()
    f.ffi, f.bamio, f.fml, f.winio, f.torch = _ffi, bamio, fml, winio, torch
    return f


@pytest.fixture(scope="module")
def edge():
    return wu.edge_records()


def result(c):
    """finish, then the download and the view's scalars against each other -> (bases, quals, offs, win_off, rec_of_read)"""
    c.finish()
    v = c.view()
    got = c.download()
    lens = [b - a for a, b in zip(got[2], got[2][1:])]
    assert (v.n_reads, v.total, v.max_len) == (len(got[4]), len(got[0]), max(lens, default=0)) and len(got[1]) == v.total and got[3][-1] == v.n_reads
    return got


def check(io, windows, batches, rules=None, **knobs):
    rules = rules or wu.Rules()
    want = wu.collect(windows, batches, rules)
    c = io.winio.Collector(windows, skip_flags=rules.skip_flags, qual_trim=rules.qual_trim, original_strand=rules.original_strand, **knobs)
    assert c.counter("device") >= 0
    for recs in batches:
        c.add_host(*ru.stream_of(recs))
    got = result(c)
    assert got == want[:5]
    st = want[5]
    assert (c.counter("records"), c.counter("reads")) == (len(st), len(want[4]))
    assert [c.counter(k) for k in ("drop_flags", "drop_no_seq", "drop_no_name", "drop_trimmed")] == [st.count(s) for s in (wu.SKIP_FLAG, wu.NO_SEQ, wu.NO_NAME, wu.TRIMMED)]
    c.close()
    return want


@pytest.mark.parametrize("n", [0, 1, 64, 65])
def test_batches_of(io, n):
    rng = np.random.default_rng(n)
    recs = [wu.record("b%d" % i, 0, 100 + i, wu.rand_seq(random.Random(i), int(rng.integers(1, 200)))) for i in range(n)]
    want = check(io, ONE, [recs])
    assert len(want[4]) == n


@pytest.mark.parametrize("strand", [0, 1])
@pytest.mark.parametrize("trim", [-1, 0, 4, 93])
def test_edge_lengths_in_one_batch(io, edge, trim, strand):
    want = check(io, ONE, [edge], wu.Rules(qual_trim=trim, original_strand=strand))
    if trim <= 0:
        assert [b - a for a, b in zip(want[2], want[2][1:])] == list(wu.EDGE_LENGTHS)
    if trim == 93:
        assert wu.TRIMMED in want[5] and wu.KEEP in want[5] and sum(b - a for a, b in zip(want[2], want[2][1:])) < sum(wu.EDGE_LENGTHS)


def test_everything_trimmed_away_is_a_valid_empty_result(io):
    recs = [wu.record("q%d" % i, 0, 100, "ACGT" * 20, bytes([10]) * 80, flag=0x10 * (i & 1)) for i in range(5)]
    want = check(io, ONE + [(0, 50, 150)], [recs], wu.Rules(qual_trim=93, original_strand=1))
    assert want[:5] == (b"", b"", [0], [0, 0, 0], []) and want[5] == [wu.TRIMMED] * 5


def test_edge_lengths_first_and_last_of_a_tile(io):
    """every edge length as the read that starts a tile of the output and as the one that ends one, odd and even, on both strands"""
    rng = random.Random(3)
    c = io.winio.Collector(ONE, original_strand=1)
    rules = wu.Rules(original_strand=1)
    for k, n in enumerate(wu.EDGE_LENGTHS):
        fill = (-(TILE + n) - n) % TILE or TILE
        lens = [TILE, n, fill, n, 100]
        recs = [wu.record("t%d" % j, 0, 100 + j, wu.rand_seq(rng, ln, wu.SEQ_CODES), bytes(rng.randrange(94) for _ in range(ln)), flag=0x10 if (j + k) & 1 else 0) for j, ln in enumerate(lens)]
        want = wu.collect(ONE, [recs], rules)
        assert want[2][1] % TILE == 0 and want[2][4] % TILE == 0
        c.clear()
        c.add_host(*ru.stream_of(recs))
        assert result(c) == want[:5], n
    c.close()


SHAPES = [(0, 3000, 3999), (0, 1000, 1999), (0, 1500, 2499), (0, 1800, 2999), (1, 0, 100), (0, 500, 900), (0, 9000, 9999)]          # unsorted; empty first, in the middle and last


def shape_records():
    r = lambda name, tid, pos, n=100, flag=0: wu.record(name, tid, pos, "ACGT" * (n // 4), bytes([30]) * n, flag=flag)
    return [r("only5", 0, 450, 100), r("last_base", 0, 900, 20, flag=4), r("one_past", 0, 901, 20, flag=4), r("one_before", 0, 898, 20, flag=4), r("in_one", 0, 1000), r("in_two", 0, 1600),
            r("in_three", 0, 1850), r("other_tid", 2, 1850), r("no_window", 0, 5000)]


def test_window_shapes(io):
    recs = shape_records()
    want = check(io, SHAPES, [recs])
    per = [want[4][a:b] for a, b in zip(want[3], want[3][1:])]
    assert per == [[], [4, 5, 6], [5, 6], [6], [], [0, 1, 3], []]          # (898, 899) and (900, 901) touch [500, 900]; (901, 902) does not
    check(io, SHAPES[1:2], [recs])          # one window
    check(io, [], [recs])                   # none


def three_adds():
    rng = random.Random(9)
    wins = [(0, 2000, 2999), (0, 0, 999), (0, 500, 2499), (1, 0, 5000)]
    recs = [wu.record("a%d" % i, rng.choice((0, 0, 0, 1)), rng.randrange(0, 3000), wu.rand_seq(rng, rng.randrange(1, 300)),
                      flag=rng.choice((0, 0x10))) for i in range(130)]
    return wins, recs


def test_three_adds_follow_the_ordinal(io):
    wins, recs = three_adds()
    split = check(io, wins, [recs[:65], recs[65:66], recs[66:]], wu.Rules(original_strand=1))
    whole = check(io, wins, [recs], wu.Rules(original_strand=1))
    assert split == whole and all(b > a for a, b in zip(split[3], split[3][1:]))
    for a, b in zip(split[3], split[3][1:]):
        assert split[4][a:b] == sorted(split[4][a:b])
    assert len(set(split[4])) < len(split[4])          # a record in several windows is a read of each


def test_a_device_batch_and_clear(io, edge):
    t = io.torch
    stream, off = ru.stream_of(edge)
    d_s = t.frombuffer(bytearray(stream), dtype=t.uint8).cuda()
    d_o = t.tensor(off, dtype=t.int64).cuda()
    t.cuda.synchronize()          # (torch copies on its own stream, the collector reads on its own)
    c = io.winio.Collector(ONE)
    c.add_device(d_s.data_ptr(), len(stream), d_o.data_ptr(), len(edge))
    d_s.zero_()                   # the batch's memory is recycled: the collector has its own copy
    t.cuda.synchronize()
    want = wu.collect(ONE, [edge])
    assert result(c) == want[:5]
    c.add_host(*ru.stream_of(edge[:2]))
    with pytest.raises(io.ffi.SlxError) as e:          # after an add the old result is gone until the next finish
        c.view()
    assert e.value.code == io.ffi.SLX_EINVAL
    assert result(c) == wu.collect(ONE, [edge, edge[:2]])[:5]
    c.clear()
    assert (c.counter("records"), c.counter("reads"), c.counter("arena_bytes_used")) == (0, 0, 0)
    c.add_host(*ru.stream_of(edge[3:9]))
    assert result(c) == wu.collect(ONE, [edge[3:9]])[:5]
    c.close()


def test_the_tail_of_a_batch(io, edge):
    """the offsets count from the first entry given: a reader's batch that Next() has begun to serve is its stream pointer moved up and its table from there on"""
    t = io.torch
    stream, off = ru.stream_of(edge)
    d_s = t.frombuffer(bytearray(stream), dtype=t.uint8).cuda()
    d_o = t.tensor(off, dtype=t.int64).cuda()
    t.cuda.synchronize()
    c = io.winio.Collector(SHAPES, original_strand=1)
    for k in (1, 5, len(edge) - 1):
        c.clear()
        c.add_device(d_s.data_ptr() + off[k], len(stream) - off[k], d_o.data_ptr() + 8 * k, len(edge) - k)
        assert result(c) == wu.collect(SHAPES, [edge[k:]], wu.Rules(original_strand=1))[:5], k
    with pytest.raises(io.ffi.SlxError) as e:          # the table moved up and the stream not: record 0 does not start at the stream's first byte... its extent is wrong
        c.add_device(d_s.data_ptr(), len(stream), d_o.data_ptr() + 8, len(edge) - 1)
    assert e.value.code == io.ffi.SLX_EIO
    c.close()


def test_skip_flags(io):
    recs = [wu.record("f%x" % f, 0, 100, "ACGTAC", bytes(6), flag=f) for f in (0, 0x1, 0x4, 0x10, 0x100, 0x400, 0x800, 0x900, 0x410)] + [wu.record("", 0, 100, "ACGT", bytes(4)), wu.record("e", 0, 100, "")]
    for skip in (0, 0x900, 0x400, 0xf04):
        want = check(io, ONE, [recs], wu.Rules(skip_flags=skip))
        assert want[5].count(wu.NO_NAME) == 1 and want[5].count(wu.NO_SEQ) == 1 and want[5].count(wu.SKIP_FLAG) == sum(1 for f in (0, 0x1, 0x4, 0x10, 0x100, 0x400, 0x800, 0x900, 0x410) if f & skip)


@pytest.mark.parametrize("strand", [0, 1])
def test_wave_len_changes_nothing(io, edge, strand):
    rng = random.Random(5)
    recs = list(edge)
    for n in (511, 512, 513, 2049):          # the first and the last base at or above the threshold anywhere in a ballot
        for at in ((0,), (63, 64), (n - 1,), (64, n - 65), ()):
            q = bytearray([3] * n)
            for a in at:
                q[a] = 40
            recs.append(wu.record("w%d" % len(recs), 0, 100, wu.rand_seq(rng, n), bytes(q), flag=0x10 if len(recs) & 1 else 0))
    rules = wu.Rules(qual_trim=4, original_strand=strand)
    want = wu.collect(ONE, [recs], rules)
    assert want[5].count(wu.TRIMMED) >= 4
    n_long = []
    for wave_len in (0, 512, 2 ** 20):
        c = io.winio.Collector(ONE, qual_trim=4, original_strand=strand, wave_len=wave_len)
        c.add_host(*ru.stream_of(recs))
        assert result(c) == want[:5], wave_len
        assert c.counter("drop_trimmed") == want[5].count(wu.TRIMMED)
        n_long.append(c.counter("long_reads"))
        c.close()
    assert n_long[0] == len(recs) and 0 < n_long[1] < len(recs) and n_long[2] == 0


def test_arena_bound_refuses_and_the_collector_goes_on(io, edge):
    c = io.winio.Collector(ONE, arena_bytes=4096)
    c.add_host(*ru.stream_of(edge[:4]))
    with pytest.raises(io.ffi.SlxError) as e:
        c.add_host(*ru.stream_of(edge))          # 2 x 12 KiB and more
    need = 2 * sum((n + 15) // 16 * 16 for n in wu.EDGE_LENGTHS) + c.counter("arena_bytes_used")
    assert e.value.code == io.ffi.SLX_EUNSUPPORTED and str(need) in str(e.value) and "4096" in str(e.value)
    assert (c.counter("records"), c.counter("reads")) == (4, 4)
    c.add_host(*ru.stream_of(edge[4:8]))
    assert result(c) == wu.collect(ONE, [edge[:4], edge[4:8]])[:5]
    c.close()


def test_a_broken_record_fails_the_add_and_changes_nothing(io, edge):
    good = wu.record("good", 0, 100, "ACGTACGTAC", bytes(range(10)))
    past = bytearray(good)
    struct.pack_into("<i", past, 20, 10 ** 6)
    no_nul = bytearray(good)
    no_nul[36 + good[12] - 1] = ord("x")
    c = io.winio.Collector(ONE, qual_trim=4)
    c.add_host(*ru.stream_of(edge[:5]))
    before = [c.counter(k) for k in io.winio.COUNTERS if not k.startswith("us_")]
    for bad in (bytes(past), bytes(no_nul)):
        recs = edge[5:9] + [bad] + edge[9:12] + [bad]
        stream, off = ru.stream_of(recs)
        assert wu.first_bad(stream, off) == 4
        with pytest.raises(io.ffi.SlxError) as e:
            c.add_host(stream, off)
        assert e.value.code == io.ffi.SLX_EIO and "record 4 of the batch" in str(e.value)
        assert [c.counter(k) for k in io.winio.COUNTERS if not k.startswith("us_")] == before
    stream, off = ru.stream_of(edge[5:9])
    off[2] += 4                     # an offset table that disagrees with the block sizes
    with pytest.raises(io.ffi.SlxError) as e:
        c.add_host(stream, off)
    assert e.value.code == io.ffi.SLX_EIO and "record %d of the batch" % wu.first_bad(stream, off) in str(e.value)
    c.add_host(*ru.stream_of(edge[5:9]))
    assert result(c) == wu.collect(ONE, [edge[:5], edge[5:9]], wu.Rules(qual_trim=4))[:5]
    c.close()


# ---------------------------------------------------------------- a real reader
def drain(rd, c, max_bytes):
    served, n_batches = [], 0
    while True:
        recs, b = rd.next(max_bytes)
        if not recs:
            return served, n_batches
        c.add_device(b.d_stream, b.n_bytes, b.d_rec_off, b.n_records)
        served.append(recs)
        n_batches += 1


def test_through_the_bam_reader(io, tmp_path):
    key = lambda r: (struct.unpack_from("<i", r, 4)[0] & 0xffffffff, struct.unpack_from("<i", r, 8)[0])
    recs = sorted((r for r in bu.sample_records(400) if struct.unpack_from("<i", r, 8)[0] >= 0 or struct.unpack_from("<i", r, 4)[0] < 0), key=key)
    wins = [(0, 0, 60000), (0, 50000, 120000), (1, 0, 10 ** 6), (2, 1000, 2000)]
    p = tmp_path / "sorted.bam"
    p.write_bytes(bu.bam_bytes(bu.TEXT, bu.REFS, recs, member_size=4000))
    io.bamio.index_build(p)
    rd = io.bamio.Reader(p)
    c = io.winio.Collector(wins, original_strand=1)
    served, n_batches = drain(rd, c, 8000)
    assert [r for b in served for r in b] == recs and n_batches >= 3
    want = wu.collect(wins, served, wu.Rules(original_strand=1))
    assert result(c) == want[:5] and len(want[4]) > 100
    # two regions that overlap: a record served twice is two records, with two ordinals
    rd.index_load()
    rd.set_regions([(0, 20000, 120000), (0, 40000, 160000)])
    c.clear()
    served, n_batches = drain(rd, c, 8000)
    flat = [r for b in served for r in b]
    assert len(flat) - len(set(flat)) >= 20
    want = wu.collect(wins, served, wu.Rules(original_strand=1))
    assert result(c) == want[:5] and c.counter("records") == len(flat)
    rd.close()
    c.close()


# ---------------------------------------------------------------- slx_fml_stage_device
def _same_utgs(got, exp, tag):
    assert len(got) == len(exp), "%s: %d unitigs, expected %d" % (tag, len(got), len(exp))
    for i, (a, b) in enumerate(zip(got, exp)):
        for k in ("len", "nsr", "seq", "cov", "n_ovlp", "ovlp"):
            assert a[k] == b[k], "%s: unitig %d differs in %s" % (tag, i, k)


@pytest.fixture(scope="module")
def ctx(io):
    c = io.fml.Context()
    yield c
    c.close()


@pytest.fixture(scope="module")
def myc():
    return fu.fixture_genome()["myc"]


def _dev(io, arr):
    t = io.torch
    d = t.from_numpy(np.ascontiguousarray(arr).view(np.uint8).copy()).cuda() if arr.size else t.zeros(16, dtype=t.uint8).cuda()
    t.cuda.synchronize()
    return d


@pytest.mark.parametrize("with_quals", [True, False])
@pytest.mark.parametrize("n", [0, 1, 64, 65])
def test_stage_device_equals_the_host_arrays(io, ctx, myc, n, with_quals):
    seqs, quals, _ = fu.sim_window(myc[1000:1600], n, seed=20 + n)
    b, q, o = io.fml.flatten(seqs, quals if with_quals else None)
    opt = io.fml.default_opt()
    want = ctx.assemble(opt, b, q, o, [0, n])
    db, dq, do = _dev(io, b), (_dev(io, q) if with_quals else None), _dev(io, o)
    ctx.stage_device(db.data_ptr() if n else None, dq.data_ptr() if with_quals and n else None, do.data_ptr(), n)
    for _ in range(2):          # every call starts from the reads as staged
        _same_utgs(ctx.assemble_staged(opt, [0, n])[0], want[0], "n = %d" % n)
    if n == 65:
        assert len(want[0]) >= 1


def test_stage_device_refusals(io, ctx):
    t = io.torch
    for lens, code in (([10, 32001, 10], io.ffi.SLX_EUNSUPPORTED), ([10, 32000, 10], 0)):
        o = np.cumsum([0] + lens).astype(np.uint64)
        db, do = _dev(io, np.full(int(o[-1]), ord("A"), np.uint8)), _dev(io, o)
        if code:
            with pytest.raises(io.ffi.SlxError) as e:
                ctx.stage_device(db.data_ptr(), None, do.data_ptr(), len(lens))
            assert e.value.code == code and "32001" in str(e.value)
        else:
            ctx.stage_device(db.data_ptr(), None, do.data_ptr(), len(lens))
    o = np.array([0, 100, 90, 200], np.uint64)          # decreasing offsets
    db, do = _dev(io, np.full(200, ord("A"), np.uint8)), _dev(io, o)
    with pytest.raises(io.ffi.SlxError) as e:
        ctx.stage_device(db.data_ptr(), None, do.data_ptr(), 3)
    assert e.value.code == io.ffi.SLX_EINVAL and "read 1" in str(e.value)
    with pytest.raises(io.ffi.SlxError) as e:          # no staged reads are left behind a refusal
        ctx.assemble_staged(io.fml.default_opt(), [0, 3])
    assert e.value.code == io.ffi.SLX_EINVAL
    host = np.zeros(64, np.uint8)
    with pytest.raises(io.ffi.SlxError) as e:          # a host pointer is no memory of the context's device
        ctx.stage_device(host.ctypes.data, None, do.data_ptr(), 3)
    assert e.value.code == io.ffi.SLX_EINVAL
    if t.cuda.device_count() > 1:
        other = t.zeros(256, dtype=t.uint8, device="cuda:1")
        with pytest.raises(io.ffi.SlxError) as e:
            ctx.stage_device(other.data_ptr(), None, do.data_ptr(), 3)
        assert e.value.code == io.ffi.SLX_EINVAL


# ---------------------------------------------------------------- end to end
def test_records_to_contigs(io, ctx, myc):
    """reads simulated with known positions, written as BAM records with their CIGAR at their position: collector -> stage_device -> assemble_staged gives per
    window exactly the contigs of slx_fml_assemble over the host loop's reads"""
    recs = wu.e2e_records(myc)
    want = wu.collect(wu.E2E_WINDOWS, [recs])
    opt = io.fml.default_opt()
    n_reads = len(want[4])
    exp = ctx.assemble(opt, np.frombuffer(want[0], np.uint8).copy(), np.frombuffer(want[1], np.uint8).copy(), np.array(want[2], np.uint64), want[3])
    assert len(exp[0]) >= 1 and len(exp[1]) >= 1 and want[3][3] - want[3][2] == 3          # (checked with the CPU oracle when the seed was fixed: one contig of 4.1 kb each)
    c = io.winio.Collector(wu.E2E_WINDOWS)
    for k in range(0, len(recs), 300):
        c.add_host(*ru.stream_of(recs[k:k + 300]))
    assert result(c) == want[:5]
    v = c.view()
    ctx.stage_device(v.d_bases, v.d_quals, v.d_offs, v.n_reads)
    got = ctx.assemble_staged(opt, want[3])
    assert v.n_reads == n_reads and len(got) == 3
    for w in range(3):
        _same_utgs(got[w], exp[w], "window %d" % w)
    c.close()
