"""GPU tests of the duplicate marker at the C-ABI (include/seqlib_amd_dup.h through seqlib_amd/dupio.py) against the Python statement of the rules in
tests/dup_util.py: batch sizes, the CIGAR and quality edges of the lane and the wave form (every edge record beside probes that are duplicates only when the
GPU's 5' end and score are exactly Python's), pairs and near misses, orphans, fragments, libraries, the knobs that must not change a result, large groups,
apply in place, the refusals, and the route through the sorter.  Equality is exact everywhere."""
import random
import struct

import pytest

from tests import dup_util as du

pytestmark = pytest.mark.gpu

D, N, U = du.DUP, du.NOT_DUP, du.UNTOUCHED


@pytest.fixture(scope="module")
def io(sl):
    import torch
    from seqlib_amd import _ffi, dupio, sortio
    dupio.lib()

    class F:
        pass
    f = F()
    f.ffi, f.dupio, f.sortio, f.torch = _ffi, dupio, sortio, torch
    return f


def run(io, batches, header=None, **knobs):
    m = io.dupio.Marker(header_text=header, **knobs)
    assert m.counter("device") >= 0
    for b in batches:
        m.add_host(*du.stream_of(b))
    m.finish()
    return m, m.flags()


def check(io, batches, header=None, **knobs):
    want, counters = du.mark(batches, header)
    m, got = run(io, batches, header, **knobs)
    assert got == want
    for k, v in counters.items():
        assert m.counter(k) == v, k
    return m, want


def upload(io, stream, off):
    t = io.torch
    d_s = t.frombuffer(bytearray(stream) or bytearray(1), dtype=t.uint8).cuda()
    d_o = t.tensor(off, dtype=t.int64).cuda()
    t.cuda.synchronize()
    return d_s, d_o


def q(v, n=50):
    return bytes([v]) * n


# ---------------------------------------------------------------- batch sizes
@pytest.mark.parametrize("n", [0, 1, 2, 64, 65])
def test_batches_of(io, n):
    rng = random.Random(n)
    recs = [du.record("b%d" % i, 0, 100 + (i % 3), qual=q(rng.choice((20, 30)))) for i in range(n)]
    m, want = check(io, [recs])
    assert len(want) == n and (n < 64 or D in want)
    m.close()


# ---------------------------------------------------------------- the signature's edges
LIB_RG = {1: b"a1", 2: b"b", 3: b"solo", 4: b"a"}


def quals_summing_to(s):
    """quality bytes in 15 .. 254 whose sum is s (0, or 15 and more)"""
    if s == 0:
        return b"\x03"
    k, r = divmod(s, 254)
    if r == 0:
        return bytes([254]) * k
    if r >= 15:
        return bytes([254]) * k + bytes([r])
    return bytes([254]) * (k - 1) + bytes([127, 127 + r])


def probed(edge):
    """every edge record on a contig of its own, twice: after a probe of the same E and score (the probe stays, by the tie rule), and before one (the record
    stays); and a probe one base off, which nothing touches.  A wrong 5' end, strand, library or score on the GPU changes one of these verdicts."""
    out = []
    for i, (label, rec) in enumerate(edge):
        for variant in (0, 1):
            r = bytearray(rec)
            refid = 10 + 2 * i + variant
            if struct.unpack_from("<i", r, 4)[0] >= 0:
                struct.pack_into("<i", r, 4, refid)
            r = bytes(r)
            cls, lib, _, upos, rev, score = du.signature(r, du.HEADER)
            if cls == du.IGNORED:
                out.append(r)
                continue
            aux = du.rg_aux(LIB_RG[lib]) if lib else b""
            same = du.record("probe_%s" % label, refid, upos, [("M", 1)], quals_summing_to(score), 0x10 if rev else 0, aux)
            near = du.record("near_%s" % label, refid, upos + 1, [("M", 1)], quals_summing_to(score), 0x10 if rev else 0, aux)
            assert du.signature(same, du.HEADER)[1:] == (lib, refid, upos, rev, score), label
            out += [r, same, near] if variant else [same, r, near]
    return out


@pytest.fixture(scope="module")
def edge():
    return du.edge_records()


@pytest.fixture(scope="module")
def edge_probed(edge):
    recs = probed(edge)
    return recs, du.mark([recs], du.HEADER)


def test_edge_records_beside_their_probes(io, edge, edge_probed):
    recs, (want, counters) = edge_probed
    assert want.count(D) >= sum(2 for _, r in edge if du.signature(r)[0] != du.IGNORED) and U in want
    m, got = run(io, [recs], du.HEADER)
    assert got == want
    for k, v in counters.items():
        assert m.counter(k) == v, k
    assert m.counter("libraries") == 4 and m.counter("read_groups") == 5
    m.close()


@pytest.mark.parametrize("wave_len", [0, 64, du.WAVE_LEN, 2 ** 20])
def test_wave_len_never_changes_a_result(io, edge_probed, wave_len):
    recs, (want, _) = edge_probed
    m, got = run(io, [recs], du.HEADER, wave_len=wave_len)
    assert got == want
    n_long = 0
    for r in recs:
        n_cig, _, l_seq = struct.unpack_from("<HHi", r, 16)
        n_long += n_cig > 64 or l_seq > wave_len
    assert m.counter("long_records") == n_long and n_long > 0 and (wave_len or n_long > len(recs) // 2)
    m.close()


def test_edge_records_split_over_adds_and_one_by_one(io, edge_probed):
    recs, (want, _) = edge_probed
    cut = [0, 1, 2, 66, 131, len(recs)]
    m, got = run(io, [recs[a:b] for a, b in zip(cut, cut[1:])], du.HEADER)
    assert got == want
    m.close()


# ---------------------------------------------------------------- pairs, orphans, fragments
def pair_cases():
    c = []
    c += du.pair("dup_lo", 0, 100, 300, q(20)) + du.pair("dup_hi", 0, 100, 300, q(30)) + du.pair("dup_tie", 0, 100, 300, q(30))
    c += du.pair("near_base", 0, 100, 301) + du.pair("near_strand", 0, 100, 300, flag1=0x10) + du.pair("near_contig", 1, 100, 300)
    c += du.pair("two_contigs_a", 0, 500, 700, q(20), refid2=2) + du.pair("two_contigs_b", 0, 500, 700, q(25), refid2=2)
    c += list(reversed(du.pair("two_contigs_c", 0, 500, 700, q(22), refid2=2)))          # the second read first
    same_e = [du.record("same_e_%d" % k, 0, 1200, qual=q(30), flag=0x1 | bit) for k in range(2) for bit in (0x40, 0x80)]
    c += same_e          # both ends of a pair with one E, twice: the second pair is a duplicate
    c += du.pair("tie_a", 1, 2000, 2300) + du.pair("tie_b", 1, 2000, 2300) + du.pair("tie_c", 1, 2000, 2300)
    c += [du.pair("missing_mate", 0, 100, 300)[0]]
    c += du.pair("three", 0, 100, 300) + [du.pair("three", 0, 100, 300)[1]]
    c += [du.pair("two_first", 0, 100, 300)[0], du.pair("two_first", 0, 100, 300)[0]]
    c += [du.record("both_bits", 0, 100, flag=0x1 | 0x40 | 0x80), du.record("both_bits", 0, 349, flag=0x1 | 0x80 | 0x10)]
    c += [du.record("frag_beside_pair", 0, 100, qual=q(40)), du.record("frag_beside_orphan", 1, 100, qual=q(40), flag=0x10), du.record("frag_rev_beside_pair", 0, 349, flag=0x10)]
    c += [du.record("alone_%d" % k, 2, 4000, qual=q(v)) for k, v in enumerate((20, 40, 40, 14))]
    c += [du.record("mate_unmapped", 0, 100, flag=0x1 | 0x8 | 0x40), du.record("secondary", 0, 100, flag=0x100 | 0x400), du.record("was_marked", 2, 6000, flag=0x400)]
    return c


def test_pairs_orphans_and_fragments(io):
    recs = pair_cases()
    m, want = check(io, [recs])
    by = {(du.fields(r)["name"].decode(), du.fields(r)["flag"] & 0xc0): v for r, v in zip(recs, want)}
    assert (by["dup_lo", 0x40], by["dup_hi", 0x40], by["dup_tie", 0x80]) == (D, N, D)
    assert [by[n, 0x40] for n in ("near_base", "near_strand", "near_contig")] == [N] * 3
    assert (by["two_contigs_a", 0x80], by["two_contigs_b", 0x40], by["two_contigs_c", 0x40]) == (D, N, D)
    assert (by["tie_a", 0x40], by["tie_b", 0x40], by["tie_c", 0x80]) == (N, D, D)
    assert (by["frag_beside_pair", 0], by["frag_beside_orphan", 0], by["secondary", 0], by["was_marked", 0]) == (D, N, U, N)
    assert m.counter("orphans") == 1 + 3 + 2 and m.counter("hash_runs_mixed") == 0
    m.close()


def test_mates_split_over_three_interleaving_adds(io):
    recs = pair_cases() + du.bulk(600, seed=3)
    firsts, seconds, rest = [], [], []
    for r in recs:
        f = du.fields(r)["flag"]
        (firsts if f & 0x40 else seconds if f & 0x80 else rest).append(r)
    m, want = check(io, [seconds, rest, firsts], du.HEADER)
    assert D in want and m.counter("pairs") > 100
    m.close()


def test_libraries(io):
    at = lambda name, rg, pos=100, **k: du.record(name, 0, pos, aux=du.rg_aux(rg) if rg is not None else b"", **k)
    recs = [at("a1", b"a1"), at("b", b"b"), at("a2", b"a2"), at("solo", b"solo"), at("none", None), du.record("type_a", 0, 100, aux=b"RGAx"),
            at("empty", b""), at("unknown", b"zz"), at("a_prefix", b"a")]
    recs += du.pair("p_a1", 0, 700, 900, aux=du.rg_aux(b"a1")) + du.pair("p_b", 0, 700, 900, aux=du.rg_aux(b"b")) + du.pair("p_a2", 0, 700, 900, aux=du.rg_aux(b"a2"))
    recs += du.pair("split", 0, 1700, 1900, aux=du.rg_aux(b"a1"))[:1] + du.pair("split", 0, 1700, 1900, aux=du.rg_aux(b"b"))[1:]          # one name in two libraries: orphans
    m, want = check(io, [recs], du.HEADER)
    assert want[:9] == [N, N, D, N, N, D, D, D, N]          # a2 follows a1 (one library); type_a, empty and unknown follow none (library 0)
    assert want[9:15] == [N, N, N, N, D, D] and want[15:] == [N, N] and m.counter("orphans") == 2
    m.close()
    m, want0 = check(io, [recs])          # without a header everything is one library
    assert want0[:9] == [N] + [D] * 8 and want0[15:] == [N, N] and m.counter("orphans") == 0
    m.close()


# ---------------------------------------------------------------- knobs
def test_hash_bits_never_change_a_result(io):
    recs = pair_cases() + du.bulk(400, seed=5)
    want, _ = du.mark([recs], du.HEADER)
    mixed = {}
    for bits in (64, 4, 0):
        m, got = run(io, [recs], du.HEADER, hash_bits=bits)
        assert got == want, bits
        mixed[bits] = m.counter("hash_runs_mixed")
        m.close()
    assert mixed[64] == 0 and mixed[4] > 0 and mixed[0] == 1


def test_a_run_past_run_max_is_refused(io):
    recs = du.pair("a", 0, 100, 300) + du.pair("b", 0, 100, 300)
    m = io.dupio.Marker(hash_bits=0, run_max=2)
    m.add_host(*du.stream_of(recs))
    with pytest.raises(io.ffi.SlxError) as e:
        m.finish()
    assert e.value.code == io.ffi.SLX_EUNSUPPORTED and "run_max" in str(e.value)
    m.set("run_max", 4)
    m.finish()
    assert m.flags() == [N, N, D, D]
    m.close()


# ---------------------------------------------------------------- large inputs
def test_one_group_larger_than_any_block(io):
    rng = random.Random(9)
    recs = [du.record("g%d" % i, 0, 777, qual=q(rng.choice((20, 30, 40)), 20), flag=0) for i in range(3000)]
    m, want = check(io, [recs])
    assert want.count(N) == 1 and want.index(N) == next(i for i, r in enumerate(recs) if du.signature(r)[5] == 800)
    m.close()


def test_bulk(io):
    recs = du.bulk(5000)
    m, want = check(io, [recs[:1700], recs[1700:1701], recs[1701:]], du.HEADER)
    assert want.count(D) > 1000 and want.count(U) > 100 and m.counter("pairs") > 500 and m.counter("orphans") > 50
    m.close()


# ---------------------------------------------------------------- apply
def test_apply_changes_bit_0x400_of_eligible_records_only(io):
    recs = pair_cases() + du.bulk(300, seed=2)
    stream, off = du.stream_of(recs)
    m, want = check(io, [recs], du.HEADER)
    expect = b"".join(du.marked(r, v) for r, v in zip(recs, want))
    assert expect != stream
    d_s, d_o = upload(io, stream, off)
    m.apply_device(d_s.data_ptr(), len(stream), d_o.data_ptr(), len(recs))
    got = bytes(d_s.cpu().numpy())
    assert got == expect
    by = {du.fields(r)["name"]: (du.fields(r)["flag"], struct.unpack_from("<H", got, o + 18)[0]) for r, o in zip(recs, off)}
    assert by[b"secondary"] == (0x500, 0x500) and by[b"was_marked"] == (0x400, 0) and by[b"frag_beside_pair"] == (0, 0x400)
    # a tail of the batch at an odd address, and then the whole batch through an ordinal column in another order
    k = 7
    t = io.torch
    d_odd = t.zeros(len(stream) + 3, dtype=t.uint8).cuda()
    d_odd[3:3 + len(stream) - off[k]] = t.frombuffer(bytearray(stream[off[k]:]), dtype=t.uint8).cuda()
    t.cuda.synchronize()
    m.apply_device(d_odd.data_ptr() + 3, len(stream) - off[k], d_o.data_ptr() + 8 * k, len(recs) - k, first_ordinal=k)
    assert bytes(d_odd.cpu().numpy())[3:3 + len(stream) - off[k]] == expect[off[k]:]
    order = list(range(len(recs)))
    random.Random(4).shuffle(order)
    s2, o2 = du.stream_of([recs[i] for i in order])
    d_s2, d_o2 = upload(io, s2, o2)
    d_ord = t.tensor(order, dtype=t.int32).cuda()
    t.cuda.synchronize()
    m.apply_device(d_s2.data_ptr(), len(s2), d_o2.data_ptr(), len(recs), d_ordinals=d_ord.data_ptr())
    assert bytes(d_s2.cpu().numpy()) == b"".join(du.marked(recs[i], want[i]) for i in order)
    m.close()


# ---------------------------------------------------------------- refusals
def test_a_truncated_record_fails_the_add_and_changes_nothing(io):
    from tests.test_dup_host import broken_batches
    b1, b3 = pair_cases()[:20], pair_cases()[20:]
    want, counters = du.mark([b1, b3])
    m = io.dupio.Marker()
    m.add_host(*du.stream_of(b1))
    for label, recs, stream, off, bad in broken_batches():
        with pytest.raises(io.ffi.SlxError) as e:
            m.add_host(stream, off)
        assert e.value.code == io.ffi.SLX_EIO and "record %d of the batch" % bad in str(e.value), label
        assert m.counter("records") == len(b1)
    m.add_host(*du.stream_of(b3))
    m.finish()
    assert m.flags() == want and m.counter("pairs") == counters["pairs"]
    m.close()


def test_max_bytes_apply_before_finish_and_ordinals_out_of_range(io):
    recs = pair_cases()
    stream, off = du.stream_of(recs)
    m = io.dupio.Marker(max_bytes=22 * len(recs))
    with pytest.raises(io.ffi.SlxError) as e:
        m.add_host(stream, off)
    assert e.value.code == io.ffi.SLX_EUNSUPPORTED and "max_bytes" in str(e.value) and m.counter("records") == 0 and m.counter("held_bytes") == 0
    m.set("max_bytes", 1 << 20)
    m.add_host(stream, off)
    d_s, d_o = upload(io, stream, off)
    for call in (lambda: m.apply_device(d_s.data_ptr(), len(stream), d_o.data_ptr(), len(recs)), m.flags):
        with pytest.raises(io.ffi.SlxError) as e:
            call()
        assert e.value.code == io.ffi.SLX_EINVAL
    m.finish()
    with pytest.raises(io.ffi.SlxError) as e:
        m.add_host(stream, off)          # after finish, without clear
    assert e.value.code == io.ffi.SLX_EINVAL
    t = io.torch
    d_ord = t.tensor(list(range(len(recs) - 1)) + [len(recs)], dtype=t.int32).cuda()
    t.cuda.synchronize()
    for kw in (dict(first_ordinal=1), dict(first_ordinal=-1), dict(d_ordinals=d_ord.data_ptr())):
        with pytest.raises(io.ffi.SlxError) as e:
            m.apply_device(d_s.data_ptr(), len(stream), d_o.data_ptr(), len(recs), **kw)
        assert e.value.code == io.ffi.SLX_EINVAL, kw
    assert bytes(d_s.cpu().numpy()) == stream          # nothing was written
    want, _ = du.mark([recs])
    assert m.flags() == want
    m.clear()
    assert m.counter("records") == 0 and m.counter("finished") == 0
    m.add_host(*du.stream_of(recs[:4]))
    m.finish()
    assert m.flags() == du.mark([recs[:4]])[0]
    m.close()


# ---------------------------------------------------------------- the sorter's route
def test_sorter_route(io):
    recs = pair_cases() + du.bulk(500, seed=8)
    random.Random(1).shuffle(recs)
    want, counters = du.mark([recs], du.HEADER)
    s = io.sortio.Sorter()
    for a in range(0, len(recs), 211):
        s.add_host(recs[a:a + 211])
    m = io.dupio.Marker(header_text=du.HEADER)
    m.mark_sorter(s.h)
    assert m.flags() == want and m.counter("duplicates") == counters["duplicates"] > 0
    stream, off, perm = s.to_host()
    order = sorted(range(len(recs)), key=lambda i: (struct.unpack_from("<i", recs[i], 4)[0] & 0xffffffff, struct.unpack_from("<i", recs[i], 8)[0]))
    assert perm == order and stream == b"".join(du.marked(recs[i], want[i]) for i in order)
    with pytest.raises(io.ffi.SlxError) as e:
        m.mark_sorter(s.h)          # the marker is not empty
    assert e.value.code == io.ffi.SLX_EINVAL
    m.close()
    s.close()
