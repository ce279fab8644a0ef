"""GPU tests of the reference genome at the C-ABI (include/seqlib_amd_ref.h through seqlib_amd/refio.py) against the Python statement of the rules in
tests/ref_util.py and the recorded samtools index of tiny.fa: the load from the three sources, every FASTA case and every failing one, a stale index, the knobs
that must not change a result, contig lengths around the tile edges, the fetch and its clipping, fetched windows aligned without leaving HBM, NM and MD over the
record cases and generated records in the three splits between lanes and waves, and NM against the aligner's own.  Equality is exact everywhere.  The C++ class is
driven in tests/test_cpp_ref.py."""
import gzip
import os
import random
import struct

import pytest

from tests import bam_util as bu
from tests import ref_util as ru

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")
TINY = os.path.join(GOLDEN, "tiny.fa")


@pytest.fixture(scope="module")
def io(sl):
    from seqlib_amd import _ffi, recio, refio
    refio.lib()

    class F:
        pass
    f = F()
    f.ffi, f.recio, f.refio = _ffi, recio, refio
    return f


@pytest.fixture(scope="module")
def tiny():
    text = open(TINY, "rb").read()
    return text, ru.contigs_of(text), open(TINY + ".fai", "rb").read()


@pytest.fixture(scope="module")
def tiny_ref(io):
    r = io.refio.Ref(TINY)
    yield r
    r.close()


@pytest.fixture(scope="module")
def bulk():
    contigs = ru.bulk_contigs()
    recs = [r for _, r in ru.REC_CASES if ru.parse(r)["tid"] < 0] + ru.bulk_records(contigs)
    return contigs, recs, [ru.nm_md(r, contigs) for r in recs]


@pytest.fixture
def bulk_ref(io, bulk, tmp_path_factory):
    p = tmp_path_factory.mktemp("bulkref") / "bulk.fa"
    p.write_bytes(ru.fasta([(b"c%d" % i, c) for i, c in enumerate(bulk[0])], 70))
    r = io.refio.Ref(p)
    yield r
    r.close()


def same_as_python(r, text):
    want = ru.contigs_of(text)
    assert r.fai_text() == ru.fai_text(text)
    assert r.nseq() == len(want) and [r.name(i) for i in range(r.nseq())] == [c[0] for c in want] and [r.length(i) for i in range(r.nseq())] == [c[1] for c in want]
    got, offs = r.fetch_host([(i, 0, c[1]) for i, c in enumerate(want)])
    assert offs == ru.fetch(want, [(i, 0, c[1]) for i, c in enumerate(want)])[1] and got == b"".join(c[5] for c in want)
    assert r.counter("contigs") == len(want) and r.counter("bases") == sum(c[1] for c in want) and r.counter("text_bytes") == len(text)
    assert all(r.tid(c[0]) == i for i, c in enumerate(want)) and r.tid(b"no such contig") == -1 and r.name(len(want)) is None and r.length(-1) == -1


# ---------------------------------------------------------------- the load
@pytest.mark.parametrize("source", ["plain", "bgzf", "gzip"])
def test_tiny_from_the_three_sources(io, tiny, tmp_path, source):
    text, want, fai = tiny
    p = tmp_path / ("tiny.fa" + {"plain": "", "bgzf": ".bgz", "gzip": ".gz"}[source])
    p.write_bytes({"plain": lambda: text, "bgzf": lambda: bu.bgzf_bytes(text), "gzip": lambda: gzip.compress(text)}[source]())
    r = io.refio.Ref(p)
    assert r.fai_text() == fai
    same_as_python(r, text)
    assert r.counter("source") == ["plain", "bgzf", "gzip"].index(source) and r.counter("windows") >= 1 and r.counter("us_class") > 0 and r.counter("us_gather") > 0
    d = r.device()
    assert d.n_contigs == 4 and d.n_bytes == sum((c[1] + 15) // 16 * 16 for c in want) == r.counter("hbm_bytes") and d.d_bases and d.d_contig_off and d.d_contig_len
    r.close()


@pytest.mark.parametrize("name", sorted(ru.GOOD))
def test_fasta_case(io, tmp_path, name):
    p = tmp_path / "case.fa"
    p.write_bytes(ru.GOOD[name])
    for window in (0, 64):
        r = io.refio.Ref(p, window_bytes=window)
        same_as_python(r, ru.GOOD[name])
        r.close()


@pytest.mark.parametrize("name", sorted(ru.BAD))
def test_failing_fasta_case(io, tmp_path, name):
    p = tmp_path / "case.fa"
    p.write_bytes(ru.BAD[name][0])
    for window in (0, 64):
        with pytest.raises(io.ffi.SlxError) as e:
            io.refio.Ref(p, window_bytes=window)
        assert e.value.code == io.ffi.SLX_EIO and ru.bad_message(name) in str(e.value), str(e.value)


def test_an_error_behind_many_windows_names_its_contig_and_byte(io, tmp_path):
    rng = random.Random(5)
    good = ru.fasta([(b"first", ru.rand_bases(rng, 700)), (b"second desc", ru.rand_bases(rng, 480))], 60)
    for tail, what, contig in ((b">third\nACGT\nAC\nACGT\n", "ragged", "third"), (b">first again\nACGT\n", "name_twice", "first"), (b"AC GT\n", "byte", "second")):
        byte = len(good) + (12 if what == "ragged" else 0)
        p = tmp_path / ("late_%s.fa" % what)
        p.write_bytes(good + tail)
        for window in (0, 64, 257):
            with pytest.raises(io.ffi.SlxError) as e:
                io.refio.Ref(p, window_bytes=window)
            assert e.value.code == io.ffi.SLX_EIO and "%s (contig '%s', byte %d)" % (ru.WHAT[what], contig, byte) in str(e.value), str(e.value)


def test_a_stale_index_fails_the_open(io, tiny, tmp_path):
    text, want, fai = tiny
    p = tmp_path / "tiny.fa"
    p.write_bytes(text)
    r = io.refio.Ref(p)
    assert not os.path.exists(str(p) + ".fai")          # nothing is written unless asked
    r.write_fai()
    assert open(str(p) + ".fai", "rb").read() == fai
    r.write_fai(tmp_path / "elsewhere.fai")
    assert (tmp_path / "elsewhere.fai").read_bytes() == fai
    r.close()
    io.refio.Ref(p).close()          # an index that is right is accepted
    (tmp_path / "tiny.fa.fai").write_bytes(fai.replace(b"141530", b"141531", 1))
    with pytest.raises(io.ffi.SlxError) as e:
        io.refio.Ref(p)
    assert e.value.code == io.ffi.SLX_EIO and "stale index" in str(e.value)
    with pytest.raises(io.ffi.SlxError) as e:
        io.refio.Ref(tmp_path / "missing.fa")
    assert e.value.code == io.ffi.SLX_EIO


# ---------------------------------------------------------------- knobs, tile edges
@pytest.mark.parametrize("knobs", [dict(window_bytes=64), dict(window_bytes=257), dict(tile_bytes=16), dict(gather_tile_bytes=16), dict(gather_tile_bytes=4096),
                                   dict(window_bytes=64, tile_bytes=16, gather_tile_bytes=16)], ids=lambda k: "-".join("%s=%d" % x for x in k.items()))
def test_knobs_never_change_a_result(io, tmp_path, knobs):
    rng = random.Random(9)
    text = ru.fasta([(b"alpha some words that make the header line longer than one window of sixty-four bytes", ru.rand_bases(rng, 1000, b"ACGTacgtN")), (b"nothing", b""),
                     (b"beta", ru.rand_bases(rng, 61)), (b"gamma\tx", ru.rand_bases(rng, 3333))], 60) + b"\n\n"
    p = tmp_path / "k.fa"
    p.write_bytes(text)
    r = io.refio.Ref(p, **knobs)
    same_as_python(r, text)
    if "window_bytes" in knobs:
        assert r.counter("windows") > len(text) // (4 * knobs["window_bytes"])
    r.close()
    for source, raw in (("bgz", bu.bgzf_bytes(text, member_size=300)), ("gz", gzip.compress(text))):
        q = tmp_path / ("k.fa." + source)
        q.write_bytes(raw)
        r = io.refio.Ref(q, **knobs)
        same_as_python(r, text)
        r.close()


@pytest.mark.parametrize("width", [1, 7, 60, 61])
def test_tile_edges(io, tmp_path, width):
    for length in (1, 15, 16, 17, 2047, 2048, 2049):
        text = ru.edge_fasta(length, width)
        p = tmp_path / ("e%d.fa" % length)
        p.write_bytes(text)
        for knobs in (dict(), dict(window_bytes=257, gather_tile_bytes=16)):
            r = io.refio.Ref(p, **knobs)
            same_as_python(r, text)
            assert r.length(1) == length
            r.close()


def test_open_ex_ranges(io):
    for bad in (dict(window_bytes=63), dict(tile_bytes=24), dict(gather_tile_bytes=4112), dict(gather_tile_bytes=8)):
        with pytest.raises(io.ffi.SlxError) as e:
            io.refio.Ref(TINY, **bad)
        assert e.value.code == io.ffi.SLX_EINVAL


# ---------------------------------------------------------------- the fetch
def regions_of(contigs):
    rng = random.Random(21)
    lens = [c[1] for c in contigs]
    R = [(0, 0, 1), (0, lens[0] - 1, lens[0]), (3, 0, lens[3]), (1, -50, 20), (2, -10, -1), (2, lens[2] - 5, lens[2] + 500), (1, lens[1], lens[1] + 10), (0, 100, 100), (0, 200, 100),
         (3, -5, lens[3] + 5), (1, 7, 7 + 2048), (1, 13, 13 + 2049), (2, 1, 1 + 2047), (0, 3, 3 + 4096), (0, 5, 5 + 4097)]
    for n in (15, 16, 17, 31, 32, 33):
        R += [(rng.randrange(4), s, s + n) for s in (rng.randrange(1, 5000) for _ in range(8))]
    while len(R) < 300:
        t = rng.randrange(4)
        b = rng.randrange(-20, lens[t] + 20)
        R.append((t, b, b + rng.choice((1, 2, 5, 40, 100, 150, 700, 2048))))
    return R


@pytest.mark.parametrize("upper", [0, 1])
def test_fetch_equals_slices(io, tiny, tiny_ref, upper):
    text, contigs, _ = tiny
    R = regions_of(contigs)
    want = ru.fetch(contigs, R, upper)
    assert len(R) == 300 and sum(want[1][i + 1] == want[1][i] for i in range(300)) >= 4
    for tile in (2048, 16, 4096):
        tiny_ref.set("gather_tile_bytes", tile)
        assert tiny_ref.fetch_host(R, upper) == want
    tiny_ref.set("gather_tile_bytes", 2048)
    assert tiny_ref.fetch_host([], upper) == (b"", [0]) and tiny_ref.fetch_host([(2, 5, 5)], upper) == (b"", [0, 0])
    assert tiny_ref.counter("us_fetch") >= 0


def test_fetch_folds_lower_case(io, tmp_path):
    text = ru.GOOD["lower_and_iupac"]
    p = tmp_path / "lower.fa"
    p.write_bytes(text)
    r = io.refio.Ref(p)
    seq = ru.contigs_of(text)[0][5]
    assert r.fetch_host([(0, 0, 200), (0, 3, 9)], 0)[0] == seq + seq[3:9] and r.fetch_host([(0, 0, 200), (0, 3, 9)], 1)[0] == seq.upper() + seq[3:9].upper() != seq + seq[3:9]
    r.close()


def test_fetch_refuses_a_tid_out_of_range(io, tiny_ref):
    for bad in ([(4, 0, 10)], [(0, 0, 10), (-1, 0, 10)]):
        with pytest.raises(io.ffi.SlxError) as e:
            tiny_ref.fetch_host(bad)
        assert e.value.code == io.ffi.SLX_EINVAL
    with pytest.raises(io.ffi.SlxError) as e:
        tiny_ref.set("no such knob", 1)
    assert e.value.code == io.ffi.SLX_EINVAL and tiny_ref.counter("nonsense") == -1


def records_of_builder(rb, b):
    stream, off = rb.to_host(b)
    return [stream[off[i]:off[i + 1]] for i in range(b.n_records)]


def test_fetched_windows_align_in_hbm(io, sl, tiny, tiny_ref, tiny_gpu):
    """windows cut from tiny.fa go from the fetch straight into slx_align_batch_device and come back to their own coordinates as one full-length match"""
    text, contigs, _ = tiny
    rng = random.Random(4)
    R = []
    for k in range(120):
        t = rng.randrange(4)
        b = rng.randrange(0, contigs[t][1] - 160)
        R.append((t, b, b + 150))
    d_bases, d_offs, n_bytes = tiny_ref.fetch_device(R, upper=1)
    assert n_bytes == 150 * len(R)
    al = sl.BWAAligner(tiny_gpu)
    rb = io.recio.Builder(al._handle())
    _, _, d_names, d_name_offs = rb.upload([b"A"] * len(R), [b"w%d" % k for k in range(len(R))])
    hits = al.align_device(d_bases, d_offs, len(R), 0, False, 0.9, 10)
    recs = records_of_builder(rb, rb.build(hits, d_bases, d_offs, d_names, d_name_offs, False))
    best = {}
    for r in recs:
        name = r[36:36 + r[12] - 1]
        if not ru.parse(r)["flag"] & 0x900 and name not in best:
            best[name] = ru.parse(r)
    upper = [c[5].upper() for c in contigs]
    n_back = n_unique = 0
    for k, (t, b, e) in enumerate(R):
        p, w = best[b"w%d" % k], upper[t][b:e]
        assert p["cig"] == [(0, 150)], (k, p["cig"])
        if p["flag"] & 16:
            w = bu.revcomp(w.decode()).encode()
        assert upper[p["tid"]][p["pos"]:p["pos"] + 150] == w          # one full-length match on these very bytes
        # a window whose bytes occur once, on one strand, can only come back to its own coordinates
        unique = sum(u.count(upper[t][b:e]) + u.count(bu.revcomp(upper[t][b:e].decode()).encode()) for u in upper) == 1
        n_unique += unique
        n_back += (p["tid"], p["pos"], p["flag"] & 16) == (t, b, 0)
        assert not unique or (p["tid"], p["pos"], p["flag"] & 16) == (t, b, 0), (k, t, b, p["tid"], p["pos"], p["flag"])
    assert n_unique >= 100 and n_back >= n_unique
    rb.close()


# ---------------------------------------------------------------- NM and MD
@pytest.mark.parametrize("long_record", [1, None, 1 << 30], ids=["all_waves", "default", "all_lanes"])
def test_record_cases(io, tmp_path_factory, long_record):
    p = tmp_path_factory.mktemp("reccases") / "cases.fa"
    p.write_bytes(ru.fasta([(b"A", ru.REC_CONTIGS[0]), (b"B", ru.REC_CONTIGS[1]), (b"S", ru.REC_CONTIGS[2])], 25))
    r = io.refio.Ref(p)
    if long_record:
        r.set("long_record", long_record)
    recs = [x for _, x in ru.REC_CASES]
    want = [ru.nm_md(x, ru.REC_CONTIGS) for x in recs]
    got = r.nm_md_host(*ru.stream_of(recs))
    for (name, _), g_nm, g_md, w in zip(ru.REC_CASES, got[0], got[1], want):
        assert (g_nm, g_md) == w, name
    if long_record == 1:
        assert r.counter("long_records") == sum(nm >= 0 for nm, _ in want)
    # a map: contig B stands for batch tid 0, tid 1 has no contig, tid 2 is S
    tid_map = [1, -1, 2]
    want = [ru.nm_md(x, ru.REC_CONTIGS, tid_map) for x in recs]
    got = r.nm_md_host(*ru.stream_of(recs), tid_map=tid_map)
    assert list(zip(*got)) == want and sum(nm >= 0 for nm, _ in want) > 5
    for bad_map in ([3], [-2]):
        with pytest.raises(io.ffi.SlxError) as e:
            r.nm_md_host(*ru.stream_of(recs), tid_map=bad_map)
        assert e.value.code == io.ffi.SLX_EINVAL
    assert r.nm_md_host(b"", [0]) == ([], [])
    r.close()


@pytest.mark.parametrize("long_record", [1, None, 1 << 30], ids=["all_waves", "default", "all_lanes"])
def test_generated_records(io, bulk, bulk_ref, long_record):
    contigs, recs, want = bulk
    default = bulk_ref.counter("long_record")
    assert 1 < default < 20000          # both kernels run by default
    if long_record:
        bulk_ref.set("long_record", long_record)
    nm, md = bulk_ref.nm_md_host(*ru.stream_of(recs))
    bad = [i for i in range(len(recs)) if (nm[i], md[i]) != want[i]]
    assert not bad, (len(bad), bad[:5], [(nm[i], md[i][:60], want[i][0], want[i][1][:60]) for i in bad[:3]])
    lens = [ru.parse(r)["l_seq"] for r in recs]
    assert len(recs) > 2000 and max(lens) == 20000 and min(lens) <= 1 and max(len(ru.parse(r)["cig"]) for r in recs) > 64
    n_long = bulk_ref.counter("long_records")
    assert n_long == (sum(x >= 0 for x in nm) if long_record == 1 else 0 if long_record else sum(x >= 0 and l >= default for x, l in zip(nm, lens)))
    assert bulk_ref.counter("us_md_size") > 0 and bulk_ref.counter("us_md_text") > 0


def test_a_broken_record_fails_the_call(io, bulk, bulk_ref):
    contigs, recs, want = bulk
    good = recs[100:140]
    for k, bad in enumerate(ru.truncated(dict(ru.REC_CASES)["every_op"])):
        batch = good[:17] + [bad] + good[17:]
        with pytest.raises(io.ffi.SlxError) as e:
            bulk_ref.nm_md_host(*ru.stream_of(batch))
        assert e.value.code == io.ffi.SLX_EIO and "record 17 " in str(e.value)
    stream, off = ru.stream_of(good)
    for bad_off in (off[:5] + [off[5] + 1] + off[6:], off[:-1] + [off[-1] + 4]):
        with pytest.raises(io.ffi.SlxError) as e:
            bulk_ref.nm_md_host(stream, bad_off)
        assert e.value.code == io.ffi.SLX_EIO


def test_nm_equals_the_aligners(io, sl, tiny, tiny_ref, tiny_gpu):
    """an independent derivation: the aligner's NM tag of every forward-strand record it builds for the golden reads (reverse-strand records keep the glue's quirk
    of leaving C and G uncomplemented in SEQ, so they differ from the reference by construction: they run, and must equal the Python statement like the rest)"""
    text, contigs, _ = tiny
    al = sl.BWAAligner(tiny_gpu)
    L = open(os.path.join(GOLDEN, "sim1_bcr.head3000.fq")).read().split("\n")
    names, seqs = [L[i][1:].split()[0].encode() for i in range(0, len(L) - 3, 4)], [L[i + 1].encode() for i in range(0, len(L) - 3, 4)]
    rb = io.recio.Builder(al._handle())
    d_bases, d_offs, d_names, d_name_offs = rb.upload(seqs, names)
    hits = al.align_device(d_bases, d_offs, len(seqs), 0, False, 0.9, 10)
    b = rb.build(hits, d_bases, d_offs, d_names, d_name_offs, False)
    nm, md = tiny_ref.nm_md_device(b.d_stream, b.n_bytes, b.d_rec_off, b.n_records)
    recs = records_of_builder(rb, b)
    seqs_of = [c[5] for c in contigs]
    n_fwd = n_pos = n_d = n_i = n_s = 0
    for r, g_nm, g_md in zip(recs, nm, md):
        assert (g_nm, g_md) == ru.nm_md(r, seqs_of)
        p = ru.parse(r)
        if p["flag"] & 16:
            continue
        aux = r[36 + r[12] + 4 * len(p["cig"]) + (p["l_seq"] + 1) // 2 + p["l_seq"]:]
        at = aux.index(b"NMi")
        tag = struct.unpack_from("<i", aux, at + 3)[0]
        assert g_nm == tag, (r[36:36 + r[12] - 1], g_nm, tag, g_md)
        ops = {op for op, _ in p["cig"]}
        n_fwd += 1; n_pos += tag > 0; n_d += 2 in ops; n_i += 1 in ops; n_s += 4 in ops
    assert n_fwd >= 1400 and n_pos >= 800 and n_d >= 15 and n_i >= 5 and n_s >= 10, (n_fwd, n_pos, n_d, n_i, n_s)
    rb.close()
