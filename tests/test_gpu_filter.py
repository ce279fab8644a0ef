"""GPU tests of the read filter at the C-ABI (include/seqlib_amd_filter.h through seqlib_amd/filterio.py) against the Python statement of the rules in
tests/filter_util.py: the keep mask of slx_filter_apply_device for every rule set and for the smallest and the default stage, the filtered batches of
slx_bam_next byte for byte (whole file and regions), the counters, detaching, a filtered batch going on to slx_bam_reads_device and slx_bgzf_write_device, and
the refusal of damaged records.  The C++ classes are driven in tests/test_cpp_filter.py."""
import ctypes as C

import pytest

from tests import bai_util as ba
from tests import bam_util as bu
from tests import filter_util as fu

pytestmark = pytest.mark.gpu


class Hip:
    """the HIP runtime the library runs on, for device buffers of the tests' own"""

    def __init__(self):
        paths = sorted({ln.split()[-1] for ln in open("/proc/self/maps") if "libamdhip64" in ln}, key=lambda x: "torch" in x)
        assert paths, "no HIP runtime mapped"
        self.l = C.CDLL(paths[0])
        self.l.hipMalloc.argtypes = [C.POINTER(C.c_void_p), C.c_size_t]
        self.l.hipMemcpy.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int]
        self.l.hipFree.argtypes = [C.c_void_p]

    def up(self, data):
        p = C.c_void_p()
        assert self.l.hipMalloc(C.byref(p), max(len(data), 1)) == 0
        assert self.l.hipMemcpy(p, bytes(data), len(data), 1) == 0
        return p.value

    def down(self, p, n):
        buf = C.create_string_buffer(max(n, 1))
        assert self.l.hipMemcpy(buf, p, n, 2) == 0
        return buf.raw[:n]

    def free(self, p):
        self.l.hipFree(p)


@pytest.fixture(scope="module")
def fx(sl, tmp_path_factory):
    """the records, the model's masks (its coverage condition asserted) and the file with small BGZF members, once"""
    from seqlib_amd import bamio, filterio
    filterio.lib()

    class F:
        pass
    f = F()
    f.bamio, f.filterio, f.hip = bamio, filterio, Hip()
    f.recs = fu.records()
    f.parsed = fu.parsed(f.recs)
    f.masks = fu.coverage(f.parsed)
    d = tmp_path_factory.mktemp("flt")
    f.path = d / "f.bam"
    f.path.write_bytes(bu.bam_bytes(bu.TEXT, bu.REFS, f.recs, member_size=0x1800))
    f.sorted_raw = ba.sorted_bam()
    f.sorted_recs = bu.parse_bam(f.sorted_raw)[2]
    f.sorted_path = d / "s.bam"
    f.sorted_path.write_bytes(f.sorted_raw)
    (d / "s.bam.bai").write_bytes(ba.build_bai(f.sorted_raw))
    stream, off = fu.stream_of(f.recs)
    f.n_bytes = len(stream)
    f.d_stream = f.hip.up(stream)
    f.d_off = f.hip.up(b"".join(off[i].to_bytes(8, "little") for i in range(len(off))))
    f.d_keep = f.hip.up(bytes(len(f.recs)))
    yield f
    for p in (f.d_stream, f.d_off, f.d_keep):
        f.hip.free(p)


def read_all(rd, max_bytes):
    out, batches = [], 0
    while True:
        raws, b = rd.next(max_bytes)
        if not raws:
            assert b.n_records == 0
            return out, batches
        assert b.n_bytes == sum(len(x) for x in raws)
        out += raws
        batches += 1


@pytest.mark.parametrize("name", list(fu.RULE_SETS))
def test_apply_device_equals_the_model(fx, name):
    """every rule set; the smallest legal stage (every record of 113 bytes or more is a long one) and the default one give the same mask"""
    want = fx.masks[name]
    got = {}
    for window, overhang, chunk in ((16384, 2048, 0), (64, 48, 0), (256, 64, 5)):
        flt = fx.filterio.Filter(fu.RULE_SETS[name])
        flt.set("overhang_bytes", 48)
        flt.set("window_bytes", window)
        flt.set("overhang_bytes", overhang)
        flt.set("chunk_bases", chunk)
        n = flt.apply_device(fx.d_stream, fx.d_off, len(fx.recs), fx.d_keep)
        got[window] = [bool(x) for x in fx.hip.down(fx.d_keep, len(fx.recs))]
        assert n == sum(want) and flt.counter("seen") == len(fx.recs) and flt.counter("passed") == n
        assert flt.counter("long_records") >= (2 if window == 16384 else 100)
        if "motif" in name:
            assert flt.counter("dfa_states") > 1 and flt.counter("dfa_in_lds") == 1
        flt.close()
    bad = [i for i, (a, b) in enumerate(zip(got[16384], want)) if a != b]
    assert not bad, (name, bad[:10], [fx.parsed[i]["name"] for i in bad[:10]])
    assert got[64] == got[16384] and got[256] == got[16384]


def test_apply_device_with_a_large_motif_set_reads_the_automaton_from_hbm(fx):
    import random
    rng = random.Random(3)
    motifs = ["".join(rng.choice("ACGT") for _ in range(20)) for _ in range(1000)] + [fu.PLANT]
    filters = [dict(rules=[dict(motifs=motifs)])]
    flt = fx.filterio.Filter(filters)
    flt.apply_device(fx.d_stream, fx.d_off, len(fx.recs), fx.d_keep)
    assert flt.counter("dfa_states") > 15000 and flt.counter("dfa_in_lds") == 0
    got = [bool(x) for x in fx.hip.down(fx.d_keep, len(fx.recs))]
    want = fu.mask(filters, fx.parsed)
    assert got == want and any(want) and not all(want)


@pytest.mark.parametrize("max_bytes", [1, 4096, 1 << 30])
def test_attached_filter_compacts_the_batches(fx, max_bytes):
    for name in ("everything", "motif_links", "excluder"):
        want = [r["raw"] for r, k in zip(fx.parsed, fx.masks[name]) if k]
        flt = fx.filterio.Filter(fu.RULE_SETS[name])
        rd = fx.bamio.Reader(fx.path)
        flt.attach(rd)
        got, _ = read_all(rd, max_bytes)
        assert got == want, (name, len(got), len(want))
        assert flt.counter("seen") == len(fx.recs) and flt.counter("passed") == len(want)
        assert flt.counter("us_filter") > 0
        rd.close()
        flt.close()


def test_region_mode_and_filter(fx):
    regs = [(0, 16000, 60000), (1, 0, 30000), (3, 500, 99000)]
    for name in ("nm", "named_flags", "hardclip_off"):
        flt = fx.filterio.Filter(fu.RULE_SETS[name])
        rd = fx.bamio.Reader(fx.sorted_path)
        assert rd.has_index()
        rd.set_regions(regs)
        flt.attach(rd)
        by_raw = {r["raw"]: r for r in fx.sorted_recs}
        want = [x for g in regs for x in ba.region_filter(fx.sorted_recs, *g) if fu.keep(fu.RULE_SETS[name], by_raw[x])]
        for max_bytes in (1 << 30, 20000):
            rd.set_regions(regs)
            got, _ = read_all(rd, max_bytes)
            assert got == want and 0 < len(want) < sum(len(ba.region_filter(fx.sorted_recs, *g)) for g in regs), name
        rd.close()
        flt.close()


def test_drop_everything_keep_everything_and_detach(fx):
    plain = fx.bamio.Reader(fx.path)
    unfiltered, n_batches = read_all(plain, 8192)
    assert unfiltered == [r["raw"] for r in fx.parsed] and n_batches > 10
    none = fx.filterio.Filter([dict(rules=[dict(mapq=(200, 255, False))])])
    everything = fx.filterio.Filter([])
    rd = fx.bamio.Reader(fx.path)
    none.attach(rd)
    raws, b = rd.next(8192)                      # every span is walked, none holds a kept record: the end, once
    assert raws == [] and b.n_records == 0
    assert none.counter("seen") == len(fx.recs) and none.counter("passed") == 0
    assert rd.next(8192)[0] == []
    rd.rewind()
    everything.attach(rd)
    assert read_all(rd, 8192) == (unfiltered, n_batches)
    fx.filterio.Filter.detach(rd)
    rd.rewind()
    before = (none.counter("seen"), everything.counter("seen"))
    assert read_all(rd, 8192) == (unfiltered, n_batches)
    assert (none.counter("seen"), everything.counter("seen")) == before
    idle = fx.filterio.Filter(fu.RULE_SETS["mapq"])          # never attached, never applied
    assert idle.counter("us_filter") == 0 and idle.counter("seen") == 0
    for h in (rd, plain, none, everything, idle):
        h.close()


def test_a_filtered_batch_goes_on(fx, tmp_path):
    name = "len"
    want = [r for r, k in zip(fx.parsed, fx.masks[name]) if k]
    flt = fx.filterio.Filter(fu.RULE_SETS[name])
    rd = fx.bamio.Reader(fx.path)
    flt.attach(rd)
    raws, b = rd.next(1 << 30)
    assert raws == [w["raw"] for w in want]
    db, do, n, rmap = rd.reads_device(0, False)
    assert n == len(want) and rmap == list(range(n))
    offs = [int.from_bytes(fx.hip.down(do, 8 * (n + 1))[8 * i:8 * i + 8], "little") for i in range(n + 1)]
    bases = fx.hip.down(db, offs[-1]).decode()
    assert [bases[offs[i]:offs[i + 1]] for i in range(n)] == [w["seq"] for w in want]
    out = tmp_path / "kept.bam"
    w = fx.bamio.Writer(out)
    w.write(bu.bam_header(bu.TEXT, bu.REFS))
    w.flush()
    w.write_device(b.d_stream, b.n_bytes)
    w.close()
    assert [r["raw"] for r in bu.parse_bam(out.read_bytes())[2]] == [x["raw"] for x in want]
    rd.close()
    flt.close()


@pytest.mark.parametrize("case", list(fu.damaged()))
def test_damaged_records_are_refused_on_the_device(fx, sl, case, tmp_path):
    from seqlib_amd import _ffi
    good = fx.recs[:5]
    recs = good + [fu.damaged()[case]] + good
    stream, off = fu.stream_of(recs)
    d_s, d_o, d_k = fx.hip.up(stream), fx.hip.up(b"".join(o.to_bytes(8, "little") for o in off)), fx.hip.up(bytes(len(recs)))
    for window in (16384, 64):
        flt = fx.filterio.Filter(fu.RULE_SETS["nm"])
        flt.set("overhang_bytes", 48)
        flt.set("window_bytes", window)
        with pytest.raises(_ffi.SlxError) as e:
            flt.apply_device(d_s, d_o, len(recs), d_k)
        assert e.value.code == _ffi.SLX_EIO and "pass its block_size" in str(e.value)
        flt.close()
    path = tmp_path / "bad.bam"
    path.write_bytes(bu.bam_bytes(bu.TEXT, bu.REFS, recs))
    flt = fx.filterio.Filter(fu.RULE_SETS["nm"])
    rd = fx.bamio.Reader(path)
    flt.attach(rd)
    with pytest.raises(_ffi.SlxError) as e:
        rd.next()
    assert e.value.code == _ffi.SLX_EIO
    rd.close()
    flt.close()
    for p in (d_s, d_o, d_k):
        fx.hip.free(p)
