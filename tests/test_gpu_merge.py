"""GPU tests of the merge of coordinate-sorted BAM files (include/seqlib_amd_merge.h) through seqlib_amd/mergeio.py, and of the sort beyond HBM that uses it
(slx_sort_spill, seqlib_amd/sortio.py): the merged stream is Python's sorted() of the concatenation of the inputs byte for byte, ties by input and then by
position; the knobs change nothing; the output is what slx_bam_index_build and the region iteration take; the refusals; a spilling sort writes the file the
sort in HBM writes.  The expectations are tests/merge_util.py's.  The C++ side is tests/test_cpp_merge.py."""
import glob
import re

import pytest

from tests import bai_util as ba
from tests import bam_util as bu
from tests import merge_util as mu

pytestmark = pytest.mark.gpu

BATCH = 0x2000


@pytest.fixture(scope="module")
def cases(sl, tmp_path_factory):
    """make(k) -> the k input files (members of 0x2000 bytes) of mu.build_inputs(k, block_in=k - 1) and Python's answer; computed once per k"""
    d = tmp_path_factory.mktemp("merge")
    made = {}

    def write(name, inputs, texts=None, refs=None):
        paths = []
        for i, recs in enumerate(inputs):
            p = d / ("%s_%02d.bam" % (name, i))
            p.write_bytes(bu.bam_bytes(texts[i] if texts else bu.TEXT, refs[i] if refs else bu.REFS, recs, member_size=BATCH))
            paths.append(p)
        return paths

    def make(k):
        if k not in made:
            inputs = mu.build_inputs(k, block_in=k - 1)
            want, frm = mu.expected_merge(inputs)
            made[k] = dict(inputs=inputs, paths=write("k%d" % k, inputs), want=want, frm=frm, header=bu.bam_header(mu.header_rule([bu.TEXT] * k), bu.REFS))
        return made[k]

    make.dir = d
    make.write = write
    return make


def merged(paths, **knobs):
    """-> (stream, offsets, inputs, batches that came, the merger's counters)"""
    from seqlib_amd import mergeio
    m = mergeio.Merger()
    for k, v in knobs.items():
        m.set(k, v)
    for p in paths:
        m.add_file(p)
    stream, off, inp, n = [], [0], [], 0
    while True:
        s, o, i = m.next()
        if not i:
            break
        n += 1
        off += [off[-1] + x for x in o[1:]]
        stream.append(s)
        inp += i
    c = {name: m.counter(name) for name in mergeio.COUNTERS}
    head = m.header()
    m.close()
    return b"".join(stream), off, inp, n, c, head


def check_merged(got, off, inp, want, frm):
    assert len(off) == len(want) + 1 and off[0] == 0 and off[-1] == len(got)
    for j, r in enumerate(want):
        assert got[off[j]:off[j + 1]] == r, "record %d of the merged stream differs" % j
    assert got == b"".join(want)
    assert inp == frm


@pytest.mark.parametrize("k", [1, 2, 3, 64])
def test_order_ties_and_inputs(cases, k):
    c = cases(k)
    got, off, inp, n, cnt, head = merged(c["paths"], batch_bytes=BATCH)
    check_merged(got, off, inp, c["want"], c["frm"])
    assert head == c["header"]
    ties = [i for r, i in zip(c["want"], inp) if mu.key(r) == mu.TIE_AT]
    assert len(ties) == mu.N_TIES and ties == sorted(ties) and len(set(ties)) == min(k, mu.N_TIES)          # the 130 ties by input, over all inputs
    assert cnt["inputs"] == k and cnt["records"] == len(c["want"]) and cnt["bytes"] == len(got) and cnt["held_records"] == 0 and cnt["held_bytes"] == 0
    # the 400-record block is longer than a batch: while the window held nothing but the block, a round emitted nothing and read on
    assert cnt["rounds"] > n + 1, (cnt, n)
    assert cnt["refills"] >= k + 3


def test_header_only_and_one_record_inputs(cases):
    base = mu.build_inputs(2)
    one = [bu.bam_record("only", 0, 1, 4242, 30, [("M", 20)], "ACGTA" * 4, bytes([30]) * 20)]          # at the tie block's key: it goes behind the ties of inputs 0 and 1
    inputs = [base[0], [], base[1], one, []]
    paths = cases.write("edge", inputs)
    want, frm = mu.expected_merge(inputs)
    got, off, inp, _, cnt, _ = merged(paths, batch_bytes=BATCH)
    check_merged(got, off, inp, want, frm)
    at = [j for j, r in enumerate(want) if mu.key(r) == mu.TIE_AT]
    assert frm[at[-1]] == 3 and want[at[-1]] == one[0] and cnt["inputs"] == 5
    # nothing but headers, and a single record
    got, off, inp, n, _, _ = merged(cases.write("empty", [[], []]))
    assert (got, off, inp, n) == (b"", [0], [], 0)
    got, off, inp, n, _, _ = merged(cases.write("single", [[], one]))
    assert (got, off, inp, n) == (one[0], [0, len(one[0])], [1], 1)


def test_knobs_change_nothing(cases):
    from seqlib_amd import mergeio
    c = cases(3)
    first = None
    for batch_bytes in (BATCH, 3 * BATCH + 7, None):
        for slab_bytes in (2048, 6144, None):
            for by_sort in (0, 1):
                out = cases.dir / ("out_%s_%s_%d.bam" % (batch_bytes, slab_bytes, by_sort))
                cnt = mergeio.merge_files(c["paths"], out, batch_bytes=batch_bytes, slab_bytes=slab_bytes, by_sort=by_sort)
                raw = out.read_bytes()
                out.unlink()
                if first is None:
                    first = raw
                    assert bu.inflate_all(raw) == c["header"] + b"".join(c["want"])
                    text, refs, recs = bu.parse_bam(raw)
                    assert text == mu.header_rule([bu.TEXT] * 3) and refs == bu.REFS and [r["raw"] for r in recs] == c["want"]
                assert raw == first, (batch_bytes, slab_bytes, by_sort)
                assert cnt["records"] == len(c["want"]) and cnt["held_records"] == 0
                if batch_bytes == BATCH:
                    assert cnt["rounds"] > 10, cnt
    out = cases.dir / "plain.bam"
    assert mergeio.merge_files(c["paths"], out) == {} and out.read_bytes() == first          # slx_merge_files itself, every knob at its default


def test_it_closes_the_loop(cases):
    """the output is what the index build demands and what the region iteration serves"""
    from seqlib_amd import bamio, mergeio
    c = cases(3)
    out = cases.dir / "loop.bam"
    mergeio.merge_files(c["paths"], out)
    bamio.index_build(out)
    raw = out.read_bytes()
    assert (cases.dir / "loop.bam.bai").read_bytes() == ba.build_bai(raw)          # (the Python builder raises Unsorted on a bad order)
    _, _, recs = bu.parse_bam(raw)
    rd = bamio.Reader(out)
    assert rd.has_index()
    for region in ((1, 4000, 4300), (0, 0, 30000), (2, 4990, 5010)):
        rd.set_regions([region])
        got = []
        while True:
            r, _ = rd.next()
            if not r:
                break
            got += r
        want = ba.region_filter(recs, *region)
        assert got == want and want, region
    rd.close()


def test_refusals(cases, tmp_path):
    from seqlib_amd import _ffi, mergeio
    c = cases(2)
    out = tmp_path / "out.bam"
    good = c["paths"]
    # an unsorted input: the path and the record's ordinal in the file; no output file
    recs = list(c["inputs"][1])
    at = 150                                                             # beyond the first batch of 0x2000 bytes: the ordinal counts from the file's start
    assert mu.key(recs[at]) < mu.key(recs[at + 3])
    recs[at], recs[at + 3] = recs[at + 3], recs[at]
    first_bad = next(j for j in range(1, len(recs)) if mu.key(recs[j]) < mu.key(recs[j - 1]))
    bad = cases.write("unsorted", [recs])[0]
    for knobs in ({}, {"batch_bytes": BATCH}):
        with pytest.raises(_ffi.SlxError) as e:
            mergeio.merge_files([good[0], bad], out, **knobs)
        assert e.value.code == _ffi.SLX_EINVAL and str(bad) in str(e.value) and "record %d " % first_bad in str(e.value) and "not coordinate-sorted" in str(e.value), str(e.value)
        assert not out.exists()
    # different references: the input and the reference index
    refs2 = [bu.REFS[0], (bu.REFS[1][0], bu.REFS[1][1] + 1), bu.REFS[2]]
    other = cases.write("refs", [c["inputs"][1]], refs=[refs2])[0]
    with pytest.raises(_ffi.SlxError) as e:
        mergeio.merge_files([good[0], other], out)
    assert e.value.code == _ffi.SLX_EINVAL and "input 1 " in str(e.value) and "reference 1 " in str(e.value) and not out.exists(), str(e.value)
    fewer = cases.write("fewer", [c["inputs"][1]], refs=[bu.REFS[:2]])[0]
    with pytest.raises(_ffi.SlxError) as e:
        mergeio.merge_files([good[0], fewer], out)
    assert e.value.code == _ffi.SLX_EINVAL and "reference 2 " in str(e.value) and not out.exists(), str(e.value)
    # an @RG ID clash
    rg = cases.write("rg", [c["inputs"][0], c["inputs"][1]], texts=[bu.TEXT + "@RG\tID:lane1\tSM:one\n", bu.TEXT + "@RG\tID:lane1\tSM:two\n"])
    with pytest.raises(_ffi.SlxError) as e:
        mergeio.merge_files(rg, out)
    assert e.value.code == _ffi.SLX_EUNSUPPORTED and "ID:lane1" in str(e.value) and not out.exists(), str(e.value)
    # 65 inputs
    with pytest.raises(_ffi.SlxError) as e:
        mergeio.merge_files([good[0]] * 65, out)
    assert e.value.code == _ffi.SLX_EUNSUPPORTED and "65" in str(e.value) and "64" in str(e.value) and not out.exists(), str(e.value)
    # the output is an input, or a pipe
    before = good[1].read_bytes()
    for knobs in ({}, {"batch_bytes": BATCH}):
        with pytest.raises(_ffi.SlxError) as e:
            mergeio.merge_files(good, good[1], **knobs)
        assert e.value.code == _ffi.SLX_EINVAL and good[1].read_bytes() == before
    with pytest.raises(_ffi.SlxError) as e:
        mergeio.merge_files([good[0], "-"], out)
    assert e.value.code == _ffi.SLX_EINVAL and not out.exists()
    # a merger goes on after refused inputs: they were not added
    m = mergeio.Merger()
    m.add_file(good[0])
    for p in (other, fewer, "-", tmp_path / "no_such_file.bam"):
        with pytest.raises(_ffi.SlxError):
            m.add_file(p)
    m.add_file(good[1])
    assert m.counter("inputs") == 2 and m.header() == c["header"]
    for _ in range(62):
        m.add_file(good[1])
    with pytest.raises(_ffi.SlxError) as e:
        m.add_file(good[1])
    assert e.value.code == _ffi.SLX_EUNSUPPORTED and m.counter("inputs") == 64
    for key, v in (("slab_bytes", 1000), ("by_sort", 2), ("batch_bytes", 0), ("max_bytes", 0), ("nonsense", 1)):
        with pytest.raises(_ffi.SlxError) as e:
            m.set(key, v)
        assert e.value.code == _ffi.SLX_EINVAL
    assert m.counter("no_such_counter") == -1
    m.close()
    # and the two good files merge after all of this
    mergeio.merge_files(good, out)
    assert bu.inflate_all(out.read_bytes()) == c["header"] + b"".join(c["want"])


# ---------------------------------------------------------------- the sort beyond HBM
SPILL_BATCH = 0x1000


@pytest.fixture(scope="module")
def unsorted(sl, tmp_path_factory):
    """the unsorted file of tests/test_gpu_sort.py's shape without its 10 000-byte record (so that every reader batch of 0x1000 bytes fits the smallest budget
    below), members of 0x1000 bytes; the sizes of the reader's batches, which are the sorter's adds; the file the sort in HBM writes"""
    from seqlib_amd import bamio, sortio
    d = tmp_path_factory.mktemp("spill")
    recs = [r for r in mu.base_records() if len(r) != 10000]
    path = d / "in.bam"
    path.write_bytes(bu.bam_bytes(bu.TEXT, bu.REFS, recs, member_size=SPILL_BATCH))
    rd = bamio.Reader(path)
    sizes = []
    while True:
        r, b = rd.next(SPILL_BATCH)
        if not r:
            break
        sizes.append(b.n_bytes)
    rd.close()
    assert sum(sizes) == sum(len(r) for r in recs)
    fit = d / "fit.bam"
    sortio.sort_file(path, fit, batch_bytes=SPILL_BATCH)
    assert bu.inflate_all(fit.read_bytes()) == bu.bam_header(bu.TEXT.replace("SO:unsorted", "SO:coordinate"), bu.REFS) + b"".join(sorted(recs, key=mu.key))
    return dict(dir=d, path=path, sizes=sizes, fit=fit.read_bytes(), recs=recs)


@pytest.mark.parametrize("max_bytes", [12000, 40000, 100000])
def test_spill_sorts_beyond_the_budget(unsorted, max_bytes):
    from seqlib_amd import sortio
    runs = mu.expected_runs(unsorted["sizes"], max_bytes)
    assert runs is not None and 2 <= runs <= 64, (runs, max(unsorted["sizes"]))          # the sizes were picked so: every batch fits, the runs can be merged in one pass
    out = unsorted["dir"] / ("spill_%d.bam" % max_bytes)
    c = sortio.sort_file(unsorted["path"], out, spill_prefix=unsorted["dir"] / "tmp", max_bytes=max_bytes, batch_bytes=SPILL_BATCH)
    assert c["runs"] == runs and c["run_bytes"] == sum(unsorted["sizes"]) and c["held_records"] == 0 and c["records"] == len(unsorted["recs"]), c
    assert out.read_bytes() == unsorted["fit"]                  # byte for byte the file of the sort that held everything
    assert not glob.glob(str(unsorted["dir"] / "*.run*.bam"))
    # the prefix defaults to the output's name, and a budget that holds everything spills nothing
    c = sortio.Sorter()
    c.set("max_bytes", max_bytes)
    c.set("batch_bytes", SPILL_BATCH)
    from seqlib_amd import _ffi
    _ffi.check(sortio.lib().slx_sort_file_spill(c.h, str(unsorted["path"]).encode(), str(out).encode(), None))
    assert c.counter("runs") == runs and out.read_bytes() == unsorted["fit"] and not glob.glob(str(unsorted["dir"] / "*.run*.bam"))
    c.set("max_bytes", 1 << 30)
    c.sort_file(unsorted["path"], out, spill_prefix=unsorted["dir"] / "tmp")
    assert c.counter("runs") == runs and out.read_bytes() == unsorted["fit"]
    c.close()


def test_spill_refusals(unsorted, tmp_path):
    from seqlib_amd import _ffi, sortio
    out = tmp_path / "out.bam"
    total = sum(unsorted["sizes"])
    # without a prefix the refusal is today's: both figures, no file, the sorter goes on
    s = sortio.Sorter()
    s.set("max_bytes", 100000)
    s.set("batch_bytes", SPILL_BATCH)
    with pytest.raises(_ffi.SlxError) as e:
        s.sort_file(unsorted["path"], out)
    figures = [int(x) for x in re.findall(r"\d+", str(e.value))]
    assert e.value.code == _ffi.SLX_EUNSUPPORTED and 100000 in figures and any(100000 < f <= total for f in figures), str(e.value)
    assert not out.exists() and s.counter("held_records") == 0 and s.counter("runs") == 0
    # a single add beyond max_bytes stays refused with a prefix too, and leaves no run behind
    s.set("max_bytes", max(unsorted["sizes"]) - 1)
    with pytest.raises(_ffi.SlxError) as e:
        s.sort_file(unsorted["path"], out, spill_prefix=tmp_path / "tmp")
    assert e.value.code == _ffi.SLX_EUNSUPPORTED and not out.exists() and not glob.glob(str(tmp_path / "*.run*.bam"))
    # more than 64 runs: every batch fits, but each is a run of its own
    small = [bu.bam_record("s%04d" % i, 0, i % 3, (i * 7919) % 90000, 30, [("M", 20)], "ACGTA" * 4, bytes([30]) * 20) for i in range(1500)]
    many = tmp_path / "many.bam"
    many.write_bytes(bu.bam_bytes(bu.TEXT, bu.REFS, small, member_size=0x200))
    from seqlib_amd import bamio
    rd = bamio.Reader(many)
    sizes = []
    while True:
        r, b = rd.next(0x200)
        if not r:
            break
        sizes.append(b.n_bytes)
    rd.close()
    s.set("batch_bytes", 0x200)
    s.set("max_bytes", max(sizes))
    assert mu.expected_runs(sizes, max(sizes)) > 64
    runs_before = s.counter("runs")
    with pytest.raises(_ffi.SlxError) as e:
        s.sort_file(many, out, spill_prefix=tmp_path / "tmp")
    assert e.value.code == _ffi.SLX_EUNSUPPORTED and "65" in str(e.value) and "64" in str(e.value), str(e.value)
    assert not out.exists() and not glob.glob(str(tmp_path / "*.run*.bam")) and s.counter("runs") - runs_before == 64 and s.counter("held_records") == 0
    # with runs pending the sorted stream does not come down, and the marker does not mark
    s.set("max_bytes", 1 << 30)
    recs = unsorted["recs"][:40]
    head = bu.bam_header(bu.TEXT, bu.REFS)
    s.spill(tmp_path / "pend", head)
    s.set("max_bytes", max(sum(len(r) for r in recs[:20]), sum(len(r) for r in recs[20:])))
    s.add_host(recs[:20])
    s.add_host(recs[20:40])                                     # passes the budget: the first twenty are a run now
    assert len(glob.glob(str(tmp_path / "pend.run*.bam"))) == 1 and s.counter("held_records") == 20
    with pytest.raises(_ffi.SlxError) as e:
        s.to_host()
    assert e.value.code == _ffi.SLX_EUNSUPPORTED and "slx_sort_finish" in str(e.value)
    from seqlib_amd import dupio
    d = dupio.Marker()
    with pytest.raises(_ffi.SlxError) as e:
        d.mark_sorter(s.h)
    assert e.value.code == _ffi.SLX_EUNSUPPORTED and "slx_dup_file" in str(e.value)
    d.close()
    w = bamio.Writer(out)
    w.write(head)
    w.flush()
    s.finish(w)
    w.close()
    assert bu.inflate_all(out.read_bytes()) == head + b"".join(sorted(recs, key=mu.key)) and not glob.glob(str(tmp_path / "pend.run*.bam"))
    s.spill(tmp_path / "gone", head)
    s.add_host(recs[:20])
    s.add_host(recs[20:40])
    assert len(glob.glob(str(tmp_path / "gone.run*.bam"))) == 1
    s.close()                                                   # a sorter that is freed takes its runs with it
    assert not glob.glob(str(tmp_path / "gone.run*.bam"))
