"""The aligner and both index builders at the EDGES of the reference (run with -m gpu on an MI355X): contig ends, the forward / reverse boundary,
the first and last bases, contigs shorter than a seed, N holes (where the pac and the BWT text carry different random fills), and degenerate
texts through the 32-bit and the 64-bit suffix sorter.  Everything against the oracle, bit for bit; the indexes also against suffixes sorted
as Python strings.  tests/test_ref_edges_oracle.py holds the conditions that make these reads test cases."""
import filecmp

import numpy as np
import pytest

from tests import edge_util as eu
from tests.test_gpu_parity import SWEEP_KNOBS, assert_same, _check_sam_mode

pytestmark = pytest.mark.gpu

EXTS = ("bwt", "sa", "pac", "ann", "amb")


def _build_pair(sl, orc, refs):
    """the product's index and the oracle's from the same lrand48 state -> (idx, oidx, that state)"""
    from seqlib_amd import _ffi
    state = int(_ffi.lib().slx_lrand48_peek_libc())
    orc.lib().orc_rng_set_state(state)
    idx = sl.BWAIndex()
    idx.ConstructIndex(refs)
    oidx = orc.Index.build([n for n, _ in refs], [s for _, s in refs])
    assert int(_ffi.lib().slx_lrand48_peek_libc()) == int(orc.lib().orc_rng_get_state())
    return idx, oidx, state


def _pac_of(idx, refs, tmp_path, name):
    prefix = str(tmp_path / name)
    idx.WriteIndex(prefix)
    return eu.pac_text(prefix, sum(len(s) for _, s in refs)), prefix


def _aligner(sl, idx, knobs=()):
    al = sl.BWAAligner(idx)
    for k, v in knobs:
        al.set(k, v)
    return al


# ---------------------------------------------------------------- Part A: both builders on degenerate texts
def _texts():
    rng = np.random.default_rng(77)
    u = eu.rand_seq(rng, 500)
    return {"A": [("x", "A")], "13": [("x", "ACGTACGTACGTA")], "A300": [("x", "A" * 300)], "AC200": [("x", "AC" * 200)], "AT100": [("x", "AT" * 100)],
            "ACGT64": [("x", "ACGT" * 64)], "63+T": [("a", eu.rand_seq(rng, 63)), ("b", "T")], "uuuU": [("u", u + u + u + eu.revcomp(u))],
            "EDGE": eu.edge_ref(), "EDGE64": eu.edge_ref(61), "TINY300": eu.tiny300_ref(), "N40": [("n", "N" * 40)]}


@pytest.mark.parametrize("build64", [0, 1], ids=["build32", "build64"])
@pytest.mark.parametrize("name", ["A", "13", "A300", "AC200", "AT100", "ACGT64", "63+T", "uuuU", "EDGE", "EDGE64", "TINY300", "N40"])
def test_both_builders_on_degenerate_texts(sl, orc, tmp_path, monkeypatch, name, build64):
    """texts shorter than the 27-symbol first key, of 2 symbols, of a multiple of 128 symbols, homopolymers, a tandem that runs through the strand
    boundary, a text and its reverse complement, many tiny contigs, contigs of N: the files are the oracle's byte for byte, and (up to 4 000 symbols)
    primary and every SA sample are those of the suffixes sorted as strings"""
    if build64:
        monkeypatch.setenv("SLX_BUILD64", "1")
    refs = _texts()[name]
    seqs = [s for _, s in refs]
    idx, oidx, state = _build_pair(sl, orc, refs)
    g, o = str(tmp_path / "g"), str(tmp_path / "o")
    idx.WriteIndex(g)
    oidx.write(o)
    for ext in EXTS:
        assert filecmp.cmp(g + "." + ext, o + "." + ext, shallow=False), ext
    total = sum(len(s) for s in seqs)
    pac, bwt = eu.both_fills(seqs, state)
    assert eu.pac_text(g, total) == pac
    if 2 * total <= 4000:
        eu.check_against_brute_sa(g, bwt)
    if name == "EDGE":
        idx2 = sl.BWAIndex()
        idx2.LoadIndex(g)
        g2 = str(tmp_path / "g2")
        idx2.WriteIndex(g2)
        for ext in EXTS:
            assert filecmp.cmp(g + "." + ext, g2 + "." + ext, shallow=False), ext


# ---------------------------------------------------------------- Part B: 150 bp reads at every edge, on every route
def test_reads_at_every_edge_on_every_route(sl, orc, tmp_path):
    """reads over every contig junction (a one-base contig and one shorter than a seed among them), over the forward / reverse boundary, on the
    first and last bases of the reference, a whole contig, a copy on another contig -- as they are, with substitutions next to the edge, with
    indels next to it, both strands -- through every schedule knob, hard clips and the record mode: the oracle's records, all inside their contigs"""
    refs = eu.edge_ref()
    lens = [len(s) for _, s in refs]
    idx, oidx, _ = _build_pair(sl, orc, refs)
    F, _ = _pac_of(idx, refs, tmp_path, "e")
    seqs = eu.with_forms(eu.edge_reads(refs, F))
    assert len(seqs) == 6 * (eu.n_junction_reads(refs) + 12)
    opt = orc.default_opt()
    exp = orc.align_batch(opt, oidx, seqs)
    assert eu.inside_contig(exp, lens)
    for knobs in SWEEP_KNOBS:
        got = _aligner(sl, idx, knobs).alignSequences(seqs)
        assert eu.inside_contig(got, lens), knobs
        assert_same(got, exp, "edge reads %s" % (knobs,))
    got = _aligner(sl, idx).alignSequences(seqs, hardclip=True)
    assert_same(got, orc.align_batch(opt, oidx, seqs, hardclip=True), "edge reads, hard clips")
    assert eu.inside_contig(got, lens)
    _check_sam_mode(sl, orc, idx, oidx, seqs, "edge reads, record mode")


@pytest.mark.parametrize("which", ["EDGE64", "TINY300"])
def test_reads_at_every_edge_other_references(sl, orc, tmp_path, which):
    """the same reads on a text of a multiple of 128 symbols, and 218 reads each over three or more of 300 contigs of 20 to 60 bases"""
    refs = eu.edge_ref(61) if which == "EDGE64" else eu.tiny300_ref()
    lens = [len(s) for _, s in refs]
    idx, oidx, _ = _build_pair(sl, orc, refs)
    F, _ = _pac_of(idx, refs, tmp_path, "e")
    if which == "EDGE64":
        seqs = eu.with_forms(eu.edge_reads(refs, F))
    else:
        plain = eu.tiny300_reads(F)
        assert len(plain) >= 200
        seqs = eu.with_forms([("", r, 75) for r in plain])
    got = _aligner(sl, idx).alignSequences(seqs)
    assert eu.inside_contig(got, lens)
    assert_same(got, orc.align_batch(orc.default_opt(), oidx, seqs), which)


# ---------------------------------------------------------------- Part C: long reads at the edges
def test_long_reads_at_contig_ends(sl, orc, tmp_path):
    """contig-length reads that overhang a contig's end, span a whole contig and both its neighbours, run through the forward / reverse boundary or
    start / end beyond the reference -- the block, segment and band kernels and the wide build at a junction -- clean and mutated, on the default
    route, with each long-read form switched off, on the u64 index, with the sampled SA, and among short reads"""
    refs = eu.long3_ref()
    lens = [len(s) for _, s in refs]
    idx, oidx, _ = _build_pair(sl, orc, refs)
    base, muts = eu.long3_reads(refs)
    seqs = [r for _, r, _ in base + muts]
    assert max(len(r) for r in seqs) >= 70000          # beyond the 16-bit packings: the wide build
    opt = orc.default_opt()
    exp = orc.align_batch(opt, oidx, seqs)
    assert eu.inside_contig(exp, lens)
    for knobs in ((), (("wide_index", 1),), (("long_budget", 0),), (("long_seg", 0),), (("long_block", 0),), (("long_coop", 0),), (("xseg_fail", 1),), (("dense_sa", 0),)):
        got = _aligner(sl, idx, knobs).alignSequences(seqs)
        assert eu.inside_contig(got, lens), knobs
        assert_same(got, exp, "long reads at contig ends %s" % (knobs,))
    A = refs[0][1]
    short = [A[100 + 151 * i:250 + 151 * i] for i in range(40)]
    mixed = seqs[:5] + short[:20] + seqs[5:12] + short[20:] + seqs[12:]
    got = _aligner(sl, idx).alignSequences(mixed)
    assert eu.inside_contig(got, lens)
    assert_same(got, orc.align_batch(opt, oidx, mixed), "long reads at contig ends among short reads")


# ---------------------------------------------------------------- Part D: reads over N holes
def _hole_case(sl, orc, refs):
    idx, oidx, state = _build_pair(sl, orc, refs)
    pac, bwt = eu.both_fills([s for _, s in refs], state)
    hr = eu.hole_reads(refs, pac, bwt)
    seqs = [r for _, rp, rb in hr for r in (rp, rb)]
    return idx, oidx, pac, seqs


def _check_stage0(sl, orc, idx, oidx, seqs, what):
    al = sl.BWAAligner(idx)
    al.set("keep_stages", 1)
    al.alignSequences(seqs)
    opt = orc.default_opt()
    for i in (0, 1):          # the hole read in its pac form and in its BWT form
        got, exp = al.debug_stage(i, 0), orc.stage_dump(opt, oidx, seqs[i], 0)
        assert np.array_equal(got, exp), "%s: intervals of read %d differ\n gpu=%s\n cpu=%s" % (what, i, got.reshape(-1, 4), exp.reshape(-1, 4))


def test_reads_over_N_holes(sl, orc, tmp_path, tiny_gpu, monkeypatch):
    """an in-memory build draws lrand48() for every N twice, once for the pac and once for the BWT text, so inside a hole the FM-index and the pac
    hold different bases: seeds follow the BWT text, extension and NM follow the pac.  Reads that carry either fill, that end inside the hole, that
    cross a single N, that have N or other bases there: the oracle's records and SMEMs on every route that reads the text directly, on the index
    written and loaded again, and through the 64-bit builder"""
    refs = eu.edge_ref()
    lens = [len(s) for _, s in refs]
    idx, oidx, pac, seqs = _hole_case(sl, orc, refs)
    F, prefix = _pac_of(idx, refs, tmp_path, "h")
    assert F == pac          # the pac's fill is the first-pass draws
    assert sum(a != b for a, b in zip(seqs[0], seqs[1])) >= 20
    opt = orc.default_opt()
    exp = orc.align_batch(opt, oidx, seqs)
    _check_stage0(sl, orc, idx, oidx, seqs, "built in memory")          # (first: the pac-form read's records are 150M either way, its SMEMs are not)
    for knobs in ((), (("dense_sa", 0),), (("bwd_direct", 1),), (("rep_k", 0),), (("wide_index", 1),)):
        got = _aligner(sl, idx, knobs).alignSequences(seqs)
        assert eu.inside_contig(got, lens)
        assert_same(got, exp, "reads over N holes %s" % (knobs,))
    # the direct text steps are off for an index whose pac is not its BWT text, and on for one whose pac is
    assert _aligner(sl, idx).counter("text_is_pac") == 0
    assert _aligner(sl, tiny_gpu).counter("text_is_pac") == 1
    # the same files loaded again
    idx2 = sl.BWAIndex()
    idx2.LoadIndex(prefix)
    al = _aligner(sl, idx2)
    assert_same(al.alignSequences(seqs), exp, "reads over N holes, index written and loaded")
    assert al.counter("text_is_pac") == 0
    _check_stage0(sl, orc, idx2, oidx, seqs, "written and loaded")
    # the 64-bit builder (fresh draws: other fills, other reads)
    monkeypatch.setenv("SLX_BUILD64", "1")
    idx3, oidx3, _, seqs3 = _hole_case(sl, orc, refs)
    assert_same(_aligner(sl, idx3).alignSequences(seqs3), orc.align_batch(opt, oidx3, seqs3), "reads over N holes, 64-bit builder")


def test_repeat_filter_on_a_hole(sl, orc):
    """an 81-mer that occurs twice in the BWT text and once in the pac (its first copy holds an N, the second the BWT text's draw for it): the re-seeding
    call from the middle of the read finds the second copy, which a repeat filter built from the pac would rule out"""
    from seqlib_amd import _ffi
    n_skipped = 0
    for _ in range(8):          # (one draw in four gives both fills the same base: take the next state)
        refs, read, d = eu.rep_ref(int(_ffi.lib().slx_lrand48_peek_libc()))
        if d[0] != d[1]:
            break
        n_skipped += 1
        _ffi.lib().slx_lrand48_skip_libc(1)
    assert d[0] != d[1] and n_skipped < 8
    idx, oidx, state = _build_pair(sl, orc, refs)
    pac, bwt = eu.both_fills([s for _, s in refs], state)
    assert bwt.count(read[30:111]) == 2 and pac.count(read[30:111]) == 1
    opt = orc.default_opt()
    exp = orc.align_batch(opt, oidx, [read])
    iv = orc.stage_dump(opt, oidx, read, 0).reshape(-1, 4)
    assert any(int(n) == 2 for _, _, _, n in iv), iv          # the re-seeding call kept the 81-mer's interval
    for knobs in ((), (("rep_k", 0),)):
        al = _aligner(sl, idx, knobs)
        al.set("keep_stages", 1)
        assert_same(al.alignSequences([read]), exp, "repeat over a hole %s" % (knobs,))
        assert np.array_equal(al.debug_stage(0, 0), iv.reshape(-1)), knobs
