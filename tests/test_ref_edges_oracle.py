"""What the checker itself gives for the reads of tests/test_gpu_ref_edges.py: the conditions under which those GPU tests test anything (the
junction reads really split at the junction, the N fills really differ, the read that carries the BWT text's fill really seeds through the hole).
The oracle alone, its lrand48 at a fixed state; no GPU."""
import numpy as np
import pytest

from tests import edge_util as eu

STATE = 0x1234ABCD330E          # glibc's state before the first draw of an unseeded process


def _build(orc, refs, tmp, name, state=STATE):
    orc.lib().orc_rng_set_state(state)
    oidx = orc.Index.build([n for n, _ in refs], [s for _, s in refs])
    prefix = str(tmp / name)
    oidx.write(prefix)
    return oidx, eu.pac_text(prefix, sum(len(s) for _, s in refs)), prefix


def _m_covers_read(rec, L):
    return any((w & 0xf) == 0 and (w >> 4) == L for w in rec["cigar"])


@pytest.fixture(scope="module")
def edge(orc, tmp_path_factory):
    refs = eu.edge_ref()
    oidx, F, prefix = _build(orc, refs, tmp_path_factory.mktemp("edge"), "edge")
    return refs, oidx, F, prefix


def test_lrand48_draws_are_the_pac_fill(orc, edge):
    refs, oidx, F, _ = edge
    at = eu.n_positions([s for _, s in refs])
    assert len(at) == 61
    d = eu.lrand48_draws(STATE, 122)
    assert [F[p] for p in at] == ["ACGT"[x] for x in d[:61]]
    # ... and the generator's state after the build is 122 draws on
    orc.lib().orc_rng_set_state(STATE)
    for x in d:
        assert int(orc.lib().orc_lrand48()) & 3 == x
    pac, bwt = eu.both_fills([s for _, s in refs], STATE)
    assert pac == F
    # the two fills of the 60-N hole differ in at least 20 places (a random pair: 45 expected; fewer than 20 has probability < 1e-9)
    assert sum(pac[p] != bwt[p] for p in at[:60]) >= 20


@pytest.mark.parametrize("text", ["A", "A" * 300, "AC" * 200, "AT" * 100, "ACGT" * 64, None, "tandem"], ids=["A", "A300", "AC200", "AT100", "ACGT64", "63+T", "uuuU"])
def test_oracle_builder_equals_sorted_suffixes(orc, tmp_path, text):
    rng = np.random.default_rng(77)
    if text is None:
        refs = [("a", eu.rand_seq(rng, 63)), ("b", "T")]
    elif text == "tandem":
        u = eu.rand_seq(rng, 500)
        refs = [("u", u + u + u + eu.revcomp(u))]
    else:
        refs = [("x", text)]
    _, _, prefix = _build(orc, refs, tmp_path, "t")
    eu.check_against_brute_sa(prefix, "".join(s for _, s in refs))


def test_junction_reads_split_at_the_junction(orc, edge):
    refs, oidx, F, _ = edge
    lens = [len(s) for _, s in refs]
    reads = eu.edge_reads(refs, F)
    opt = orc.default_opt()
    n_j = 0
    for lab, r, e in reads:
        out = orc.align_batch(opt, oidx, [r])
        recs = eu.records(out)
        assert eu.inside_contig(out, lens), lab
        if lab.startswith("junction") or lab == "c0|one|short|hole":
            n_j += 1
            assert len(recs) >= 2, (lab, recs)
            assert not any(_m_covers_read(x, len(r)) for x in recs), (lab, recs)
        elif lab.startswith("strand boundary"):
            assert len(recs) == 2 and sorted(x["flag"] & 16 for x in recs) == [0, 16], (lab, recs)
            assert all(any((w & 0xf) in (4, 5) for w in x["cigar"]) for x in recs), (lab, recs)
        elif lab == "20 random + first 130":
            assert (recs[0]["rid"], recs[0]["pos"], orc.cigar_str(recs[0]["cigar"])) == (0, 0, "20S130M"), recs
        elif lab == "whole contig":
            assert (recs[0]["rid"], recs[0]["pos"], orc.cigar_str(recs[0]["cigar"])) == (4, 0, "150M"), recs
    assert n_j == eu.n_junction_reads(refs) + 1
    # every form of every read stays inside its contig, too
    assert eu.inside_contig(orc.align_batch(opt, oidx, eu.with_forms(reads)), lens)


def test_tiny_contigs_reads_split(orc, tmp_path):
    refs = eu.tiny300_ref()
    oidx, F, _ = _build(orc, refs, tmp_path, "tiny300")
    reads = eu.tiny300_reads(F)
    assert len(reads) >= 200
    out = orc.align_batch(orc.default_opt(), oidx, reads)
    assert eu.inside_contig(out, [len(s) for _, s in refs])
    assert int((np.diff(out["hit_off"]) >= 2).sum()) >= 200


def test_long_junction_reads_split(orc, tmp_path):
    refs = eu.long3_ref()
    lens = [len(s) for _, s in refs]
    oidx, F, _ = _build(orc, refs, tmp_path, "long3")
    base, muts = eu.long3_reads(refs)
    opt = orc.default_opt()
    for lab, r, touched in base[:6]:
        out = orc.align_batch(opt, oidx, [r])
        assert eu.inside_contig(out, lens), lab
        recs = eu.records(out)
        ends = [(x["rid"], x["pos"], x["pos"] + _reflen(x)) for x in recs]
        assert sorted(x[0] for x in ends) == sorted(touched), (lab, ends)
        if touched[0] == touched[-1]:          # the strand boundary: both records end with the contig, one on each strand
            assert all(x[2] == lens[x[0]] for x in ends) and sorted(x["flag"] & 16 for x in recs) == [0, 16], (lab, ends)
            continue
        for rid, b, e in ends:
            assert rid == touched[0] or b == 0, (lab, ends)
            assert rid == touched[-1] or e == lens[rid], (lab, ends)
    out = orc.align_batch(opt, oidx, [r for _, r, _ in base[6:] + muts])
    assert eu.inside_contig(out, lens)


def _reflen(rec):
    return sum(w >> 4 for w in rec["cigar"] if (w & 0xf) in (0, 2, 3, 7, 8))


def test_hole_reads_seed_as_the_bwt_text_says(orc, edge):
    refs, oidx, F, _ = edge
    pac, bwt = eu.both_fills([s for _, s in refs], STATE)
    hr = eu.hole_reads(refs, pac, bwt)
    lab, r_pac, r_bwt = hr[0]
    assert len(r_pac) == 150 and len(r_bwt) == 150
    n_diff = sum(a != b for a, b in zip(r_pac, r_bwt))
    assert n_diff >= 20
    opt = orc.default_opt()
    # the BWT text's fill: one interval as long as the read; 150M, AS 150, NM = the places where the pac differs
    iv = orc.stage_dump(opt, oidx, r_bwt, 0).reshape(-1, 4)
    assert any(int(a) == 0 and int(b) == 150 for a, b, _, _ in iv), iv
    rec = orc.align_sequence(opt, oidx, r_bwt)
    assert (orc.cigar_str(rec[0]["cigar"]), rec[0]["AS"], rec[0]["NM"]) == ("150M", 150, n_diff), rec
    # the pac's fill: no interval covers the hole (read positions 45 .. 105); NM 0
    iv = orc.stage_dump(opt, oidx, r_pac, 0).reshape(-1, 4)
    assert len(iv) and not any(int(a) <= 45 and int(b) >= 105 for a, b, _, _ in iv), iv
    rec = orc.align_sequence(opt, oidx, r_pac)
    assert rec[0]["NM"] == 0 and orc.cigar_str(rec[0]["cigar"]) == "150M", rec
