"""k_first_lanes (dev_ext_lane.h): the light reads' top-seed extensions that need the dynamic program, one lane per job, both sides of the seed in
one row loop (dev_lane_rows.h).  Every field of every record, CIGAR words included, against the CPU oracle, for first_lanes 0 / 1 (0 = one wave
per job, k_ext_first) and lane_narrow 0 / 1, on the fixture reads plus 150 bp reference windows edited so that each kind of job occurs: bases to extend only to
the right of the seed, only to the left, on both sides; a 5 bp and a 4 bp deletion under a 4-column band (the 4 bp one stays inside one chain and
takes the second band trial); a 40 bp read beside 150 bp ones; error-free reads only (no job at all)."""
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

FIELDS = ("hit_off", "rid", "pos", "flag", "mapq", "score", "nm", "na", "n_cigar", "cig_off", "cigar")
SIZES = (16, 63, 64, 65, 129, 513, 3000)
COMBOS = [(fl, nar) for fl in (0, 1) for nar in (0, 1)]
N_WINDOWS = 60


def same(got, exp, what):
    for k in FIELDS:
        assert np.array_equal(got[k], exp[k]), "%s: field %s differs" % (what, k)


def sub(s, *at):
    s = list(s)
    for p in at:
        s[p] = "ACGT"[("ACGT".index(s[p]) + 1 + p % 3) % 4]
    return "".join(s)


def windows(refs):
    """150 bp of reference (and the 5 bases after them), plain ACGT, spread over the second contig"""
    out, ref, p = [], refs[1].upper(), 1000
    while len(out) < N_WINDOWS:
        w = ref[p:p + 155]
        if len(w) == 155 and set(w) <= set("ACGT"):
            out.append(w)
        p += 997
    return out


def kinds(w):
    return [sub(w[:150], 125, 140),                  # two substitutions 15 bp apart near the right end: a right-only job
            sub(w[:150], 9, 24),                     # the mirror image: a left-only job
            sub(w[:150], 9, 24, 125, 140),           # both in one read
            w[:110] + w[115:155],                    # the reference has 5 bases the read lacks, 40 bp before the read's end
            del4(w)]


def del4(w):
    """... 4 bases: with band 4 the two parts still chain (a gap of at most w), the top seed's right extension meets the gap at the band's edge
    (max_off 4 >= 3/4 w) and mem_chain2aln tries it again with band 8"""
    return w[:110] + w[114:154]


@pytest.fixture(scope="module")
def pool(orc, tiny_index, sim_reads, golden_dir):
    _, refs = orc.read_fasta(os.path.join(golden_dir, "tiny.fa"))
    (_, s1), _ = sim_reads
    ws = windows(refs)
    head = kinds(ws[0]) + [s1[0][:40], s1[1]] + kinds(ws[1])          # the first 16 reads hold every kind, a 40 bp read and 150 bp reads
    edited = [r for w in ws[2:] for r in kinds(w)]
    seqs = head + list(s1[2:6]) + edited
    seqs = seqs + list(s1[6:6 + 3000 - len(seqs)])
    assert len(seqs) == 3000 and len(head) + 4 == 16
    opt = orc.default_opt()
    opt4 = orc.default_opt()
    opt4.w = 4
    d4 = set(del4(w) for w in ws)
    # band 4: the checker's regions say that the 4 bp deletions took the second band trial -- one region over the whole read, found with band 8
    doubled = 0
    for sq in seqs[:513]:
        if sq in d4:
            regs = orc.stage_dump(opt4, tiny_index, sq, 2).reshape(-1, 10)          # rb re qb qe rid score truesc w seedcov seedlen0
            doubled += len(regs) >= 1 and tuple(regs[0][2:4]) == (0, 150) and regs[0][7] == 8
    assert doubled >= 30, doubled
    # error-free reads only -- those of them for which the checker runs no extension at all (a window inside a repeat keeps chains whose seeds end early)
    def cells(sq):
        a = orc.counters()["ext_cells"]
        orc.align_batch(opt, tiny_index, [sq])
        return orc.counters()["ext_cells"] - a
    clean = [w[:150] for w in ws if cells(w[:150]) == 0]
    assert len(clean) >= 20
    clean = clean * 14
    return {"seqs": seqs, "exp": {n: orc.align_batch(opt, tiny_index, seqs[:n]) for n in SIZES}, "exp_w4": orc.align_batch(opt4, tiny_index, seqs[:513]),
            "clean": clean, "exp_clean": orc.align_batch(opt, tiny_index, clean)}


def aligner(sl, tiny_gpu, first_lanes, narrow):
    al = sl.BWAAligner(tiny_gpu)
    al.set("split_min", 16)          # light / heavy partition and the split extension, as for large chunks
    al.set("first_lanes", first_lanes)
    al.set("lane_narrow", narrow)
    return al


def check_counters(al, first_lanes, what):
    jobs = al.counter("first_lane_jobs")
    print("%s: first_lane_jobs %d" % (what, jobs))
    assert (jobs > 0) if first_lanes else (jobs == 0), what


@pytest.mark.parametrize("first_lanes,narrow", COMBOS)
def test_oracle_by_batch_size(sl, tiny_gpu, pool, first_lanes, narrow):
    al = aligner(sl, tiny_gpu, first_lanes, narrow)
    for n in SIZES:
        what = "first_lanes=%d lane_narrow=%d n=%d" % (first_lanes, narrow, n)
        al.ordinal = 0
        same(al.alignSequences(pool["seqs"][:n]), pool["exp"][n], what)
        check_counters(al, first_lanes, what)


@pytest.mark.parametrize("first_lanes,narrow", COMBOS)
def test_second_band_trial(sl, tiny_gpu, pool, first_lanes, narrow):
    """band 4: the reads with the 4 bp deletion take mem_chain2aln's second trial, twice the band (the fixture checks that in the oracle's regions);
    those with the 5 bp deletion split into two regions"""
    al = aligner(sl, tiny_gpu, first_lanes, narrow)
    al.SetBandwidth(4)
    what = "w=4 first_lanes=%d lane_narrow=%d" % (first_lanes, narrow)
    same(al.alignSequences(pool["seqs"][:513]), pool["exp_w4"], what)
    check_counters(al, first_lanes, what)


@pytest.mark.parametrize("first_lanes,narrow", COMBOS)
def test_error_free_reads_leave_no_job(sl, tiny_gpu, pool, first_lanes, narrow):
    al = aligner(sl, tiny_gpu, first_lanes, narrow)
    same(al.alignSequences(pool["clean"]), pool["exp_clean"], "error-free reads, first_lanes=%d lane_narrow=%d" % (first_lanes, narrow))
    assert al.counter("first_lane_jobs") == 0
    assert len(pool["exp_clean"]["rid"]) >= len(pool["clean"])
