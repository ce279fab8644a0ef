"""The row exit of the short-read extension loops (knob ext_row_exit, counter ext_row_exits; dev_ext_wave.h "the row exit"): reg_ksw_extend2 in
k_extend_reg / k_extend_cand / k_ext_first and lane_rows_extend in k_ext_lanes / k_first_lanes end a DP after a row that rules out any change of what
their caller reads.  Every field of every record, CIGAR words included, against the CPU oracle with the knob 0 and 1, on knob settings that send the
dynamic programs to each of those kernels.  (ext_row_exits is ONE counter over all of them: `> 0` says the exit fired in the batch, not in which kernel.
Only the "walk" path has a single kernel running DPs; on the others the parity with the oracle is what holds each kernel.)
The reference is made here: about 35 kb -- a family of 70 copies of a 220 bp segment (a read from it keeps 70 one-seed chains, each extended in place
by the walk) and unique sequence.  Reads: a stretch of reference with bases the reference does not have (junk) on its left, its right or both sides;
flanks whose first third is the reference with 10 % errors and junk after that; family reads with a junk flank; reads at a contig's first and
last bases; 250 bp reads whose junk flank is longer than the band (qlen > w + 1: the exit only behind a short seed); with band 4, reads that
take mem_chain2aln's second band trial; and, with band 4, reads whose extension comes back into the band through row -1's ramp, which the exit's
precondition has to bar (with the precondition taken out of a scratch build, test_band_reentry_bars_the_exit fails)."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

FIELDS = ("hit_off", "rid", "pos", "flag", "mapq", "score", "nm", "na", "n_cigar", "cig_off", "cigar")
COMP = {"A": "T", "C": "G", "G": "C", "T": "A", "N": "N"}
COPIES = 70
# (name, knobs): which kernel runs the dynamic programs
PATHS = (("walk", (("ext_split", 0), ("heavy_seeds", 1), ("cand_top", 0), ("top_reuse", 0))),                                      # k_extend_reg, every DP in place
         ("split_lanes", (("split_min", 16), ("first_lanes", 1))),                                                                      # k_first_lanes + the walk of the heavy reads
         ("split_waves", (("split_min", 16), ("first_lanes", 0))),                                                                      # k_ext_first
         ("cand_waves", (("split_min", 1), ("heavy_seeds", 3), ("cand_seeds", 1), ("cand_lanes", 0))),                                  # k_extend_cand
         ("cand_lanes", (("split_min", 1), ("heavy_seeds", 3), ("cand_seeds", 1), ("cand_lanes", 1), ("cand_lane_seeds", 1))))          # k_ext_lanes


def revcomp(s):
    return "".join(COMP[c] for c in reversed(s))


def rand_seq(rng, n):
    return "".join("ACGT"[int(x)] for x in rng.integers(0, 4, n))


def noisy(rng, s, rate):
    """s with substitutions at the given rate and now and then a missing or an extra base"""
    out = []
    for ch in s:
        x = rng.random()
        if x < rate * 0.8:
            out.append("ACGT"[("ACGT".index(ch) + 1 + int(rng.integers(0, 3))) % 4])
        elif x < rate * 0.9:
            out += [rand_seq(rng, 1), ch]
        elif x >= rate:
            out.append(ch)
    return "".join(out)


def fit(rng, s, n):
    return (s + rand_seq(rng, n))[:n]


@pytest.fixture(scope="module")
def world(sl, orc, tmp_path_factory):
    rng = np.random.default_rng(1019)
    seg = rand_seq(rng, 220)
    fam, fam_at = [], []
    for _ in range(COPIES):
        fam.append(rand_seq(rng, int(rng.integers(40, 90))))
        fam_at.append(sum(map(len, fam)))
        fam.append(seg)
    contigs = ["".join(fam) + rand_seq(rng, 300), rand_seq(rng, 12000)]
    # what the exit's precondition is for (band 4): a seed of 64 or 70 bases, then a run of 65 A in the read where the reference has 18 other bases and
    # then its run of A.  The seed's score keeps row -1's ramp alive beyond the band, the match comes back through it, and the window (65 + 8 rows) ends
    # before the bound would let the loop go on: without the precondition the extension ends at the seed (host test, c_guard: 70 where the checker has 85)
    rng_g = np.random.default_rng(53)
    guard, blocks = [], []
    for i in range(16):
        core = rand_seq(rng_g, (64, 70)[i % 2])
        blocks.append(rand_seq(rng_g, 150) + core + "".join("GC"[int(x)] for x in rng_g.integers(0, 2, 18)) + "A" * 70 + rand_seq(rng_g, 150))
        guard.append(core + "A" * 65 if i % 4 < 2 else revcomp(core + "A" * 65))
    contigs.append("".join(blocks))
    assert 30000 < sum(map(len, contigs)) < 45000
    prefix = str(tmp_path_factory.mktemp("ext_row_exit") / "ref")
    orc.Index.build(["chrA", "chrB", "chrC"], contigs).write(prefix)
    oidx = orc.Index.load(prefix)
    idx = sl.BWAIndex()
    idx.LoadIndex(prefix)
    uni = contigs[1]
    reads = []
    for i in range(40):
        p = 300 + 280 * i
        core = int(rng.integers(50, 100))
        left = int(rng.integers(10, 150 - core - 9))
        right = 150 - core - left
        h = uni[p:p + core]
        reads.append(rand_seq(rng, 150 - core) + h)                                      # junk on the left
        reads.append(h + rand_seq(rng, 150 - core))                                      # ... on the right
        reads.append(rand_seq(rng, left) + h + rand_seq(rng, right))                     # ... on both sides
        # partly homologous flanks: a third of the flank is the reference with 10 % errors, junk after that
        third = (150 - core) // 3
        reads.append(fit(rng, h + noisy(rng, uni[p + core:p + core + third], 0.10), 150))
        lf = noisy(rng, uni[p - third:p], 0.10)
        reads.append((rand_seq(rng, 150) + lf + h)[-150:])
        reads.append(fit(rng, uni[p:p + 150 - 12] if i % 2 else noisy(rng, uni[p:p + 150], 0.02), 150))      # homologous over the whole read
    # the family: 90 .. 120 bases of the segment and junk beside them -- 70 one-seed chains, every one extended in place into the junk
    for i, at in enumerate(fam_at[:6]):
        k = 90 + 6 * i
        r = seg[20:20 + k] + rand_seq(rng, 150 - k) if i % 2 else rand_seq(rng, 150 - k) + seg[200 - k:200]
        reads.append(revcomp(r) if i in (2, 3) else r)
    # a contig's first and last bases: reads that end there, with two substitutions near that end (the window is clipped: tlen binds)
    def sub(s, *at):
        s = list(s)
        for q in at:
            s[q] = "ACGT"[("ACGT".index(s[q]) + 2) % 4]
        return "".join(s)
    reads += [sub(uni[:150], 5, 17), sub(uni[-150:], 132, 144), revcomp(sub(uni[-150:], 130, 141)), sub(contigs[0][:150], 4, 20), rand_seq(rng, 30) + uni[:120], uni[-110:] + rand_seq(rng, 40)]
    for i in range(len(reads)):
        if i % 3 == 1:
            reads[i] = revcomp(reads[i])
    assert all(len(r) == 150 for r in reads) and 200 <= len(reads) <= 400
    opt = orc.default_opt()
    kept = [int(orc.stage_dump(opt, oidx, r, 1)[0]) for r in reads[240:246]]
    assert min(kept) >= 64, kept                                                         # the family reads keep at least 64 chains
    # 250 bp: the stretch of reference at one end, 130 .. 190 junk bases beside it (longer than the band + 1: the exit only where the seed's score is small)
    long_reads = []
    for i in range(24):
        p = 400 + 450 * i
        core = (60, 70, 120)[i % 3]          # h0 = 120: the ramp of row -1 reaches past the band, no exit with a flank longer than the band either
        r = uni[p:p + core] + rand_seq(rng, 250 - core) if i % 2 else rand_seq(rng, 250 - core) + uni[p:p + core]
        long_reads.append(revcomp(r) if i % 4 >= 2 else r)
    # band 4: four bases the read lacks, 40 bp and 8 bp before the read's end (the second trial runs with band 8)
    opt4 = orc.default_opt()
    opt4.w = 4
    band = []
    for i in range(30):
        p = 500 + 370 * i
        wdw = uni[p:p + 160]
        band += [wdw[:110] + wdw[114:154], wdw[:142] + wdw[146:154], rand_seq(rng, 60) + wdw[:90]]
    regs = [orc.stage_dump(opt4, oidx, r, 2).reshape(-1, 10) for r in band[0::3]]
    assert sum(len(g) >= 1 and g[0][7] == 8 for g in regs) >= 10                         # ... says the checker's region: found with band 8
    gained = 0
    for r in guard:
        g = orc.stage_dump(opt4, oidx, r, 2).reshape(-1, 10)          # rb re qb qe rid score truesc w seedcov seedlen0
        gained += any(x[9] in (64, 70) and x[5] > x[9] + 5 for x in g)
    assert gained >= 12, gained          # the checker's extension of the seed went on through the run of A (a region that scores well above its seed)
    return {"guard": guard, "exp_guard": orc.align_batch(opt4, oidx, guard), "idx": idx, "reads": reads, "exp": orc.align_batch(opt, oidx, reads), "long": long_reads, "exp_long": orc.align_batch(opt, oidx, long_reads),
            "band": band, "exp_band": orc.align_batch(opt4, oidx, band)}


def same(got, exp, what):
    for k in FIELDS:
        assert np.array_equal(got[k], exp[k]), "%s: field %s differs" % (what, k)


def run(sl, world, knobs, row_exit, seqs, band=None):
    al = sl.BWAAligner(world["idx"])
    for key, val in knobs:
        al.set(key, val)
    al.set("ext_row_exit", row_exit)
    if band:
        al.SetBandwidth(band)
    got = al.alignSequences(seqs)
    return got, al.counter("ext_row_exits")


@pytest.mark.parametrize("path", PATHS, ids=[p[0] for p in PATHS])
def test_oracle_with_and_without_the_exit(sl, world, path):
    name, knobs = path
    got = {}
    for row_exit in (0, 1):
        got[row_exit], exits = run(sl, world, knobs, row_exit, world["reads"])
        what = "%s ext_row_exit=%d" % (name, row_exit)
        print("%s: ext_row_exits %d" % (what, exits))
        same(got[row_exit], world["exp"], what)
        assert (exits > 0) if row_exit else (exits == 0), what
    same(got[1], got[0], name + ": the two knob settings")


@pytest.mark.parametrize("path", (PATHS[0], PATHS[1], PATHS[4]), ids=[PATHS[0][0], PATHS[1][0], PATHS[4][0]])
def test_longer_reads(sl, world, path):
    """250 bp reads with 130 .. 190 junk bases on one side: a query longer than the band + 1"""
    name, knobs = path
    got = {}
    for row_exit in (0, 1):
        got[row_exit], exits = run(sl, world, knobs, row_exit, world["long"])
        print("%s 250 bp ext_row_exit=%d: ext_row_exits %d" % (name, row_exit, exits))
        same(got[row_exit], world["exp_long"], "%s 250 bp ext_row_exit=%d" % (name, row_exit))
        assert row_exit or exits == 0
    same(got[1], got[0], name + " 250 bp: the two knob settings")


@pytest.mark.parametrize("path", (PATHS[0], PATHS[1], PATHS[2]), ids=[PATHS[0][0], PATHS[1][0], PATHS[2][0]])
def test_second_band_trial(sl, world, path):
    name, knobs = path
    got = {}
    for row_exit in (0, 1):
        got[row_exit], exits = run(sl, world, knobs, row_exit, world["band"], band=4)
        print("%s w=4 ext_row_exit=%d: ext_row_exits %d" % (name, row_exit, exits))
        same(got[row_exit], world["exp_band"], "%s w=4 ext_row_exit=%d" % (name, row_exit))
        assert row_exit or exits == 0
    same(got[1], got[0], name + " w=4: the two knob settings")


@pytest.mark.parametrize("path", PATHS, ids=[p[0] for p in PATHS])
def test_band_reentry_bars_the_exit(sl, world, path):
    """band 4, a seed of 64 or 70 bases and a query longer than the band: the exit's precondition says no (row -1's ramp is alive beyond the band), and has to"""
    name, knobs = path
    got = {}
    for row_exit in (0, 1):
        got[row_exit], exits = run(sl, world, knobs, row_exit, world["guard"], band=4)
        print("%s guard reads ext_row_exit=%d: ext_row_exits %d" % (name, row_exit, exits))
        same(got[row_exit], world["exp_guard"], "%s guard reads ext_row_exit=%d" % (name, row_exit))
        assert row_exit or exits == 0
    same(got[1], got[0], name + " guard reads: the two knob settings")
