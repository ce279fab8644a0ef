"""The narrow band of the light reads' top-seed extensions (knob ext_narrow, counters ext_narrow_sides / ext_narrow_jobs; dev_ext_wave.h "the narrow band"):
k_first_diag measures what a flank's main diagonal loses, k_first_lanes runs the flank in the band that loss allows, and the jobs whose sides all have such a
band run on rows of 32 columns in a launch of their own.  Every field of every record, CIGAR words included, against the CPU oracle with the knob 0, 1, 2 and 3
(2 = the band without the separate launch, 3 = that launch with the other binning key), and with 16-bit cells (lane_narrow 0: no ring).
The reference is made here: a unique contig of 36 kb and a contig of blocks with a periodic stretch (period 1 .. 6) between unique sequence.  The reads are
150 bp windows of it, edited: two, three and four substitutions on one flank and on both; substitutions next to the seed and at the read's last base; a loss at
the cap (20: four substitutions, or two and five N) and just above (21: three and three N; 25); an N in a flank; flanks with an insertion or a deletion; a
seed at the read's start (no left side); 19-base seeds between substitutions (h0 = 19 <= L); a narrow side beside a wide one, either way round; periodic
flanks; and batches that hold exactly 1, 63, 64 and 65 narrow jobs among reads that leave no job."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

FIELDS = ("hit_off", "rid", "pos", "flag", "mapq", "score", "nm", "na", "n_cigar", "cig_off", "cigar")
COMP = {"A": "T", "C": "G", "G": "C", "T": "A", "N": "N"}
SETTINGS = ((0, 1), (1, 1), (2, 1), (3, 1), (1, 0), (0, 0))          # (ext_narrow, lane_narrow); 2 = the band without the launch, 3 = the launch binned as the wide one


def revcomp(s):
    return "".join(COMP[c] for c in reversed(s))


def rand_seq(rng, n):
    return "".join("ACGT"[int(x)] for x in rng.integers(0, 4, n))


def sub(s, *at):
    s = list(s)
    for p in at:
        s[p] = "ACGT"[("ACGT".index(s[p]) + 1 + p % 3) % 4]
    return "".join(s)


def with_n(s, *at):
    s = list(s)
    for p in at:
        s[p] = "N"
    return "".join(s)


def one_flank(w, k):
    """a seed of 100 bases at the read's start (no left side), then k substitutions in the 50 bases to its right: L = 5 k"""
    return sub(w[:150], *(100, 112, 124, 136, 143, 147)[:k])


@pytest.fixture(scope="module")
def world(sl, orc, tmp_path_factory):
    rng = np.random.default_rng(2061)
    uni = rand_seq(rng, 36000)
    blocks = []
    for i in range(24):
        unit = rand_seq(rng, 1 + i % 6)
        while len(set(unit)) < min(2, len(unit)):
            unit = rand_seq(rng, 1 + i % 6)
        blocks.append(rand_seq(rng, 130) + (unit * 70)[:70] + rand_seq(rng, 130))
    contigs = [uni, "".join(blocks)]
    prefix = str(tmp_path_factory.mktemp("ext_narrow") / "ref")
    orc.Index.build(["chrA", "chrP"], contigs).write(prefix)
    oidx = orc.Index.load(prefix)
    idx = sl.BWAIndex()
    idx.LoadIndex(prefix)
    win = lambda i: uni[300 + 160 * i:300 + 160 * i + 156]
    reads = []
    for i in range(12):
        w = win(i)
        for k in (2, 3, 4):
            reads.append(one_flank(w, k))                                   # two, three, four substitutions to the right of the seed (L = 10, 15, 20 = the cap)
            reads.append(revcomp(one_flank(w, k)))
            reads.append(sub(w[:150], *(49, 37, 25, 13)[:k]))               # ... to its left
        reads.append(sub(w[:150], 20, 35, 110, 125))                        # two on either side
        reads.append(sub(w[:150], 8, 20, 35, 110, 125, 140))                # three on either side
        reads.append(sub(w[:150], 100, 101))                                # next to the seed, next to each other
        reads.append(sub(w[:150], 49, 48))
        reads.append(sub(w[:150], 120, 149))                                # the read's last base
        reads.append(sub(w[:150], 0, 30))                                   # ... and its first
        reads.append(with_n(sub(w[:150], 112, 136), 104, 108, 118, 128, 141))          # L = 20 with N: the cap
        reads.append(with_n(sub(w[:150], 112, 124, 136), 104, 118, 141))    # L = 21: just above
        reads.append(one_flank(w, 5))                                       # L = 25
        reads.append(with_n(sub(w[:150], 112), 130))                        # an N in the flank: L = 7
        reads.append(with_n(w[:150], 120, 121, 122, 123))                   # four N: L = 8
        reads.append(w[:110] + w[115:155])                                  # the reference has 5 bases the read lacks
        reads.append(w[:120] + "ACG" + w[120:147])                          # the read has 3 the reference lacks
        reads.append(sub(w[:30] + w[32:152], 60, 75))                       # ... a gap to the left of the seed, substitutions in it
        reads.append(sub(w[:150], *range(19, 150, 20)))                     # 19-base seeds between substitutions: h0 = 19, L >= 15 on the longer sides
        reads.append(sub(w[:150], 19, 39, 59, 79, 99, 119))                 # ... and a 30-base seed at the end
        reads.append(sub(w[:150], 20, 35, 105, 111, 118, 126, 133, 141))    # a narrow left side, a wide right side (L = 30)
        reads.append(sub(w[:150], 5, 12, 19, 26, 33, 41, 110, 125))         # the reverse
        reads.append(sub(w[:40] + w[43:153], 110, 125))                     # a deletion on the left, a narrow right side
        reads.append(sub(w[:150], 30, 31, 32))                              # L = 15 in three adjacent bases
    # periodic flanks: the seed in the unique sequence before (after) the periodic stretch, substitutions inside the stretch
    for i, b in enumerate(blocks):
        at = sum(map(len, blocks[:i]))
        assert contigs[1][at:at + len(b)] == b
        reads.append(sub(b[30:180], 112, 131))              # block[130:200] is periodic: the read's bases 100 .. 170
        reads.append(sub(b[30:180], 105, 118, 127, 139))
        reads.append(revcomp(sub(b[150:300], 12, 33)))      # the periodic stretch on the left
        reads.append(sub(b[150:300], 9, 21, 40))
    for i in range(len(reads)):
        if i % 5 == 3:
            reads[i] = revcomp(reads[i])
    assert 300 <= len(reads) <= 600
    opt = orc.default_opt()
    assert (opt.o_del, opt.e_del, opt.o_ins, opt.e_ins, opt.a, opt.b, opt.w, opt.zdrop) == (6, 1, 6, 1, 1, 4, 100, 100)
    # batches with exactly n narrow jobs: reads with one chain and two substitutions right of a 100-base seed (one job, its only side narrow), among error-free
    # reads, which leave no job.  The checker says that each of these reads keeps exactly one chain
    one_job = [one_flank(win(100 + i), 2) for i in range(65)]
    clean = [win(170 + i)[:150] for i in range(40)]
    for r in one_job + clean:
        assert int(orc.stage_dump(opt, oidx, r, 1)[0]) == 1
    counted = {}
    for n in (1, 63, 64, 65):
        seqs = clean[:20] + one_job[:n] + clean[20:]
        counted[n] = (seqs, orc.align_batch(opt, oidx, seqs))
    return {"idx": idx, "reads": reads, "exp": orc.align_batch(opt, oidx, reads), "counted": counted}


def same(got, exp, what):
    for k in FIELDS:
        assert np.array_equal(got[k], exp[k]), "%s: field %s differs" % (what, k)


def run(sl, world, narrow, lane_narrow, seqs):
    al = sl.BWAAligner(world["idx"])
    al.set("split_min", 16)          # light / heavy partition and the split extension, as for large chunks
    al.set("ext_narrow", narrow)
    al.set("lane_narrow", lane_narrow)
    got = al.alignSequences(seqs)
    return got, {k: al.counter(k) for k in ("ext_narrow_sides", "ext_narrow_jobs", "first_lane_jobs")}


def test_oracle_with_and_without_the_band(sl, world):
    got, cnt = {}, {}
    for s in SETTINGS:
        what = "ext_narrow=%d lane_narrow=%d" % s
        got[s], cnt[s] = run(sl, world, s[0], s[1], world["reads"])
        print(what, cnt[s])
        same(got[s], world["exp"], what)
        if s[0]:
            assert cnt[s]["ext_narrow_sides"] >= 150 and cnt[s]["ext_narrow_jobs"] >= 100, what          # (12 windows x ~20 narrow kinds, and the periodic ones)
            assert cnt[s]["ext_narrow_jobs"] < cnt[s]["first_lane_jobs"], what                            # some jobs stay wide
        else:
            assert cnt[s]["ext_narrow_sides"] == 0 and cnt[s]["ext_narrow_jobs"] == 0, what
        assert cnt[s]["first_lane_jobs"] == cnt[SETTINGS[0]]["first_lane_jobs"] > 0, what                 # the same jobs run, whichever launch takes them
        same(got[s], got[SETTINGS[0]], what + " and the knob off")
    assert cnt[(1, 1)]["ext_narrow_sides"] == cnt[(2, 1)]["ext_narrow_sides"] == cnt[(3, 1)]["ext_narrow_sides"] == cnt[(1, 0)]["ext_narrow_sides"]


@pytest.mark.parametrize("n", (1, 63, 64, 65))
def test_counted_narrow_jobs(sl, world, n):
    """exactly n narrow jobs in the batch: one wave less one lane, a full wave, a wave and one lane"""
    seqs, exp = world["counted"][n]
    for narrow in (1, 0):
        got, cnt = run(sl, world, narrow, 1, seqs)
        what = "n=%d ext_narrow=%d %r" % (n, narrow, cnt)
        same(got, exp, what)
        assert cnt["first_lane_jobs"] == n, what
        assert (cnt["ext_narrow_jobs"], cnt["ext_narrow_sides"]) == ((n, n) if narrow else (0, 0)), what
