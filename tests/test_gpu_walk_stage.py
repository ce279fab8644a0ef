"""The staged extension walk (k_extend_reg with walk_stage = 1): chain headers made 64 at a time, one per lane (dev_chain_hdr.h; 16 at a time
for reads of 321 .. 704 bp), one-seed chains walked from their header alone, and the covered test's keys of a read's first 128 regions in LDS
(64 for reads of 161 .. 320 bp; later regions and the 704-column form keep them in HBM).  Every field of every record, CIGAR words
included, against the CPU oracle for walk_stage 0 and 1.
The reference is made here: three contigs, about 200 kb of random sequence with families of 63 / 64 / 65 / 128 / 129 exact copies of a 220 bp
segment (a read from a family keeps that many one-seed chains and as many regions: both sides of the 64- and 128-region edges), diverged
copies of longer segments (chains of several seeds, with a deleted base on two diagonals) and period-1 to period-6 tracts (reads with hundreds
of seed occurrences and regions).  Reads from all of them and from unique sequence, both strands, a 40 bp read and a read with an N among the
150 bp ones; 250 bp and 330 bp reads of the same places for the other two short-read forms of the kernel."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

FIELDS = ("hit_off", "rid", "pos", "flag", "mapq", "score", "nm", "na", "n_cigar", "cig_off", "cigar")
FAMILIES = (63, 64, 65, 128, 129)
CHAIN_COUNTS = (1,) + FAMILIES
SIZES = (1, 63, 64, 65, 2000)
COMP = {"A": "T", "C": "G", "G": "C", "T": "A", "N": "N"}


def revcomp(s):
    return "".join(COMP[c] for c in reversed(s))


def rand_seq(rng, n):
    return "".join("ACGT"[int(x)] for x in rng.integers(0, 4, n))


def make_reference(rng):
    """-> (names, contigs, sites): sites[kind] = list of (contig, position) from which reads are drawn"""
    sites = {"unique": [], "tract": [], "tract_edge": [], "copy": [], "family": {k: [] for k in FAMILIES}}
    parts = [[], [], []]          # pieces of the three contigs
    pos = [0, 0, 0]

    def put(c, s):
        at = pos[c]
        parts[c].append(s)
        pos[c] += len(s)
        return at
    # contig 0: the families, copies separated by random spacers (each copy starts a fresh diagonal)
    for k in FAMILIES:
        seg = rand_seq(rng, 220)
        for i in range(k):
            put(0, rand_seq(rng, int(rng.integers(40, 90))))
            at = put(0, seg)
            if i in (0, k // 2, k - 1):
                sites["family"][k].append((0, at))
    put(0, rand_seq(rng, 300))
    # contig 1 (short): unique sequence and a few tracts, so that windows are clipped at both of its ends
    put(1, rand_seq(rng, 700))
    for unit in ("A", "AC", "GTT"):
        at = put(1, unit * (240 // len(unit)))
        sites["tract"].append((1, at + 30))
        sites["tract_edge"].append((1, at - 75))
        put(1, rand_seq(rng, 400))
    # contig 2: tracts of every period many times, diverged copies, unique sequence
    units = ("T", "AG", "CAT", "GATA", "GTTAT", "CCTGAA")
    for rep in range(9):
        for unit in units:
            put(2, rand_seq(rng, int(rng.integers(300, 700))))
            n = int(rng.integers(170, 330))
            at = put(2, (unit * (n // len(unit) + 1))[:n])
            if rep < 3:
                sites["tract"].append((2, at + int(rng.integers(0, 15))))
                sites["tract_edge"].append((2, at - int(rng.integers(40, 110))))
                sites["tract_edge"].append((2, at + n - int(rng.integers(40, 110))))
    for _ in range(6):
        seg = rand_seq(rng, 400)
        for i in range(5):
            put(2, rand_seq(rng, 200))
            s = list(seg)
            for _ in range(6 * i):                                  # copy i: 6 i substitutions and, from the second on, a deleted base
                s[int(rng.integers(0, len(s)))] = "ACGT"[int(rng.integers(0, 4))]
            if i:
                del s[int(rng.integers(150, 250))]
            at = put(2, "".join(s))
            sites["copy"].append((2, at + int(rng.integers(60, 190))))
    while pos[2] < 60000:
        at = put(2, rand_seq(rng, 2000))
        sites["unique"].append((2, at + 100))
    contigs = ["".join(p) for p in parts]
    sites["unique"] += [(0, len(contigs[0]) - 150), (1, 0), (1, 5), (2, 0), (2, len(contigs[2]) - 150)]      # the contigs' first and last bases
    return ["chrA", "chrB", "chrC"], contigs, sites


def chain_sizes(orc, opt, oidx, seq):
    """seeds per kept chain, from the oracle's chain stage"""
    d = orc.stage_dump(opt, oidx, seq, 1)
    n, at, out = int(d[0]), 1, []
    for _ in range(n):
        k = int(d[at + 2])
        out.append(k)
        at += 3 + 4 * k
    return out


@pytest.fixture(scope="module")
def world(sl, orc, tmp_path_factory):
    rng = np.random.default_rng(2024)
    names, contigs, sites = make_reference(rng)
    assert 150000 < sum(map(len, contigs)) < 260000
    prefix = str(tmp_path_factory.mktemp("walk_stage") / "ref")
    orc.Index.build(names, contigs).write(prefix)
    oidx = orc.Index.load(prefix)
    idx = sl.BWAIndex()
    idx.LoadIndex(prefix)
    opt = orc.default_opt()

    def read(c, p, n=150):
        p = max(0, min(p, len(contigs[c]) - n))
        return contigs[c][p:p + n]
    # the reads the shape checks need come first, so that the smallest batches hold them
    head, counts, most_seeds = [], {}, 0
    for k in FAMILIES:
        for i, (c, p) in enumerate(sites["family"][k]):
            r = read(c, p + 20 + 7 * i)
            head.append(revcomp(r) if i == 1 else r)
    head.append(read(*sites["unique"][0]))
    head.append(read(*sites["unique"][1])[:40])                                     # a 40 bp read among the 150 bp ones
    withn = list(read(*sites["copy"][0]))
    withn[70] = "N"
    head.append("".join(withn))                                                      # a read with an N
    body = []
    for kind in ("tract", "tract_edge", "copy", "unique"):
        for i, (c, p) in enumerate(sites[kind]):
            r = read(c, p)
            body += [r, revcomp(r)] if i % 2 else [revcomp(r), r]
    seqs = head + body
    # the oracle's chains: the batch edges occur, chains of several seeds occur, and (if the reference yields one) a chain of more than 64 seeds
    multi, regions = 0, set()
    for s in seqs:
        regions.add(len(orc.stage_dump(opt, oidx, s, 2)) // 10)
        cs = chain_sizes(orc, opt, oidx, s)
        counts[len(cs)] = counts.get(len(cs), 0) + 1
        multi += sum(1 for k in cs if 2 <= k <= 8)
        most_seeds = max([most_seeds] + cs)
    missing = [k for k in CHAIN_COUNTS if k not in counts]
    assert not missing, "no read keeps %r chains (kept-chain counts seen: %r)" % (missing, sorted(counts))
    assert multi > 0 and max(counts) > 129
    assert {127, 128, 129} & regions and any(x <= 128 for x in regions) and any(x > 128 for x in regions), sorted(regions)      # the 128-region edge
    if most_seeds <= 64:
        print("walk_stage: the case 'a chain of more than 64 seeds' is missing (the longest chain has %d)" % most_seeds)
    fill = [read(2, int(p)) for p in rng.integers(0, len(contigs[2]) - 150, 2000)]
    seqs = (seqs + fill)[:2000]
    assert len(seqs) == 2000 and len(head) + len(body) <= 2000
    exp = {n: orc.align_batch(opt, oidx, seqs[:n]) for n in SIZES}
    # the other two forms of the kernel: reads of 250 bp (headers 64 at a time, 64 region keys in LDS) and of 330 bp (headers 16 at a time, no keys
    # in LDS).  A family's 220 bp segment with bases the reference does not have before or after it (and an N between them) keeps the family's chains, as many regions
    longer = {}
    for n in (250, 330):
        rs = []
        for k in FAMILIES:
            for i, (c, p) in enumerate(sites["family"][k]):
                junk = rand_seq(rng, n - 221)          # behind an N, so that no copy's own flank lengthens the match
                r = junk + "N" + read(c, p, 220) if i == 2 else read(c, p, 220) + "N" + junk
                rs.append(revcomp(r) if i == 1 else r)
        for kind in ("tract", "tract_edge", "copy", "unique"):
            for i, (c, p) in enumerate(sites[kind][:10]):
                r = read(c, p - 40, n)
                rs.append(revcomp(r) if i % 2 else r)
        regions = [len(orc.stage_dump(opt, oidx, r, 2)) // 10 for r in rs]
        assert set(FAMILIES) <= set(len(chain_sizes(orc, opt, oidx, r)) for r in rs[:15])          # the edges of the 16- and 64-chain batches
        assert {63, 64, 65} <= set(regions), regions                                                # both sides of the 64-region edge
        longer[n] = (rs, orc.align_batch(opt, oidx, rs))
    return {"idx": idx, "seqs": seqs, "exp": exp, "most_seeds": most_seeds, "longer": longer}


def same(got, exp, what):
    for k in FIELDS:
        assert np.array_equal(got[k], exp[k]), "%s: field %s differs" % (what, k)


@pytest.mark.parametrize("walk_stage", (0, 1))
@pytest.mark.parametrize("top_reuse,cand_top", ((1, 2), (0, 2), (1, 0)))
def test_oracle_by_batch_size(sl, world, walk_stage, top_reuse, cand_top):
    """ext_split 0 sends every read through k_extend_reg; heavy_seeds 1 makes every read heavy; a small cand_top gives the first reads of the
    heaviest-first list regions extended ahead of time (have_cand), so that both ways to a region meet in one batch of chains"""
    al = sl.BWAAligner(world["idx"])
    for key, val in (("ext_split", 0), ("heavy_seeds", 1), ("top_reuse", top_reuse), ("cand_top", cand_top), ("walk_stage", walk_stage)):
        al.set(key, val)
    for n in SIZES:
        what = "walk_stage=%d top_reuse=%d cand_top=%d n=%d" % (walk_stage, top_reuse, cand_top, n)
        al.ordinal = 0
        same(al.alignSequences(world["seqs"][:n]), world["exp"][n], what)
        staged = al.counter("walk_staged_chains")
        print("%s: walk_staged_chains %d" % (what, staged))
        assert (staged > 0) if walk_stage else (staged == 0), what
    assert al.counter("guard_dirty") == 0 and al.counter("retries") == 0


@pytest.mark.parametrize("walk_stage", (0, 1))
def test_default_path(sl, world, walk_stage):
    """the split extension as large chunks run it: k_extend_reg gets the heavy reads and the light reads k_ext_replay gives up"""
    al = sl.BWAAligner(world["idx"])
    al.set("split_min", 16)
    al.set("walk_stage", walk_stage)
    same(al.alignSequences(world["seqs"]), world["exp"][2000], "split extension, walk_stage=%d" % walk_stage)
    staged = al.counter("walk_staged_chains")
    assert (staged > 0) if walk_stage else (staged == 0)


@pytest.mark.parametrize("walk_stage", (0, 1))
@pytest.mark.parametrize("length", (250, 330))
def test_longer_reads(sl, world, walk_stage, length):
    """k_extend_reg<320> (64 region keys in LDS) and <704> (headers 16 at a time, no keys in LDS): reads of 250 and of 330 bp, every read through the walk"""
    seqs, exp = world["longer"][length]
    al = sl.BWAAligner(world["idx"])
    for key, val in (("ext_split", 0), ("heavy_seeds", 1), ("walk_stage", walk_stage)):
        al.set(key, val)
    same(al.alignSequences(seqs), exp, "%d bp reads, walk_stage=%d" % (length, walk_stage))
    staged = al.counter("walk_staged_chains")
    assert (staged > 0) if walk_stage else (staged == 0)
