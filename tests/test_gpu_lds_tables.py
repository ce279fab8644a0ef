"""The wave kernels whose tables live in LDS -- k_regs_wave (region sorts, de-duplication, marking: dev_fin.h) and k_chain_coop (heavy-read chaining:
dev_chain_coop.h) -- address those tables through LDS-typed pointers and the columns in HBM through global ones (dev_as.h).  A typed layout that is
wrong reads the wrong table, so every table and every aliased stretch of one is driven here, bit for bit against the oracle:

  * reads inside ONE dispersed repeat family: ~500 chains and regions, the 768-chain and the 640-region table; some of them with a stretch of
    unique sequence whose two halves mem_patch_reg tries to join (the event path of the de-duplication scan);
  * reads made of half a copy of family A's element and half of family B's: more than 768 chains and more than 640 regions, so
    k_chain_coop<.., 4096, true> and k_regs_wave<.., 2048> (whose sorts run serially on one lane by the m > 768 rule);
  * reads from a tandem tract of period 5: equal region ends (the tie fall-back of the first sort), chains that share a position past the ninth
    chain (the chain set goes on as the kbtree), neighbouring shifted regions (de-duplication events, mem_patch_reg's pre-tests and alignment);
  * unique reads in between, so that lists and queues are not homogeneous;
  * a second reference with ALT contigs that carry copies of family A: the staged two-round marking, whose l_alt / l_par live in the halves of
    m_rb and whose l_rank lives in k64.

That the reads reach those paths is asserted, not assumed: on the GPU through the keep_stages hook's snapshot of the regions before de-duplication,
and for the chains through the oracle's n_chains counter on single-read calls."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

KEYS = ("hit_off", "rid", "pos", "flag", "mapq", "score", "nm", "na", "n_cigar", "cigar")
# A copy only gives the read a seed where it matches EXACTLY: a supermaximal match hides every shorter one it contains, so the copies that
# differ from the read inside the element add next to nothing.  At 1-2 % divergence a third of the 75 bp copies carry no difference at all;
# 1 800 copies per family leave ~600 such copies, above bwa's max_occ of 500: the element's seed is sampled down to 500 occurrences.
N_COPIES = 1800
ELEM = 75
REGS_MID_N, COOP_N1 = 640, 768          # dev_fin2.h, slx_chunk.inc


def _same(got, exp, what):
    for k in KEYS:
        assert np.array_equal(got[k], exp[k]), "%s: %s differs from the oracle" % (what, k)


def _diverged(rng, e, rate):
    e = e.copy()
    m = rng.random(len(e)) < rate
    e[m] = (e[m] + rng.integers(1, 4, size=int(m.sum()), dtype=np.uint8)) & 3
    return e


def _build(tmp, with_alt):
    from oracle import orc
    from seqlib_amd import synth
    rng = np.random.default_rng(20251)
    code = {65: 0, 67: 1, 71: 2, 84: 3}
    g = synth.make_genome(460000, seed=611).copy()
    A = rng.integers(0, 4, size=ELEM, dtype=np.uint8)
    B = rng.integers(0, 4, size=ELEM, dtype=np.uint8)
    # The base on either side of a copy is an A, and neither element begins or ends with one, nor does what a read puts next to an element: no
    # occurrence can be extended past the element, so the element itself is the supermaximal match and keeps all its occurrences (a random
    # flank would match a quarter of the copies one base further, a sixteenth two bases, ... and leave a staircase of seeds with few occurrences).
    for e in (A, B):
        e[0] = 1 + e[0] % 3; e[-1] = 1 + e[-1] % 3

    def place(h, p, e):
        h[p:p + ELEM] = e; h[p - 1] = 0; h[p + ELEM] = 0
    # unlinked loci: one slot of 120 bp per copy, the families interleaved at random; the tandem tract and its surroundings stay free
    slots = [s for s in range(2000, 458000, 120) if not 248000 <= s <= 252000]
    pick = rng.choice(len(slots), size=2 * N_COPIES, replace=False)
    for n, si in enumerate(pick):
        place(g, slots[si] + 1 + int(rng.integers(0, 40)), _diverged(rng, A if n < N_COPIES else B, rng.uniform(0.01, 0.02)))
    g[250000:250600] = np.array([code[c] for c in b"GTTAT" * 120], dtype=np.uint8)          # the tandem tract of test_gpu_parity
    refs = [("chrS", g)]
    if with_alt:
        for name, length, n_cp, seed in (("alt_a", 30000, 150, 612), ("alt_b", 20000, 100, 613)):
            h = synth.make_genome(length, seed=seed).copy()
            for p in np.sort(rng.choice(np.arange(500, length - 500, 150), size=n_cp, replace=False)):
                place(h, int(p), _diverged(rng, A, rng.uniform(0.01, 0.02)))
            refs.append((name, h))
    prefix = str(tmp / ("ldsalt" if with_alt else "lds"))
    orc.Index.build([n for n, _ in refs], [synth.genome_ascii(h) for _, h in refs]).write(prefix)
    if with_alt:
        open(prefix + ".alt", "w").write("alt_a\nalt_b\n")
    asc = synth.genome_ascii

    def rnd(n):                                   # a read's own flank: unrelated sequence that does not put an A next to the element
        f = rng.integers(0, 4, size=n, dtype=np.uint8)
        f[0] = 1 + f[0] % 3; f[-1] = 1 + f[-1] % 3
        return f
    one, two, tandem = [], [], []
    for k in range(24):                                                                     # inside one family, unrelated flanks; every fourth read differs
        e = _diverged(rng, A if k % 3 else B, 0.0 if k % 4 else 0.02)                       # from the element itself (two shorter seeds, other copies)
        one.append(asc(np.concatenate([rnd(37), e, rnd(38)])))
    for k in range(16):                                                                     # half A + half B
        ea, eb = _diverged(rng, A, 0.0 if k % 4 else 0.02), _diverged(rng, B, 0.0 if k % 4 else 0.02)
        two.append(asc(np.concatenate([ea, eb] if k % 2 else [eb, ea])))
    for lo in range(249860, 250600, 9):                                                     # across the tract's start, inside it, across its end
        tandem.append(asc(g[lo:lo + 150]))
    for lo in range(250100, 250400, 37):                                                    # ... and with a few mismatches inside the tract
        tandem.append(asc(_diverged(rng, g[lo:lo + 150], 0.02)))
    blk, _, _ = synth.make_reads_block(g, 0, 120, 150, 7171)
    unique = [bytes(r).decode() for r in blk]
    # A patch attempt: a stretch of unique sequence with 20 substituted bases in its middle gives two regions on one diagonal that no extension
    # joins, which pass mem_patch_reg's pre-tests (its alignment then runs on the wave) -- as a read of its own (two regions: deferred to the
    # 64-region table) and next to a copy of element A (~500 regions: the 640-region table's event path)
    def gapped(z, n):
        u = g[z:z + n].copy()
        u[n // 2 - 10:n // 2 + 10] = (u[n // 2 - 10:n // 2 + 10] + 2) & 3
        return u
    zs = list(range(248100, 249700, 160))                                                   # (no copy of either family near the tract)
    for k, z in enumerate(zs):
        if k % 2:
            u = gapped(z, 75)
            u[0] = 1 + u[0] % 3
            one.append(asc(np.concatenate([A, u])))
        else:
            unique.append(asc(np.concatenate([rnd(75), gapped(z, 75)])))
    reads, kind = [], []
    for i in range(max(len(one), len(two), len(tandem), len(unique))):                      # interleaved: no homogeneous stretch of a list
        for name, lst in (("one", one), ("unique", unique), ("two", two), ("tandem", tandem)):
            if i < len(lst):
                reads.append(lst[i]); kind.append(name)
    if with_alt:
        for gi in (1, 2):
            blk, _, _ = synth.make_reads_block(refs[gi][1], gi, 40, 150, 7272)
            reads += [bytes(r).decode() for r in blk]; kind += ["unique"] * len(blk)
    return prefix, reads, np.array(kind)


class _Case:
    def __init__(self, tmp, with_alt):
        from oracle import orc
        self.prefix, self.reads, self.kind = _build(tmp, with_alt)
        self.oidx = orc.Index.load(self.prefix)
        self.opt = orc.default_opt()
        before = orc.counters()["n_patch"]
        self.exp_all = orc.align_batch(self.opt, self.oidx, self.reads, keep_sec_frac=0.0, max_secondary=1 << 20)
        self.n_patch = orc.counters()["n_patch"] - before          # mem_patch_reg calls that passed the pre-tests
        self._gpu = None

    def gpu_index(self, sl):
        if self._gpu is None:
            self._gpu = sl.BWAIndex()
            self._gpu.LoadIndex(self.prefix)
        return self._gpu


@pytest.fixture(scope="module")
def plain(tmp_path_factory):
    return _Case(tmp_path_factory.mktemp("lds_tables"), False)


@pytest.fixture(scope="module")
def alt(tmp_path_factory):
    return _Case(tmp_path_factory.mktemp("lds_tables_alt"), True)


def _oracle_counts(orc, case, i):
    """(chains created, regions before de-duplication) of read i, from the oracle alone"""
    before = orc.counters()["n_chains"]
    n_reg = len(orc.stage_dump(case.opt, case.oidx, case.reads[i], 2)) // 10
    return orc.counters()["n_chains"] - before, n_reg


def test_the_reads_reach_both_tables_of_both_kernels(sl, orc, plain):
    """the copy numbers put the one-family reads into the 640-region / 768-chain tables and the two-family reads beyond both (oracle), and the GPU's
    own region lists before de-duplication say the same (keep_stages) and equal the oracle's"""
    al = sl.BWAAligner(plain.gpu_index(sl))
    al.set("keep_stages", 1)
    _same(al.alignSequences(plain.reads, keepSecFrac=0.0, maxSecondary=1 << 20), plain.exp_all, "keep_stages")
    n_reg = np.array([len(al.debug_stage(i, 2)) // 10 for i in range(len(plain.reads))])
    print("regions before de-duplication: one family %s, two families %s, tandem max %d, unique max %d" % (
        sorted(n_reg[plain.kind == "one"])[::6], sorted(n_reg[plain.kind == "two"])[::4], n_reg[plain.kind == "tandem"].max(), n_reg[plain.kind == "unique"].max()))
    assert (n_reg > REGS_MID_N).sum() >= 1, "no read beyond the 640-region table"
    assert ((n_reg >= 48) & (n_reg <= REGS_MID_N)).sum() >= 1, "no read inside the 640-region table"
    one, two, tandem = (n_reg[plain.kind == k] for k in ("one", "two", "tandem"))
    assert (two > 768).sum() >= 8                                        # beyond 768 the staged sorts run serially on one lane
    assert ((one >= 256) & (one <= REGS_MID_N)).sum() >= 16 and ((one >= 2) & (one < 64)).any()
    assert ((tandem >= 48) & (tandem <= REGS_MID_N)).sum() >= 16
    assert plain.n_patch >= 10                                           # mem_patch_reg's alignment: in ~500-region reads and in two-region reads
    big = lambda k: int(np.flatnonzero(plain.kind == k)[np.argmax(n_reg[plain.kind == k])])
    for k, i in (("one", big("one")), ("two", big("two")), ("tandem", big("tandem"))):
        chains, regs = _oracle_counts(orc, plain, i)
        print("read %d (%s): oracle %d chains, %d regions; GPU %d regions" % (i, k, chains, regs, n_reg[i]))
        assert regs == n_reg[i]
        assert np.array_equal(al.debug_stage(i, 2), orc.stage_dump(plain.opt, plain.oidx, plain.reads[i], 2))
        if k == "one":
            assert 256 <= chains <= COOP_N1                              # the 768-chain table
        if k == "two":
            assert chains > COOP_N1                                      # ... and beyond it
        if k == "tandem":
            assert chains >= 10                                          # (bwa's chain set is a single sorted leaf up to nine chains)


@pytest.mark.parametrize("knobs", [(), (("regs_big", 2),), (("heavy_seeds", 1),), (("wide_index", 1),)], ids=["default", "regs_big2", "heavy_seeds1", "wide_index"])
def test_repeat_families_and_tandem_tract_match_oracle(sl, orc, plain, knobs):
    al = sl.BWAAligner(plain.gpu_index(sl))
    for k, v in knobs:
        al.set(k, v)
    _same(al.alignSequences(plain.reads, keepSecFrac=0.0, maxSecondary=1 << 20), plain.exp_all, "every hit kept, %s" % (knobs,))
    if not knobs:                                  # (a new aligner: read i of a batch is the aligner's i-th call, which salts mem_mark_primary_se's hash)
        al = sl.BWAAligner(plain.gpu_index(sl))
        _same(al.alignSequences(plain.reads), orc.align_batch(plain.opt, plain.oidx, plain.reads), "the glue's default filters")


@pytest.mark.parametrize("knobs", [(), (("regs_big", 2), ("heavy_seeds", 1))], ids=["default", "regs_big2_heavy_seeds1"])
def test_family_copies_on_alt_contigs_match_oracle(sl, orc, alt, knobs):
    """the staged two-round marking (ALT-aware index, many regions): hits on the ALT contigs and on the primary assembly in one read"""
    rid = alt.exp_all["rid"]
    assert np.isin(rid, (1, 2)).sum() > 500 and (rid == 0).sum() > 5000
    al = sl.BWAAligner(alt.gpu_index(sl))
    for k, v in knobs:
        al.set(k, v)
    _same(al.alignSequences(alt.reads, keepSecFrac=0.0, maxSecondary=1 << 20), alt.exp_all, "ALT contigs, %s" % (knobs,))
