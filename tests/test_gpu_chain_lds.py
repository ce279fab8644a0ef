"""k_chain_lds (dev_chain_lds.h): the light reads' chaining with a read's lists in LDS ("chain_lds" = 1, the default) against the same
algorithm on the seed-slot columns in HBM ("chain_lds" = 0, k_chain) and against the CPU oracle -- every field of every record, CIGAR
words included -- on the fixture reads plus reads built to meet each edge of the LDS pass: the last seed-slot count it takes and the
first it does not, a 10th chain (the pass gives the read up and it starts over on the HBM columns), no interval at all, seeds that all
bridge two contigs, the exact-match shortcut, a read heavy enough for the wave-per-read kernel, mixed lengths in one wave."""
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

CHAIN_LDS_SEEDS = 12          # dev_chain_lds.h
FIELDS = ("hit_off", "rid", "pos", "flag", "mapq", "score", "nm", "na", "n_cigar", "cig_off", "cigar")
SIZES = (1, 63, 64, 65, 129, 513, 3000)          # up to 512 reads a chunk runs one read per wave (k_chain); 513 is the first size on lanes
# two k-mers with a handful of copies each, joined: at most 12 seed slots on 10 or more diagonals far apart
TEN_CHAINS = ("AAAAAAAAAAAAAAAAAAAAGGTAGACGGGGTTTCACCGTGTTAG", "ACCTCAGGTGATCTGCCCACCTTGAGTTCAAGACCAGCCTGGGCA",
              "CTCAAGTGATCCTCCCACCTCATCAGGGTTTCACCATGTTAGCCA", "AATGCCAGCACTTTGGGAGGCCTCTGCCTCAGCCTCCCAAAGTGC")


def same(got, exp, what):
    for k in FIELDS:
        assert np.array_equal(got[k], exp[k]), "%s: field %s differs" % (what, k)


def seed_slots(orc, opt, index, seq):
    """the read's seed-slot count as k_seed_epi accounts it: the occurrences mem_chain will look up, over the read's intervals"""
    n = 0
    for _, _, _, x2 in orc.stage_dump(opt, index, seq, 0).reshape(-1, 4):
        x2 = int(x2)
        if x2 > opt.max_occ:
            step = x2 // opt.max_occ
            n += min((x2 + step - 1) // step, opt.max_occ)
        else:
            n += x2
    return n


@pytest.fixture(scope="module")
def pool(orc, tiny_index, sim_reads, golden_dir):
    names, refs = orc.read_fasta(os.path.join(golden_dir, "tiny.fa"))
    (_, s1), (_, s2) = sim_reads
    opt = orc.default_opt()
    slots1 = [seed_slots(orc, opt, tiny_index, s) for s in s1]
    at = lambda n: s1[slots1.index(n)]
    bridge = refs[0][-15:] + refs[1][:15]         # 30 bp: a seed has 19 bp or more, so every seed of it holds the contig boundary
    exact = refs[1][60000:60150].upper()
    edges = [at(CHAIN_LDS_SEEDS), at(CHAIN_LDS_SEEDS + 1), TEN_CHAINS[0], "N" * 150, bridge, exact, s1[int(np.argmax(slots1))],
             s1[0][:40], s1[1][:75], s2[0][:101], refs[2][500:750], "", "ACGT"] + list(TEN_CHAINS[1:])
    assert max(slots1) >= 64
    assert seed_slots(orc, opt, tiny_index, "N" * 150) == 0
    seqs = edges + list(s1[:3000 - len(edges)])
    slots = [seed_slots(orc, opt, tiny_index, s) for s in edges] + slots1[:3000 - len(edges)]
    assert all(slots[edges.index(t)] <= CHAIN_LDS_SEEDS for t in TEN_CHAINS)

    def chaining(sq):
        """what mem_chain does with one read in the checker: occurrences looked up, seeds on one contig (rid >= 0), chains created"""
        a = orc.counters()
        orc.align_batch(opt, tiny_index, [sq])
        b = orc.counters()
        return tuple(b[k] - a[k] for k in ("n_sa", "n_seeds", "n_chains"))
    for t in TEN_CHAINS:
        assert chaining(t)[2] >= 10, "%s: fewer than ten chains" % t
    n_sa, n_seeds, _ = chaining(bridge)
    assert n_sa > 0 and n_seeds == 0, "the bridging read: %d occurrences, %d of them inside a contig" % (n_sa, n_seeds)
    return seqs, slots, {n: orc.align_batch(opt, tiny_index, seqs[:n]) for n in SIZES}, len(edges)


def aligner(sl, tiny_gpu, on, production):
    al = sl.BWAAligner(tiny_gpu)
    al.set("chain_lds", on)
    if production:
        al.set("split_min", 16)                    # light / heavy partition, cooperative chaining of the heavy reads, split extension
    return al


@pytest.mark.parametrize("production", (0, 1))
def test_on_off_oracle_by_batch_size(sl, tiny_gpu, pool, production):
    seqs, slots, exp, _ = pool
    for on in (1, 0):
        al = aligner(sl, tiny_gpu, on, production)
        for n in SIZES:
            al.ordinal = 0
            same(al.alignSequences(seqs[:n]), exp[n], "chain_lds=%d production=%d n=%d" % (on, production, n))
            n_fit = sum(1 for c in slots[:n] if c <= CHAIN_LDS_SEEDS)
            lanes = on and (n == 1 or n > 512 or (production and n >= 16))      # (else one read per wave: small_spread, k_chain)
            # every read with at most CHAIN_LDS_SEEDS seed slots went through the LDS pass, and no other read did
            assert al.counter("chain_lds_reads") + al.counter("chain_lds_bail") == (n_fit if lanes else 0), (on, production, n)
            if lanes and n == 3000:
                assert al.counter("chain_lds_bail") > 0             # the 10th chain
                assert al.counter("heavy_reads") > 0                # 64 seed occurrences or more: one wave per read, not this kernel


def test_u64_index(sl, tiny_gpu, pool):
    """the 64-bit index keeps positions as 8-byte elements in the slice (another layout, fewer waves per CU)"""
    seqs, slots, exp, _ = pool
    for on in (1, 0):
        al = aligner(sl, tiny_gpu, on, 1)
        al.set("wide_index", 1)
        for n in (513, 3000):
            al.ordinal = 0
            same(al.alignSequences(seqs[:n]), exp[n], "u64 index, chain_lds=%d n=%d" % (on, n))
            assert al.counter("chain_lds_reads") + al.counter("chain_lds_bail") == (sum(1 for c in slots[:n] if c <= CHAIN_LDS_SEEDS) if on else 0)
        if on:
            assert al.counter("chain_lds_bail") > 0


def test_chunk_with_long_read_stays_on_hbm_columns(sl, orc, tiny_gpu, tiny_index, pool, golden_dir):
    names, refs = orc.read_fasta(os.path.join(golden_dir, "tiny.fa"))
    seqs, _, _, n_edges = pool
    batch = seqs[:n_edges + 600] + [refs[1][2000:2900]]          # 900 bp: bwa's seed filter is live, the chunk carries per-seed scores
    exp = orc.align_batch(orc.default_opt(), tiny_index, batch)
    for on in (1, 0):
        al = aligner(sl, tiny_gpu, on, 0)
        same(al.alignSequences(batch), exp, "long-read chunk, chain_lds=%d" % on)
        assert al.counter("chain_lds_reads") + al.counter("chain_lds_bail") == 0


@pytest.mark.parametrize("production", (0, 1))
def test_stage_dump_on_off(sl, orc, tiny_gpu, tiny_index, pool, production):
    """kept chains with their seeds, and the regions of extension, read by read: LDS pass == HBM columns == oracle"""
    seqs, _, _, n_edges = pool
    batch = seqs[:n_edges + 700]
    opt = orc.default_opt()
    dumps = []
    for on in (1, 0):
        al = aligner(sl, tiny_gpu, on, production)
        al.set("keep_stages", 1)
        al.alignSequences(batch)
        if on:
            assert al.counter("chain_lds_reads") > 0
        dumps.append([(al.debug_stage(i, 1), al.debug_stage(i, 2)) for i in range(len(batch))])
    assert any(len(d[0]) and d[0][0] == -1 for d in dumps[0])          # an error-free read: the exact-match shortcut
    for i, sq in enumerate(batch):
        for what in (0, 1):
            assert np.array_equal(dumps[0][i][what], dumps[1][i][what]), "read %d: stage %d differs between chain_lds = 1 and 0" % (i, what + 1)
        ch = dumps[0][i][0]
        if not (len(ch) and ch[0] == -1):             # (the exact-match shortcut has no chain list; its region is checked below)
            assert np.array_equal(ch, orc.stage_dump(opt, tiny_index, sq, 1)), "read %d: chains differ from the oracle's" % i
        assert np.array_equal(dumps[0][i][1].reshape(-1, 10), orc.stage_dump(opt, tiny_index, sq, 2).reshape(-1, 10)), "read %d: regions differ from the oracle's" % i
