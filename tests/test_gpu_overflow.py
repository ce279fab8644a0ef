"""The overflow-and-retry paths of the traceback arena and the CIGAR pool ("What a flagged CIGAR job leaves behind").

A chunk's CIGAR kernels take space from two bump-allocated pools and compare each take with the cap; a take that does not fit raises
OVF_ZARENA / OVF_CIGAR, the job stops, and the host doubles the cap and runs the chunk again (at most 12 times), remembering what it
learnt.  The budgets are generous, so a small batch never gets there: the test hooks "z_start" / "cig_start" set the caps of a chunk's
first attempt instead.  Under the hook 1 MiB behind each pool is filled with a pattern before every attempt and compared after it
("guard_dirty": a check that lets a job write past its cap shows up as changed bytes, inside allocated memory), and every check ORs a bit
of its own into the flag word ("ovf_sites": which of the thirteen checks the batch reached).

Every case: records equal to the CPU oracle's in all eleven fields, a clean guard, at least one retry, no further retry when the same
batch runs again on the same aligner (what a chunk needed is remembered), and the same records with no retry from an aligner with the
hook off."""
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

FIELDS = ("hit_off", "rid", "pos", "flag", "mapq", "score", "nm", "na", "n_cigar", "cig_off", "cigar")
# OVS_* of seqlib_amd/csrc/dev_types.h
SITES = dict(Z_GEN=1 << 8, Z_BAND=1 << 9, Z_BAND_BLOCK=1 << 10, Z_SEG=1 << 11, Z_LANE=1 << 12, Z_DP=1 << 13, Z_DP_WAVE=1 << 14,
             C_BAND=1 << 15, C_LANE=1 << 16, C_LONG=1 << 17, C_FAST=1 << 18, C_FAST_COOP=1 << 19, C_DP=1 << 20)
# Sites the inputs of this module cannot reach, each with the reason in the code (at most two may stand here).
UNREACHED = {}
Z_SMALL, C_SMALL = 4096, 16            # less than one 150 bp band; room for five no-DP CIGARs
Z_AMPLE, C_AMPLE = 1 << 27, 1 << 20    # more than any batch of this module needs


def names_of(bits):
    return sorted(k for k, v in SITES.items() if bits & v)


def same(got, exp, what):
    for k in FIELDS:
        assert np.array_equal(got[k], exp[k]), "%s: field %s differs from the oracle" % (what, k)


def revcomp(s):
    return s[::-1].translate(str.maketrans("ACGT", "TGCA"))


def subst(rng, s, n):
    s = list(s)
    for _ in range(n):
        s[int(rng.integers(0, len(s)))] = "ACGT"[int(rng.integers(0, 4))]
    return "".join(s)


def has_indel(res, i):
    c = res["cigar"][int(res["cig_off"][int(res["hit_off"][i])]):int(res["cig_off"][int(res["hit_off"][i + 1])])]
    return bool(np.any(((c & 0xf) == 1) | ((c & 0xf) == 2)))


class Cases:
    """the inputs with their oracle records (computed once), and every case's outcome (run once, whichever test asks first)"""

    def __init__(self, sl, orc, tiny_gpu, tiny_index, sim_reads, golden_dir):
        self.sl, self.orc, self.gpu, self.index = sl, orc, tiny_gpu, tiny_index
        self.memo, self.exp = {}, {}
        _, refs = orc.read_fasta(os.path.join(golden_dir, "tiny.fa"))
        (_, s1), _ = sim_reads
        opt = orc.default_opt()
        first = orc.align_batch(opt, tiny_index, list(s1[:700]))
        dp = next(i for i in range(700) if has_indel(first, i))          # a read whose CIGAR needs the dynamic program, put first: the batch of one read has work for the arena
        self.short = [s1[dp]] + [s for i, s in enumerate(s1[:700]) if i != dp]
        # the reads of 900 bp and more of test_long_reads_seed_filter_path (tests/test_gpu_parity.py), the first eight
        rng = np.random.default_rng(5)
        longs = []
        for L in (700, 726, 727, 728, 733, 800, 1000, 1500, 2500, 3999, 5000, 5000, 7990):
            for rep in range(3):
                ci = int(rng.integers(0, len(refs)))
                L2 = min(L, len(refs[ci]) - 10)
                p = int(rng.integers(0, len(refs[ci]) - L2))
                s = list(refs[ci][p:p + L2])
                for _ in range(int(L2 * (0.0, 0.01, 0.04)[rep])):
                    s[int(rng.integers(0, L2))] = "ACGT"[int(rng.integers(0, 4))]
                if rep == 2:
                    q = L2 // 3
                    s[q:q] = list("ACGTTGCAAC")
                    del s[2 * q:2 * q + 7]
                    cj = (ci + 1) % len(refs)
                    s[-200:] = list(refs[cj][1000:1200])
                t = "".join(s)
                if rng.random() < 0.5:
                    t = revcomp(t)
                longs.append(t)
        self.long = [t for t in longs if len(t) >= 900][:8]
        assert len(self.long) == 8
        # Contigs.  A chunk's CIGAR jobs go to the block kernel only when it has two or more of them (run_chunk sorts the list then), so each read is a
        # chimera: the part under test, and 600 bp of another contig with substitutions (a second job for the dynamic program).
        rng = np.random.default_rng(7)
        tail = lambda ci: subst(rng, refs[ci][2000:2600], 6)
        a = refs[0][20000:24400]
        # a 70 bp deletion in 4 330 bp: the first band is at least 2 * 73 + 1 = 147 columns -- more than two per lane of a wave -- on 4 096 rows or more
        # (k_cig_job_keys: a block job), and too short to be cut into segments (gseg_count: 6 144 reference rows)
        self.block = subst(rng, a[:2200] + a[2270:], 8) + tail(2)
        # 17 000 bp >= 4 * GSEG_LEN: a block job whatever its band, cut into four segments (k_gseg_plan)
        self.seg = subst(rng, refs[1][5000:22000], 30) + tail(3)
        # With bandwidth 450 the extension crosses a 420 bp insertion between two flanks of 500 bp: one region, whose CIGAR's band is 2 * 423 + 1 columns -- beyond
        # the 832 of the wave kernel (CIG_BAND_MAX_COLS), so the job is left to k_cig_long: one lane, dev_gen_cigar2.  (At the default bandwidth of 100 no region
        # has a band that wide: the extension does not cross such a gap, and mem_patch_reg joins two regions across at most 2 w = 200 bp.)  The alignment is
        # 847 x 1 000 cells on ONE lane, a second each time: the slowest case of the module
        b = refs[1][30000:31000]
        self.wide = b[:500] + "".join("ACGT"[int(x)] for x in rng.integers(0, 4, 420)) + b[500:]

    def oracle(self, key, seqs, w=None):
        if key not in self.exp:
            opt = self.orc.default_opt()
            if w:
                opt.w = w
            self.exp[key] = self.orc.align_batch(opt, self.index, seqs)
        return self.exp[key]

    def aligner(self, knobs, w=None):
        al = self.sl.BWAAligner(self.gpu)
        for k, v in knobs:
            al.set(k, v)
        if w:
            al.SetBandwidth(w)
        return al

    def hooked(self, what, seqs, exp, knobs=(), z=Z_SMALL, c=C_SMALL, w=None):
        """one case: the five assertions of the module's docstring; returns the sites the batch reached"""
        al = self.aligner(knobs, w)
        al.set("z_start", z)
        al.set("cig_start", c)
        same(al.alignSequences(seqs), exp, what + ", first call")
        retries, sites = al.counter("retries"), al.counter("ovf_sites")
        print("%s: %d retries, sites %s" % (what, retries, names_of(sites)))
        assert al.counter("guard_dirty") == 0, "%s: %d bytes behind the pools changed" % (what, al.counter("guard_dirty"))
        assert retries >= 1, what
        assert sites & ~SITES["Z_DP_WAVE"], "%s: a retry, and no site that raised it" % what
        al.ordinal = 0
        same(al.alignSequences(seqs), exp, what + ", second call")
        assert al.counter("retries") == retries, "%s: the second call of the same batch ran a chunk again" % what
        assert al.counter("guard_dirty") == 0, what
        off = self.aligner(knobs, w)
        same(off.alignSequences(seqs), exp, what + ", hook off")
        assert (off.counter("retries"), off.counter("ovf_sites"), off.counter("guard_dirty")) == (0, 0, 0), what
        return sites

    def run(self, name):
        if name not in self.memo:
            self.memo[name] = CASES[name][0](self)
        return self.memo[name]


def short_case(knobs, n=700, **kw):
    return lambda cs: cs.hooked("short reads n=%d %s %s" % (n, knobs, kw), cs.short[:n], cs.oracle(("short", n), cs.short[:n]), knobs, **kw)


def contig_case(attr, **kw):
    def run(cs):
        seq = getattr(cs, attr)
        z = (len(seq) * 208 + 1023) >> 10          # a 4096th of twice the long reads' budget: eleven or twelve doublings reach what the read needs
        return cs.hooked("contig %s (%d bp, z_start %d)" % (attr, len(seq), z), [seq], cs.oracle(attr, [seq]), (), z=z, **kw)
    return run


# name -> (case, sites it must reach: the ones its routing makes certain, whatever the order in which the two pools run out)
PROD = (("split_min", 16),)
CASES = {
    # production routing (light / heavy partition, k_cig_lanes from 256 reads): the lane kernel's block, the no-DP CIGARs, k_cig_dp behind them
    "short_il1": (short_case(PROD + (("cig_lane_il", 1),)), ("Z_LANE", "C_FAST_COOP")),
    "short_il0": (short_case(PROD + (("cig_lane_il", 0),)), ("Z_LANE", "C_FAST_COOP")),
    "short_dp": (short_case(PROD + (("cig_lanes", 0),)), ("Z_DP_WAVE", "Z_DP", "C_FAST_COOP")),          # every DP job on k_cig_dp
    "short_fast": (short_case(PROD + (("cig_fast_coop", 0),)), ("C_FAST",)),                            # k_cig_fast
    "short_u64": (short_case(PROD + (("wide_index", 1),)), ("Z_LANE", "C_FAST_COOP")),
    # with the arena ample every lane job gets as far as its CIGAR words
    "short_il1_c": (short_case(PROD, z=Z_AMPLE), ("C_LANE",)),
    "short_il0_c": (short_case(PROD + (("cig_lane_il", 0),), z=Z_AMPLE), ("C_LANE",)),
    "short_dp_c": (short_case(PROD + (("cig_lanes", 0),), z=Z_AMPLE), ("C_DP",)),
    # small chunks, one read per wave (below split_min, up to 512 reads): k_cig_dp; a wave's own 16 KiB stretch does not fit 4 096 bytes
    "small_1": (short_case((), 1), ("Z_DP_WAVE", "Z_DP")),
    "small_63": (short_case((), 63), ("Z_DP_WAVE", "Z_DP")),
    "small_64": (short_case((), 64), ("Z_DP_WAVE", "Z_DP")),
    "small_65": (short_case((), 65), ("Z_DP_WAVE", "Z_DP")),
    # 900 bp and more: band coordinates, one wave per job (k_cig_band)
    "long": (lambda cs: cs.hooked("long reads", cs.long, cs.oracle("long", cs.long)), ("Z_BAND",)),
    "long_c": (lambda cs: cs.hooked("long reads, arena ample", cs.long, cs.oracle("long", cs.long), z=Z_AMPLE, c=1), ("C_BAND",)),
    "contig_block": (contig_case("block"), ("Z_BAND_BLOCK",)),
    "contig_seg": (contig_case("seg"), ("Z_SEG", "Z_BAND_BLOCK")),          # (the job whose cut was dropped runs uncut into the band check)
    "contig_seg_c": (lambda cs: cs.hooked("contig seg, arena ample", [cs.seg], cs.oracle("seg", [cs.seg]), z=Z_AMPLE, c=1), ("C_BAND",)),
    # z: every attempt whose arena is too small ends at dev_gen_cigar2's check; c = 4: once the arena fits, the five words of "500M420I500M" do not
    "wide_band": (lambda cs: cs.hooked("420 bp insertion, w = 450", [cs.wide], cs.oracle("wide", [cs.wide], w=450), c=4, w=450), ("Z_GEN", "C_LONG")),
}


@pytest.fixture(scope="module")
def cases(sl, orc, tiny_gpu, tiny_index, sim_reads, golden_dir):
    return Cases(sl, orc, tiny_gpu, tiny_index, sim_reads, golden_dir)


@pytest.mark.parametrize("name", list(CASES))
def test_overflow_retry_learn(cases, name):
    sites = cases.run(name)
    missing = [s for s in CASES[name][1] if not sites & SITES[s]]
    assert not missing, "%s reached %s, not %s" % (name, names_of(sites), missing)


def fits(cases, al, seq, exp, knob, v):
    """one read with `knob` at v: records and guard checked; True when no chunk ran again"""
    al.set(knob, v)
    al.ordinal = 0
    before = al.counter("retries")
    same(al.alignSequences([seq]), exp, "%s = %d" % (knob, v))
    assert al.counter("guard_dirty") == 0, "%s = %d: %d bytes behind the pools changed" % (knob, v, al.counter("guard_dirty"))
    return al.counter("retries") == before


@pytest.mark.parametrize("knob,other,ample", [("z_start", "cig_start", C_AMPLE), ("cig_start", "z_start", Z_AMPLE)])
def test_edge_of_fit(cases, knob, other, ample):
    """the smallest cap at which one read with an indel runs once (Z*: the arena with the pool ample; C*: the pool with the arena ample): one less retries, and
    either side of the edge gives the oracle's records with a clean guard.  Measured on an MI355X: Z* = 16 384 (the 16 KiB stretch the wave of k_cig_dp
    keeps), C* = 256 (the words it reserves ahead); not asserted, they follow the routing."""
    seq = cases.short[0]
    exp = cases.oracle(("short", 1), [seq])
    al = cases.aligner(())
    al.set(other, ample)
    lo, hi = 1, 65536
    assert fits(cases, al, seq, exp, knob, hi)
    while lo < hi:                                # 16 steps
        mid = (lo + hi) // 2
        if fits(cases, al, seq, exp, knob, mid):
            hi = mid
        else:
            lo = mid + 1
    print("edge of fit: smallest %s with no retry = %d" % (knob, lo))
    assert lo > 1
    assert not fits(cases, al, seq, exp, knob, lo - 1)
    assert fits(cases, al, seq, exp, knob, lo)


def test_refusal_after_twelve_doublings(cases):
    """z_start = 1 doubles to 4 096 bytes in twelve retries, less than the band of one 150 bp read: the call fails with SLX_ENOMEM, nothing was written behind the
    pools, and the aligner works again with the hook off"""
    from seqlib_amd import _ffi
    seq = cases.short[0]
    exp = cases.oracle(("short", 1), [seq])
    al = cases.aligner(())
    al.set("z_start", 1)
    al.set("cig_start", C_AMPLE)
    with pytest.raises(_ffi.SlxError) as e:
        al.alignSequences([seq])
    assert e.value.code == _ffi.SLX_ENOMEM and "still overflows" in str(e.value), str(e.value)
    assert al.counter("guard_dirty") == 0
    assert al.counter("ovf_sites") & SITES["Z_DP"]
    al.set("z_start", 0)
    al.set("cig_start", 0)
    al.ordinal = 0
    before = al.counter("retries")
    same(al.alignSequences([seq]), exp, "after the refusal, hook off")
    assert al.counter("retries") == before and al.counter("guard_dirty") == 0


def test_hook_off_reports_nothing(sl, orc, tiny_gpu, tiny_index, sim_reads):
    (_, s1), _ = sim_reads
    al = sl.BWAAligner(tiny_gpu)
    same(al.alignSequences(s1), orc.align_batch(orc.default_opt(), tiny_index, list(s1)), "3 000 fixture reads")
    assert (al.counter("retries"), al.counter("ovf_sites"), al.counter("guard_dirty")) == (0, 0, 0)


def test_every_site_was_reached(cases):
    """the union over the module's cases holds every check that compares a take with a cap, but the ones UNREACHED names"""
    assert len(UNREACHED) <= 2
    seen = 0
    for name in CASES:
        seen |= cases.run(name)
    want = [s for s in SITES if s not in UNREACHED]
    missing = [s for s in want if not seen & SITES[s]]
    assert not missing, "never reached: %s (reached: %s)" % (missing, names_of(seen))
    assert not [s for s in UNREACHED if seen & SITES[s]], "listed as unreachable, and reached: fix the list"
