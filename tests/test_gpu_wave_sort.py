"""The wave sort of the many-region and many-hit reads ("wave_sort": dev_wave_sort.h in dev_fin_regs' sort_handles and in k_hits_wave), bit for bit
against the oracle on the small reference of tests/test_gpu_lds_tables.py (460 kb, two dispersed families, the period-5 tract):

  * one-family reads: ~500 regions, the 640-region table;
  * two-family reads: more than 768 regions, the 2 048-region table, whose sorts ran on one lane before;
  * tract reads: equal region ends, so the first sort has a tie and falls back to one lane from the saved order;
  * unique reads in between.

"wave_sort" 1 sends lists of 128 handles or more through the network and counts ranks for shorter ones; 2 sends every list through it (the tract
reads have 50 to 100 regions), 0 none.

Which path a sort took is asserted through the counters "sort_wave", "sort_serial" and "sort_serial_re" (the reads' first sort, by region end), and
for the hit sort "hits_sort_wave" / "hits_sort_serial": the
reads for those batches are picked on the CPU from the oracle's regions before de-duplication, so that the reference alone decides what must happen."""
import numpy as np
import pytest

from tests.test_gpu_lds_tables import _Case, _same

pytestmark = pytest.mark.gpu

HITS_BIG = 12           # dev_fin2.h: reads with more hits than this take k_hits_wave
RANK_MAX = 768          # "wave_sort" 0: lists longer than this were sorted by one lane
REGS_BIG_N = 2048       # the largest LDS stage: longer lists are not staged (and not counted)


class _SortCase(_Case):
    def __init__(self, tmp):
        from oracle import orc
        super().__init__(tmp, False)
        self.exp_default = orc.align_batch(self.opt, self.oidx, self.reads)
        # region ends before de-duplication, per read, from the oracle alone
        self.re = [orc.stage_dump(self.opt, self.oidx, r, 2).reshape(-1, 10)[:, 1] for r in self.reads]
        n_reg = np.array([len(e) for e in self.re])
        distinct = np.array([len(np.unique(e)) == len(e) for e in self.re])
        self.n_reg = n_reg
        # two-family reads beyond the rank count's 768 handles whose region ends are all different: their first sort has no tie
        self.two_distinct = [i for i in np.flatnonzero(self.kind == "two") if RANK_MAX < n_reg[i] <= REGS_BIG_N and distinct[i]]
        # tract reads with a repeated region end: their first sort has one
        self.tract_tied = [i for i in np.flatnonzero(self.kind == "tandem") if 48 <= n_reg[i] <= REGS_BIG_N and not distinct[i]]
        # one-family reads with hundreds of hits of which no two have the same (mapq, rid, pos): their hit sort has no tie
        off = self.exp_all["hit_off"]

        def hits_distinct(i):
            keys = set(zip(self.exp_all["mapq"][off[i]:off[i + 1]].tolist(), self.exp_all["rid"][off[i]:off[i + 1]].tolist(), self.exp_all["pos"][off[i]:off[i + 1]].tolist()))
            return len(keys) == off[i + 1] - off[i]
        self.many_hits = [i for i in np.flatnonzero(self.kind == "one") if off[i + 1] - off[i] > 20 * HITS_BIG and hits_distinct(i)]


@pytest.fixture(scope="module")
def case(tmp_path_factory):
    return _SortCase(tmp_path_factory.mktemp("wave_sort"))


def _aligner(sl, case, knobs):
    al = sl.BWAAligner(case.gpu_index(sl))
    for k, v in knobs:
        al.set(k, v)
    return al


def _counts(al):
    return al.counter("sort_wave"), al.counter("sort_serial"), al.counter("sort_serial_re")


def test_the_reference_offers_every_kind_of_list(case):
    """what the batches below rely on, from the oracle alone"""
    print("regions: two-family distinct %s, tract tied %s, many hits %s" % (
        [int(case.n_reg[i]) for i in case.two_distinct], [int(case.n_reg[i]) for i in case.tract_tied][:8], [int(case.n_reg[i]) for i in case.many_hits][:8]))
    assert len(case.two_distinct) >= 4
    assert len(case.tract_tied) >= 8
    assert len(case.many_hits) >= 4
    one = case.n_reg[case.kind == "one"]
    assert ((one >= 256) & (one <= 640)).sum() >= 16


@pytest.mark.parametrize("knobs", [(("wave_sort", 1),), (("wave_sort", 0),), (("wave_sort", 2),), (("wave_sort", 1), ("regs_big", 2)), (("wave_sort", 0), ("regs_big", 2)),
                                   (("wave_sort", 2), ("regs_big", 2))],
                         ids=["wave_sort1", "wave_sort0", "wave_sort2", "wave_sort1_regs_big2", "wave_sort0_regs_big2", "wave_sort2_regs_big2"])
def test_mixed_batch_matches_oracle(sl, case, knobs):
    al = _aligner(sl, case, knobs)
    _same(al.alignSequences(case.reads, keepSecFrac=0.0, maxSecondary=1 << 20), case.exp_all, "every hit kept, %s" % (knobs,))
    on_wave, serial, serial_re = _counts(al)
    print("%s: sort_wave %d, sort_serial %d (by region end %d)" % (knobs, on_wave, serial, serial_re))
    assert on_wave > 0 and serial > 0 and 0 < serial_re <= serial
    al = _aligner(sl, case, knobs)          # (a new aligner: read i of a batch is the aligner's i-th call, which salts mem_mark_primary_se's hash)
    _same(al.alignSequences(case.reads), case.exp_default, "the glue's default filters, %s" % (knobs,))
    assert _counts(al) == (on_wave, serial, serial_re)


def test_default_is_the_wave_sort(sl, case):
    """no knob set: the same counts as wave_sort = 1"""
    a, b = _aligner(sl, case, ()), _aligner(sl, case, (("wave_sort", 1),))
    a.alignSequences(case.reads)
    b.alignSequences(case.reads)
    assert _counts(a) == _counts(b) and _counts(a)[0] > 0


def test_long_lists_without_a_tie_stay_on_the_wave(sl, orc, case):
    """two-family reads (more than 768 regions) whose region ends all differ: no first sort falls back; with the knob off every one of them did"""
    reads = [case.reads[i] for i in case.two_distinct]
    exp = orc.align_batch(case.opt, case.oidx, reads, keep_sec_frac=0.0, max_secondary=1 << 20)
    al = _aligner(sl, case, (("wave_sort", 1),))
    _same(al.alignSequences(reads, keepSecFrac=0.0, maxSecondary=1 << 20), exp, "two-family reads, wave_sort 1")
    on_wave, serial, serial_re = _counts(al)
    print("two-family reads: sort_wave %d, sort_serial %d (by region end %d)" % (on_wave, serial, serial_re))
    assert serial_re == 0
    assert on_wave >= len(reads)                 # at least the first sort of every read
    al = _aligner(sl, case, (("wave_sort", 0),))
    _same(al.alignSequences(reads, keepSecFrac=0.0, maxSecondary=1 << 20), exp, "two-family reads, wave_sort 0")
    assert al.counter("sort_serial_re") == len(reads)


def test_tied_region_ends_fall_back(sl, orc, case):
    """tract reads with a repeated region end: every first sort falls back to one lane, from the order saved before the network ran"""
    reads = [case.reads[i] for i in case.tract_tied]
    exp = orc.align_batch(case.opt, case.oidx, reads, keep_sec_frac=0.0, max_secondary=1 << 20)
    for v in (2, 1, 0):          # (2: the network for these lists of 50 to 100 handles too; 1: they are short enough for the rank count)
        al = _aligner(sl, case, (("wave_sort", v),))
        _same(al.alignSequences(reads, keepSecFrac=0.0, maxSecondary=1 << 20), exp, "tract reads, wave_sort %d" % v)
        on_wave, serial, serial_re = _counts(al)
        print("tract reads, wave_sort %d: sort_wave %d, sort_serial %d (by region end %d)" % (v, on_wave, serial, serial_re))
        assert serial > 0 and serial_re == len(reads)


@pytest.mark.parametrize("wave_sort", [1, 0, 2])
def test_many_hit_read_through_k_hits_wave(sl, orc, case, wave_sort):
    """one read with hundreds of hits, no two with equal keys, alone in its batch: k_hits_wave sorts them (mapq descending, rid, pos) on the wave, not on one lane"""
    read = [case.reads[case.many_hits[0]]]
    exp = orc.align_batch(case.opt, case.oidx, read, keep_sec_frac=0.0, max_secondary=1 << 20)
    assert len(exp["rid"]) > HITS_BIG
    assert len(set(zip(exp["mapq"].tolist(), exp["rid"].tolist(), exp["pos"].tolist()))) == len(exp["rid"])          # (alone in its batch too: no tie)
    al = _aligner(sl, case, (("wave_sort", wave_sort),))
    _same(al.alignSequences(read, keepSecFrac=0.0, maxSecondary=1 << 20), exp, "many hits, wave_sort %d" % wave_sort)
    assert al.counter("hits_wave_reads") == 1
    assert (al.counter("hits_sort_wave"), al.counter("hits_sort_serial")) == (1, 0)
    al = _aligner(sl, case, (("wave_sort", wave_sort),))
    _same(al.alignSequences(read), orc.align_batch(case.opt, case.oidx, read), "many hits, default filters, wave_sort %d" % wave_sort)
