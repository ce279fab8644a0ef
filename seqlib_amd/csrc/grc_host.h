// grc_host.h -- what the interval unit (include/seqlib_amd_grc.h) computes per interval and per query, compilable for host and device like cov_host.h: the sort
// keys of the build, the searches of the sorted index, the overlap and containment tests, the exact count, the fill of one query's hits by one lane, the width
// sweep and the merge flags.  dev_grc.h's kernels, slx_grc_query_host, the host-only object and tests/cpp/grc_host_test.cpp (under ASan + UBSan) all go over these
// bodies.  The record's end is the read filter's (dev_rfilter.h: rf_end).
#pragma once
#include <stdint.h>
#include <algorithm>
#include <numeric>
#include <vector>
#include "dev_rfilter.h"

// one interval as the C-ABI passes it (slx_grc_iv has the same layout)
struct grc_iv { int32_t chr, pos1, pos2; char strand; };

// The index over n intervals sorted by (chr, pos1, pos2), ties in the caller's order:
//   chr, p1, p2, strand, perm   entry i of the sorted order and the caller's index of it
//   run_p2                      the largest p2 among the entries of chr[i] up to and including i (non-decreasing inside a chr)
//   ends                        the p2 values of every chr's segment once more, ascending inside the segment
//   seg_chr, seg_beg            the n_seg distinct chr values ascending, and seg_beg[k] .. seg_beg[k + 1] the entries of seg_chr[k]
struct grc_idx {
    const int32_t *chr, *p1, *p2, *perm, *run_p2, *ends, *seg_chr;
    const uint8_t *strand;
    const uint32_t *seg_beg;
    uint32_t n, n_seg;
};

#define GRC_IGNORE_STRAND 1u
#define GRC_CONTAINED 2u

// ---- the build's sort keys: signed numbers in unsigned order
RF_HD uint32_t grc_flip(int32_t v) { return (uint32_t)v ^ 0x80000000u; }
RF_HD int32_t grc_unflip(uint32_t v) { return (int32_t)(v ^ 0x80000000u); }
RF_HD uint64_t grc_key2(int32_t hi, int32_t lo) { return (uint64_t)grc_flip(hi) << 32 | grc_flip(lo); }
RF_HD bool grc_less(const grc_iv &a, const grc_iv &b) { return a.chr != b.chr ? a.chr < b.chr : a.pos1 != b.pos1 ? a.pos1 < b.pos1 : a.pos2 < b.pos2; }

// ---- searches.  [b, e) is a chr's segment; every result lies in [b, e]
RF_HD bool grc_segment(const grc_idx &X, int32_t chr, uint32_t *b, uint32_t *e)
{
    uint32_t lo = 0, hi = X.n_seg;          // the first segment with seg_chr >= chr
    while (lo < hi) { const uint32_t mid = (lo + hi) >> 1; if (X.seg_chr[mid] < chr) lo = mid + 1; else hi = mid; }
    if (lo == X.n_seg || X.seg_chr[lo] != chr) { *b = *e = 0; return false; }
    *b = X.seg_beg[lo]; *e = X.seg_beg[lo + 1];
    return true;
}
// the first i with a[i] > x (a ascending on [b, e))
RF_HD uint32_t grc_first_above(const int32_t *a, uint32_t b, uint32_t e, int32_t x)
{
    while (b < e) { const uint32_t mid = b + ((e - b) >> 1); if (a[mid] <= x) b = mid + 1; else e = mid; }
    return b;
}
// the first i with a[i] >= x
RF_HD uint32_t grc_first_at_least(const int32_t *a, uint32_t b, uint32_t e, int32_t x)
{
    while (b < e) { const uint32_t mid = b + ((e - b) >> 1); if (a[mid] < x) b = mid + 1; else e = mid; }
    return b;
}

// The candidates of query q: every subject that overlaps q lies in the sorted entries [lo, hi) -- hi the first entry of the chr with p1 > q.pos2, lo the first
// whose running maximum of p2 reaches q.pos1 (nothing before it ends at or after q.pos1).  seg: the chr's segment.
struct grc_cand { uint32_t lo, hi, seg_b, seg_e; };
RF_HD grc_cand grc_range(const grc_idx &X, const grc_iv &q)
{
    grc_cand c = {0, 0, 0, 0};
    uint32_t b, e;
    if (!grc_segment(X, q.chr, &b, &e)) return c;
    c.seg_b = b; c.seg_e = e;
    c.hi = grc_first_above(X.p1, b, e, q.pos2);
    c.lo = grc_first_at_least(X.run_p2, b, c.hi, q.pos1);
    return c;
}

// entry i of [lo, hi) against q: IntervalTree.h:198 (overlap; p1 <= q.pos2 holds for every candidate) and :224 (contained), the strand as
// GenomicRegionCollection.cpp:604
RF_HD bool grc_hit(const grc_idx &X, uint32_t i, const grc_iv &q, uint32_t flags)
{
    if (X.p2[i] < q.pos1) return false;
    if (!(flags & GRC_IGNORE_STRAND) && X.strand[i] != (uint8_t)q.strand) return false;
    if ((flags & GRC_CONTAINED) && (X.p1[i] < q.pos1 || X.p2[i] > q.pos2)) return false;
    return true;
}

// The number of hits of q.  Without a strand or containment test no candidate is looked at: #{p1 <= q.pos2} - #{p2 < q.pos1} over the chr, two binary searches
// (every interval has p1 <= p2 and q.pos1 <= q.pos2, so an interval with p2 < q.pos1 is among those with p1 <= q.pos2).  Otherwise the candidates are scanned.
RF_HD uint32_t grc_count(const grc_idx &X, const grc_iv &q, uint32_t flags, const grc_cand &C)
{
    if (C.lo >= C.hi) return 0;
    if (flags == GRC_IGNORE_STRAND) return (C.hi - C.seg_b) - (grc_first_at_least(X.ends, C.seg_b, C.seg_e, q.pos1) - C.seg_b);
    uint32_t c = 0;
    for (uint32_t i = C.lo; i < C.hi; ++i) c += grc_hit(X, i, q, flags) ? 1u : 0u;
    return c;
}

// one hit's outputs: the caller's index of the subject and the clipped interval (GenomicRegionCollection.cpp:608)
RF_HD void grc_put(const grc_idx &X, uint32_t i, const grc_iv &q, int32_t *sid, int32_t *c1, int32_t *c2)
{
    *sid = X.perm[i];
    *c1 = X.p1[i] > q.pos1 ? X.p1[i] : q.pos1;
    *c2 = X.p2[i] < q.pos2 ? X.p2[i] : q.pos2;
}

// the hits of q among [lo, hi) in sorted order, by one lane; returns how many (the count pass gave the same number).  sid / c1 / c2 may be null (ids only, or
// nothing but the number); at most cap are written
RF_HD uint64_t grc_fill(const grc_idx &X, const grc_iv &q, uint32_t flags, uint32_t lo, uint32_t hi, int32_t *sid, int32_t *c1, int32_t *c2, uint64_t cap)
{
    uint64_t k = 0;
    for (uint32_t i = lo; i < hi; ++i) {
        if (!grc_hit(X, i, q, flags)) continue;
        if (k < cap) {
            int32_t s, a, b;
            grc_put(X, i, q, &s, &a, &b);
            if (sid) sid[k] = s;
            if (c1) c1[k] = a;
            if (c2) c2[k] = b;
        }
        ++k;
    }
    return k;
}

// positions covered by n closed intervals whose starts ascend (a query's clipped hits are: they come in sorted order and the clip keeps it); 64-bit throughout
RF_HD uint64_t grc_width(const int32_t *c1, const int32_t *c2, uint64_t n)
{
    uint64_t w = 0;
    int64_t reach = 0;          // one past the last position counted
    for (uint64_t k = 0; k < n; ++k) {
        const int64_t a = c1[k], b = (int64_t)c2[k] + 1;
        const int64_t from = k && reach > a ? reach : a;
        if (b > from) { w += (uint64_t)(b - from); reach = b; }
    }
    return w;
}

// ---- merge (GenomicRegionCollection.cpp:267-306): sorted entry i starts a run when it is the first of its chr or starts past everything before it on the chr
RF_HD uint32_t grc_run_starts(const grc_idx &X, uint32_t i) { return i == 0 || X.chr[i] != X.chr[i - 1] || X.p1[i] > X.run_p2[i - 1] ? 1u : 0u; }

// ---- a record as a query: (tid, pos, end), end as the read filter has it, held to int32 (no subject starts past INT32_MAX, so the hits are the same)
RF_HD grc_iv grc_record_iv(const rf_feat &F)
{
    const int64_t e = rf_end(&F);
    grc_iv q;
    q.chr = F.tid; q.pos1 = F.pos; q.pos2 = e > 0x7fffffffll ? 0x7fffffff : (int32_t)e; q.strand = '*';
    return q;
}

// ---- the index on the host (host functions only): the mirror of the arrays in HBM, and the build of a host-only object.  std::stable_sort stands where the device
// build has hipCUB's stable radix sorts; the two must come out identical.
struct grc_host_arrays {
    std::vector<int32_t> chr, p1, p2, perm, run_p2, ends, seg_chr;
    std::vector<uint8_t> strand;
    std::vector<uint32_t> seg_beg;
    void resize(uint32_t n) { chr.resize(n); p1.resize(n); p2.resize(n); perm.resize(n); run_p2.resize(n); ends.resize(n); strand.resize(n); }
    grc_idx idx() const
    {
        return grc_idx{chr.data(), p1.data(), p2.data(), perm.data(), run_p2.data(), ends.data(), seg_chr.data(), strand.data(), seg_beg.data(), (uint32_t)chr.size(), (uint32_t)seg_chr.size()};
    }
};
// the per-chr segments from the sorted chr array (a collection has a few dozen)
static inline void grc_segments(grc_host_arrays &H)
{
    const uint32_t n = (uint32_t)H.chr.size();
    H.seg_chr.clear(); H.seg_beg.clear();
    for (uint32_t i = 0; i < n; ++i)
        if (i == 0 || H.chr[i] != H.chr[i - 1]) { H.seg_chr.push_back(H.chr[i]); H.seg_beg.push_back(i); }
    H.seg_beg.push_back(n);
}
static inline void grc_build_host(const grc_iv *v, uint32_t n, grc_host_arrays &H)
{
    H.resize(n);
    std::iota(H.perm.begin(), H.perm.end(), 0);
    std::stable_sort(H.perm.begin(), H.perm.end(), [v](int32_t a, int32_t b) { return grc_less(v[a], v[b]); });
    for (uint32_t i = 0; i < n; ++i) {
        const grc_iv &x = v[H.perm[i]];
        H.chr[i] = x.chr; H.p1[i] = x.pos1; H.p2[i] = x.pos2; H.strand[i] = (uint8_t)x.strand;
        H.run_p2[i] = i && H.chr[i - 1] == x.chr && H.run_p2[i - 1] > x.pos2 ? H.run_p2[i - 1] : x.pos2;
    }
    grc_segments(H);
    H.ends = H.p2;
    for (size_t k = 0; k + 1 < H.seg_beg.size(); ++k) std::sort(H.ends.begin() + H.seg_beg[k], H.ends.begin() + H.seg_beg[k + 1]);
}
