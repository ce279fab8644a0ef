// cov_host.h -- what the coverage unit (include/seqlib_amd_cov.h) computes per record and per position, compilable for host and device like dev_rfilter.h and
// dev_samw.h (`lane` of `nlanes` lanes that call together, with dev_lanes.h's collectives; the host build runs lane 0 of 1): the array layout, the eligibility test, the intervals a record contributes in the three modes,
// the decimal formatter and the piece of bedGraph text one position gives.  dev_cov.h's kernels, slx_cov_record_intervals and tests/cpp/cov_host_test.cpp (under
// ASan + UBSan) all go over these bodies.  The fixed fields and the record's end are the read filter's (dev_rfilter.h: rf_fixed, rf_end).
#pragma once
#include <stdint.h>
#include "dev_lanes.h"
#include "dev_rfilter.h"

#define COV_SPAN 0
#define COV_FULL 1
#define COV_ALIGNED 2

#define COV_R_BAD (-1)          // the record's fields pass its block_size, or its extent is not block_size + 4
#define COV_R_SKIP 0            // not eligible: contributes nothing
#define COV_R_COUNTED 1
#define COV_R_LONG 2            // eligible, with more than long_cigar ops: the wave's

struct cov_par { int32_t mode, buff, count_del, min_mapq; uint32_t exclude_flags, long_cigar; };
// per contig t: the positions [beg[t], end[t]) it keeps (the whole contig, the window, or nothing) and the entry off[t] of the one array where its
// end[t] - beg[t] + 1 entries start; total: entries of the array
struct cov_geo { const int64_t *beg, *end, *off; int32_t n_ref; int32_t pad; int64_t total; };
// the reference names one behind the other: name t is names[noff[t], noff[t + 1])
struct cov_names { const uint8_t *names; const uint32_t *noff; };

// ---- layout: contig t takes len[t] + 1 entries (the last one takes the -1 of an interval that ends at the contig's end), rounded up to 4 so that every contig
// starts on a 16-byte boundary; offsets are 64-bit (GRCh38: 3.1 G entries, 12.4 GB)
RF_HD uint64_t cov_entries(int64_t len) { return ((uint64_t)len + 1u + 3u) & ~3ull; }
RF_HD uint64_t cov_layout(const int64_t *len, int32_t n, int64_t *off)
{
    uint64_t at = 0;
    for (int32_t i = 0; i < n; ++i) { off[i] = (int64_t)at; at += cov_entries(len[i]); }
    return at;
}

// ---- decimal text
RF_HD uint32_t cov_dec_len(uint64_t v) { uint32_t n = 1; while (v >= 10) { v /= 10; ++n; } return n; }
RF_HD uint32_t cov_dec_put(uint8_t *o, uint64_t v)
{
    const uint32_t n = cov_dec_len(v);
    for (uint32_t i = n; i-- > 0;) { o[i] = (uint8_t)('0' + v % 10); v /= 10; }
    return n;
}
// a depth: int32, negative only after 2^31 reads on one position (counts do not saturate)
RF_HD uint32_t cov_depth_len(int32_t d) { return d < 0 ? 1 + cov_dec_len((uint64_t)(-(int64_t)d)) : cov_dec_len((uint64_t)d); }
RF_HD uint32_t cov_depth_put(uint8_t *o, int32_t d)
{
    if (d >= 0) return cov_dec_put(o, (uint64_t)d);
    o[0] = '-';
    return 1 + cov_dec_put(o + 1, (uint64_t)(-(int64_t)d));
}

// ---- one record
// the fixed fields and the verdict; F is the filter's feature block (reflen not yet set)
RF_HD int cov_head(const uint8_t *h, uint64_t span, const cov_par &P, int32_t n_ref, rf_feat *F)
{
    if (!rf_fixed(h, span, F)) return COV_R_BAD;
    if (F->tid < 0 || F->tid >= n_ref || F->pos < 0 || (F->flag & P.exclude_flags) || (int32_t)F->mapq < P.min_mapq) return COV_R_SKIP;
    return F->n_cig > P.long_cigar ? COV_R_LONG : COV_R_COUNTED;
}

// [lo, hi) of contig tid, clipped to what the contig keeps, to the sink
template <class Sink> RF_HD void cov_emit(const cov_geo &G, int32_t tid, int64_t lo, int64_t hi, Sink &S)
{
    const int64_t b = G.beg[tid], e = G.end[tid];
    if (lo < b) lo = b;
    if (hi > e) hi = e;
    if (lo < hi) S(tid, lo, hi);
}

// SLX_COV_SPAN and SLX_COV_FULL of a record whose reflen is known: STCoverage::addRead (src/non_api/STCoverage.cpp:44-109 of the reference), positions p..e with e
// included -- e is the record's end, one past its last aligned base: the reference's quirk, kept
template <class Sink> RF_HD void cov_span_full(const rf_feat &F, const cov_par &P, const cov_geo &G, Sink &S)
{
    int64_t p = F.pos, e = rf_end(&F);
    if (P.mode == COV_FULL) {
        if (F.n_cig) {          // the first and the last op only: H S M gets no extension, as in the reference
            const uint32_t w0 = rf_u32(F.cig), w1 = rf_u32(F.cig + 4ull * (F.n_cig - 1));
            if ((w0 & 15u) == 4u) { p -= (int64_t)(w0 >> 4); if (p < 0) p = 0; }
            if ((w1 & 15u) == 4u) e += (int64_t)(w1 >> 4);
        }
    } else { p += P.buff; e -= P.buff; }
    if (p < 0 || e < 0 || p > e) return;
    cov_emit(G, F.tid, p, e + 1, S);
}

// The intervals of an eligible record (cov_head said COUNTED or LONG), by `nlanes` lanes that call together: lane `lane` takes ops lane, lane + nlanes, ...;
// W.scan gives a block its start from the reference lengths of the ops before it, W.sum the reference length.  nlanes == 1 with lanes_one (dev_lanes.h) is the plain walk.
template <class Wave, class Sink> RF_HD void cov_record(const rf_feat &F0, const cov_par &P, const cov_geo &G, uint32_t lane, uint32_t nlanes, const Wave &W, Sink &S)
{
    if (P.mode != COV_ALIGNED) {
        rf_feat F = F0;
        uint64_t r = 0;
        for (uint32_t i = lane; i < F.n_cig; i += nlanes) {
            const uint32_t w = rf_u32(F.cig + 4ull * i);
            if ((0x18du >> (w & 15u)) & 1u) r += w >> 4;          // M D N = X
        }
        F.reflen = W.sum(r);
        if (lane == 0) cov_span_full(F, P, G, S);
        return;
    }
    int64_t x = F0.pos;
    const uint32_t covers = P.count_del ? 0x185u : 0x181u;          // M = X, and D on request; N advances without covering
    for (uint32_t base = 0; base < F0.n_cig; base += nlanes) {          // (uniform over the lanes)
        const uint32_t i = base + lane;
        const uint32_t w = i < F0.n_cig ? rf_u32(F0.cig + 4ull * i) : 0u, op = w & 15u, len = w >> 4;
        uint64_t total = 0;
        const uint64_t before = W.scan(((0x18du >> op) & 1u) ? (uint64_t)len : 0ull, &total);
        if ((covers >> op) & 1u) cov_emit(G, F0.tid, x + (int64_t)before, x + (int64_t)before + (int64_t)len, S);
        x += (int64_t)total;
    }
}

// ---- bedGraph: the text entry g of a settled array gives.  A position that starts a run of equal depth gives "name \t start \t", one that ends a run
// "end \t depth \n"; the pieces of all entries in order are the file.  The entries behind a contig's last position give nothing, nor do runs of depth 0
// unless include_zero.  o == nullptr: the length only.
RF_HD int32_t cov_contig_of(const cov_geo &G, uint64_t g)
{
    int32_t lo = 0, hi = G.n_ref;          // off[lo] <= g < off[hi]
    while (hi - lo > 1) { const int32_t mid = (lo + hi) >> 1; if ((uint64_t)G.off[mid] <= g) lo = mid; else hi = mid; }
    return lo;
}
RF_HD uint32_t cov_bg_piece(const int32_t *a, const cov_geo &G, const cov_names &N, uint64_t g, int include_zero, uint8_t *o, uint32_t *is_head)
{
    *is_head = 0;
    const int32_t t = cov_contig_of(G, g);
    const int64_t p = (int64_t)(g - (uint64_t)G.off[t]), L = G.end[t] - G.beg[t];
    if (p >= L) return 0;
    const int32_t d = a[g];
    if (d == 0 && !include_zero) return 0;
    const bool head = p == 0 || a[g - 1] != d, tail = p == L - 1 || a[g + 1] != d;
    uint32_t n = 0;
    if (head) {
        const uint32_t nl = N.noff[t + 1] - N.noff[t];
        *is_head = 1;
        if (o) {
            for (uint32_t i = 0; i < nl; ++i) o[i] = N.names[N.noff[t] + i];
            o[nl] = '\t';
            n = nl + 1;
            n += cov_dec_put(o + n, (uint64_t)(G.beg[t] + p));
            o[n++] = '\t';
        } else n = nl + 2 + cov_dec_len((uint64_t)(G.beg[t] + p));
    }
    if (tail) {
        if (o) {
            n += cov_dec_put(o + n, (uint64_t)(G.beg[t] + p + 1));
            o[n++] = '\t';
            n += cov_depth_put(o + n, d);
            o[n++] = '\n';
        } else n += cov_dec_len((uint64_t)(G.beg[t] + p + 1)) + cov_depth_len(d) + 2;
    }
    return n;
}
