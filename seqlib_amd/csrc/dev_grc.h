// dev_grc.h -- the kernels of the interval unit (slx_grc.hip launches them; grc_host.h has the per-interval and per-query bodies).  The index is a handful of
// sorted arrays (grc_idx), no pointer tree.  A join is a count pass (one lane per query: two or three binary searches, the exact count, and the job lists of the
// two fill forms), hipCUB's exclusive sum over the counts, and a fill pass that writes every query's hits at its offset in sorted order.  Every store to HBM is a
// plain store or an atomic from vector lanes.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "dev_lanes.h"
#include "grc_host.h"

typedef unsigned long long grc_ull;

// device counters of one join
enum { GRC_C_ERR = 0, GRC_C_NLANE, GRC_C_NWAVE, GRC_C_NLONG, GRC_C_N };

// lanes with `take` set get consecutive slots of a list whose length is *len: one atomic per wave.  Every lane of the wave calls.
__device__ __forceinline__ grc_ull grc_slot(bool take, grc_ull *len)
{
    const grc_ull mask = __ballot(take);
    const uint32_t lane = threadIdx.x & 63u;
    grc_ull base = 0;
    if (mask && lane == (uint32_t)(__ffsll((long long)mask) - 1)) base = atomicAdd(len, (grc_ull)__popcll(mask));
    base = (grc_ull)__shfl(base, mask ? __ffsll((long long)mask) - 1 : 0, 64);
    return base + (grc_ull)__popcll(mask & ((1ull << lane) - 1ull));
}

// ---- build: hipCUB sorts (index, flipped pos2), then (index, flipped (chr, pos1)) stably; these make the keys and gather the result
__global__ __launch_bounds__(256) void k_grc_key_p2(const grc_iv *iv, uint32_t n, uint32_t *key, uint32_t *val)
{
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) { key[i] = grc_flip(iv[i].pos2); val[i] = i; }
}
__global__ __launch_bounds__(256) void k_grc_key_chr_p1(const grc_iv *iv, const uint32_t *by_p2, uint32_t n, grc_ull *key)
{
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) { const grc_iv v = iv[by_p2[i]]; key[i] = grc_key2(v.chr, v.pos1); }
}
// the sorted arrays, and key[i] = (chr, p2) for the running maximum and the end-sorted array
__global__ __launch_bounds__(256) void k_grc_gather(const grc_iv *iv, const uint32_t *perm, uint32_t n, int32_t *chr, int32_t *p1, int32_t *p2, uint8_t *strand, int32_t *perm_out, grc_ull *key)
{
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const grc_iv v = iv[perm[i]];
    chr[i] = v.chr; p1[i] = v.pos1; p2[i] = v.pos2; strand[i] = (uint8_t)v.strand; perm_out[i] = (int32_t)perm[i];
    key[i] = grc_key2(v.chr, v.pos2);
}
// The maximum of (chr, p2) keys over a prefix of the sorted order is (the entry's chr, the largest p2 of that chr so far): chr ascends, so one plain max-scan is
// the segmented one.  The low halves of the scanned and of the sorted keys are run_p2 and ends.
__global__ __launch_bounds__(256) void k_grc_low_halves(const grc_ull *scanned, const grc_ull *sorted, uint32_t n, int32_t *run_p2, int32_t *ends)
{
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) { run_p2[i] = grc_unflip((uint32_t)scanned[i]); ends[i] = grc_unflip((uint32_t)sorted[i]); }
}

// ---- count pass: queries [q0, q1), one lane each.  cand[i] = its candidate range, cnt[i] = its hits (cnt[nq] is the scan's last item, set by the host).
// lists != 0: a query with hits goes to the lane list or, when its range is longer than wave_range (and wave_range < 2^20), to the wave list.
__global__ __launch_bounds__(256) void k_grc_count(grc_idx X, const grc_iv *q, grc_ull q0, grc_ull q1, uint32_t flags, uint32_t wave_range, int lists, uint2 *cand, uint32_t *cnt32,
                                                   grc_ull *cnt, uint32_t *lane_list, uint32_t *wave_list, grc_ull *ctr)
{
    const grc_ull i = q0 + (grc_ull)blockIdx.x * blockDim.x + threadIdx.x;
    uint32_t k = 0, len = 0;
    if (i < q1) {
        const grc_iv v = q[i];
        const grc_cand C = grc_range(X, v);
        k = grc_count(X, v, flags, C);
        cand[i] = make_uint2(C.lo, C.hi); cnt32[i] = k; cnt[i] = k;
        len = C.hi - C.lo;
    }
    if (!lists) return;
    const bool wave = k && wave_range < (1u << 20) && len > wave_range, lane = k && !wave;
    const grc_ull a = grc_slot(lane, &ctr[GRC_C_NLANE]), b = grc_slot(wave, &ctr[GRC_C_NWAVE]);
    if (lane) lane_list[a] = (uint32_t)i;
    if (wave) wave_list[b] = (uint32_t)i;
}

struct grc_out { int32_t *qid, *sid, *c1, *c2; };

// ---- fill pass, lane form: one lane per query of the list
__global__ __launch_bounds__(256) void k_grc_fill_lane(grc_idx X, const grc_iv *q, const uint32_t *list, grc_ull n_jobs, uint32_t flags, const uint2 *cand, const grc_ull *at, const uint32_t *cnt32,
                                                       grc_out O)
{
    const grc_ull j = (grc_ull)blockIdx.x * blockDim.x + threadIdx.x;
    if (j >= n_jobs) return;
    const uint32_t i = list[j];
    const grc_ull o = at[i];
    const uint64_t k = grc_fill(X, q[i], flags, cand[i].x, cand[i].y, O.sid + o, O.c1 + o, O.c2 + o, cnt32[i]);
    for (uint64_t t = 0; t < k && t < cnt32[i]; ++t) O.qid[o + t] = (int32_t)i;
}
// wave form: one wave per query of the list, 64 consecutive candidates a step (coalesced), a ballot, and the prefix popcount places a hit: sorted order is kept
__global__ __launch_bounds__(256) void k_grc_fill_wave(grc_idx X, const grc_iv *q, const uint32_t *list, grc_ull n_jobs, uint32_t flags, const uint2 *cand, const grc_ull *at, const uint32_t *cnt32,
                                                       grc_out O)
{
    const grc_ull j = (grc_ull)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (j >= n_jobs) return;          // (whole waves leave)
    const uint32_t i = list[j], lane = threadIdx.x & 63u;
    const grc_iv v = q[i];
    const uint2 c = cand[i];
    const grc_ull o = at[i], cap = cnt32[i];
    grc_ull done = 0;
    for (uint32_t base = c.x; base < c.y; base += 64) {          // (uniform over the wave)
        const uint32_t e = base + lane;
        const bool hit = e < c.y && grc_hit(X, e, v, flags);
        const grc_ull mask = __ballot(hit), k = done + (grc_ull)__popcll(mask & ((1ull << lane) - 1ull));
        if (hit && k < cap) {
            int32_t s, a, b;
            grc_put(X, e, v, &s, &a, &b);
            O.qid[o + k] = (int32_t)i; O.sid[o + k] = s; O.c1[o + k] = a; O.c2[o + k] = b;
        }
        done += (grc_ull)__popcll(mask);
        if (c.y - base <= 64) break;          // (base + 64 cannot wrap)
    }
}
// the width of every query from its own hit list
__global__ __launch_bounds__(256) void k_grc_width(grc_ull nq, const grc_ull *at, const uint32_t *cnt32, const int32_t *c1, const int32_t *c2, grc_ull *width)
{
    const grc_ull i = (grc_ull)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < nq) width[i] = grc_width(c1 + at[i], c2 + at[i], cnt32[i]);
}

// ---- records as queries: one lane per record; a record with more than long_cigar ops goes to long_list and a whole wave sums its CIGAR.  The lowest index of
// a record whose fields pass its block_size goes to ctr[GRC_C_ERR].  ks / ke: the (tid, pos) and (tid, end) keys of the per-subject counts.
__global__ __launch_bounds__(256) void k_grc_records(const uint8_t *s, grc_ull n_bytes, const grc_ull *rec_off, grc_ull n, uint32_t long_cigar, grc_iv *q, grc_ull *ks, grc_ull *ke,
                                                     uint32_t *long_list, grc_ull *ctr)
{
    const grc_ull k = (grc_ull)blockIdx.x * blockDim.x + threadIdx.x;
    bool is_long = false;
    if (k < n) {
        const grc_ull b = rec_off[k], e = rec_off[k + 1];
        rf_feat F;
        if (!(b <= e && e <= n_bytes && rf_fixed(s + b, e - b, &F))) {
            atomicMin(&ctr[GRC_C_ERR], k);
            memset(&F, 0, sizeof F);          // (the call fails; the entry is still a valid interval)
        } else if (F.n_cig > long_cigar) is_long = true;
        else {
            rf_part P;
            memset(&P, 0, sizeof P);
            rf_cigar_part(F.cig, 0, F.n_cig, 1, &P);
            F.reflen = P.reflen;
        }
        if (!is_long) { const grc_iv v = grc_record_iv(F); q[k] = v; ks[k] = grc_key2(v.chr, v.pos1); ke[k] = grc_key2(v.chr, v.pos2); }
    }
    const grc_ull a = grc_slot(is_long, &ctr[GRC_C_NLONG]);
    if (is_long) long_list[a] = (uint32_t)k;
}
__global__ __launch_bounds__(256) void k_grc_records_long(const uint8_t *s, const grc_ull *rec_off, const uint32_t *long_list, grc_ull m, grc_iv *q, grc_ull *ks, grc_ull *ke)
{
    const grc_ull j = (grc_ull)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (j >= m) return;          // (whole waves leave)
    const uint32_t k = long_list[j];
    const grc_ull b = rec_off[k];
    rf_feat F;
    (void)rf_fixed(s + b, rec_off[k + 1] - b, &F);          // (k_grc_records took it: the fields are inside the record)
    rf_part P;
    memset(&P, 0, sizeof P);
    rf_cigar_part(F.cig, threadIdx.x & 63u, F.n_cig, 64, &P);
    F.reflen = wave_sum((grc_ull)P.reflen);
    if ((threadIdx.x & 63u) == 0) { const grc_iv v = grc_record_iv(F); q[k] = v; ks[k] = grc_key2(v.chr, v.pos1); ke[k] = grc_key2(v.chr, v.pos2); }
}

// the first index of a[0, n) with a[i] >= x
__device__ __forceinline__ grc_ull grc_key_lower(const grc_ull *a, grc_ull n, grc_ull x)
{
    grc_ull b = 0, e = n;
    while (b < e) { const grc_ull mid = b + ((e - b) >> 1); if (a[mid] < x) b = mid + 1; else e = mid; }
    return b;
}
// Per-subject record counts without atomics: ks / ke are the batch's start and end keys sorted.  For subject i: the records of its chr, less those that start
// past its p2, less those that end before its p1 (a record's start is not past its end, so no record is in both).  One lane per subject adds to its own entry.
__global__ __launch_bounds__(256) void k_grc_subject_counts(grc_idx X, const grc_ull *ks, const grc_ull *ke, grc_ull n_rec, long long *counts)
{
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= X.n) return;
    const int32_t chr = X.chr[i];
    const grc_ull first = grc_key2(chr, INT32_MIN), k2 = grc_key2(chr, X.p2[i]);
    const grc_ull s0 = grc_key_lower(ks, n_rec, first);
    const grc_ull start_le = (k2 == ~0ull ? n_rec : grc_key_lower(ks, n_rec, k2 + 1)) - s0;          // records of chr with start <= p2
    const grc_ull end_lt = grc_key_lower(ke, n_rec, grc_key2(chr, X.p1[i])) - grc_key_lower(ke, n_rec, first);
    const grc_ull c = start_le - end_lt;
    if (c) counts[X.perm[i]] += (long long)c;
}

// ---- merge: flag[i] = entry i starts a run (flag[n] = 0); with at = the exclusive sum of flag, run r = at[i] + flag[i] - 1 takes chr, pos1 and strand from its
// first entry and pos2 = the running maximum at its last
__global__ __launch_bounds__(256) void k_grc_merge_flag(grc_idx X, grc_ull *flag)
{
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i < X.n) flag[i] = grc_run_starts(X, i);
    else if (i == X.n) flag[i] = 0;
}
__global__ __launch_bounds__(256) void k_grc_merge_fill(grc_idx X, const grc_ull *flag, const grc_ull *at, grc_iv *out)
{
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= X.n) return;
    const grc_ull r = at[i] + flag[i] - 1;
    if (flag[i]) { out[r].chr = X.chr[i]; out[r].pos1 = X.p1[i]; out[r].strand = (char)X.strand[i]; }
    if (i == X.n - 1 || flag[i + 1]) out[r].pos2 = X.run_p2[i];
}
