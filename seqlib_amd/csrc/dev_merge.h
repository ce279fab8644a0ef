// dev_merge.h -- the k-way merge of coordinate-sorted record streams in HBM: the bodies of k_merge_key, k_merge_elig, k_merge_rank and k_merge_place
// (slx_merge.hip).  Host-compilable like dev_recsort.h, whose rs_key and rs_gather_tile it builds on, so that tests/cpp/merge_host_test.cpp can drive a whole
// merge through them under ASan + UBSan before they run on a GPU.  DESIGN.md section 9.17.
//
// The data is sorted already, so nothing is sorted: every eligible record computes where it goes.
//   key    per record of a batch read from one input: rs_key (block_size against the offsets, the 64-bit key, the length), and the order test -- a key below
//          its predecessor's is named; the predecessor of a batch's first record is the last key of the batch before, which comes in as an argument
//   table  the keys of all windows lie side by side in ONE table: input i's window is keys[beg[i], beg[i + 1]), its eligible prefix (key < the round's bound)
//          the first elig[i] of them; ebeg[] is the running sum of elig[].  beg and ebeg have k + 1 entries and live in LDS.
//   elig   per input one wave: lower_bound of the bound in the window, by the cooperative search
//   rank   one lane per eligible record g = ebeg[i] + j:
//              rank = j + sum over r < i of upper_bound(keys_r[0, elig_r), key) + sum over r > i of lower_bound(keys_r[0, elig_r), key)
//          -- records of earlier inputs with an equal key go first, those of later inputs after: the stable order.  Not k - 1 full binary searches per lane: the
//          lanes of a wave hold consecutive g, so their keys are consecutive and sorted (inside an input; a wave that straddles inputs takes the wave-wide minimum
//          and maximum).  Per other input the WAVE brackets once -- lower_bound of its smallest key, upper_bound of its largest, each by the cooperative search
//          of rs_gather_tile (nlanes evenly spaced probes per step and a count, the interval shrinks (nlanes + 1)-fold per round trip) -- and each lane then
//          searches inside the bracket only, which is normally a few entries.
//   place  lengths, source addresses and input indices scattered to their ranks; rs_gather_tile (dev_recsort.h) takes it from there.
//
// A wave on the host.  The collectives (a count over the lanes, a minimum, a maximum) make a body more than "lane 0 of 1".  The bodies are written over per-lane
// SLOTS: on the GPU a lane has one slot and MG_EACH runs once; on the host one call plays all nlanes lanes (1 or 64), MG_EACH loops over them, and the
// collectives loop over the slots.  The text between two collectives is the same on both.
// Memory safety: every index into keys[] is below beg[k]; a probe is read only where it is below the interval's end; every rank is below ebeg[k] (the sum of
// the counts of disjoint sets of eligible records); LDS indices are below k + 1 <= MG_MAX_IN + 1.
#pragma once
#include <stdint.h>
#include "dev_lanes.h"
#include "dev_recsort.h"

#define MG_MAX_IN 64            // inputs of one merger
#define MG_NONE (~0ull)

#if defined(__HIPCC__)
#define MG_LDS __attribute__((address_space(3)))
#define MG_SLOTS 1
#define MG_EACH(l, nlanes) for (int l = 0; l < 1; ++l)
#define MG_ID(l, lane) (lane)
#else
#define MG_LDS
#define MG_SLOTS 64
#define MG_EACH(l, nlanes) for (int l = 0; l < (nlanes); ++l)
#define MG_ID(l, lane) (l)
#endif

typedef unsigned long long mg_ull;

// ---- the collectives over the (whole) wave
RS_FN uint32_t mg_count(const bool *p, int nlanes)
{
#if defined(__HIPCC__)
    return (uint32_t)__popcll(__ballot(p[0]));
#else
    uint32_t c = 0;
    for (int l = 0; l < nlanes; ++l) c += p[l] ? 1u : 0u;
    return c;
#endif
}
RS_FN mg_ull mg_min(const mg_ull *v, int nlanes)
{
#if defined(__HIPCC__)
    return wave_min(v[0]);
#else
    mg_ull m = v[0];
    for (int l = 1; l < nlanes; ++l) m = v[l] < m ? v[l] : m;
    return m;
#endif
}
RS_FN mg_ull mg_max(const mg_ull *v, int nlanes)
{
#if defined(__HIPCC__)
    return wave_max(v[0]);
#else
    mg_ull m = v[0];
    for (int l = 1; l < nlanes; ++l) m = v[l] > m ? v[l] : m;
    return m;
#endif
}

// ---- key and order test
// Record i of the n of a batch: rs_key's verdict (false = record i is the one to name as broken).  *unsorted: its key is below its predecessor's -- record i - 1
// of the batch where that one's span can be read, for i = 0 prev_last when has_prev.
RS_FN bool mg_key(const uint8_t *stream, uint64_t n_bytes, const uint64_t *off, uint64_t i, uint64_t n, bool has_prev, uint64_t prev_last, uint64_t *key, uint32_t *len, bool *unsorted)
{
    *unsorted = false;
    if (!rs_key(stream, n_bytes, off, i, n, key, len)) return false;
    if (i == 0) { *unsorted = has_prev && *key < prev_last; return true; }
    const uint64_t z = off[i - 1], a = off[i];
    if (rs_span_ok(z, a, n_bytes)) {          // (a span that is not is named by lane i - 1)
        const uint8_t *p = stream + z;
        const uint64_t pk = (uint64_t)rs_ld32(p + 4) << 32 | (uint64_t)(rs_ld32(p + 8) ^ 0x80000000u);
        *unsorted = *key < pk;
    }
    return true;
}

// ---- the searches
// The first x of [lo, hi) with keys[x] >= t (upper = false) or keys[x] > t (upper = true), hi when there is none; keys rise.  lo, hi and t are the same in
// every lane: the wave probes nlanes places per step.  All lanes of the wave take part.
RS_FN uint64_t mg_coop_bound(const mg_ull *keys, uint64_t lo, uint64_t hi, mg_ull t, bool upper, int lane, int nlanes)
{
    while (hi > lo) {
        const uint64_t step = (hi - lo + (uint64_t)nlanes) / ((uint64_t)nlanes + 1);          // >= 1; the probes lo + step - 1, lo + 2 step - 1, ...: those below hi count
        bool p[MG_SLOTS];
        MG_EACH(l, nlanes) {
            const uint64_t probe = lo + (uint64_t)(MG_ID(l, lane) + 1) * step - 1;
            p[l] = probe < hi && (upper ? keys[probe] <= t : keys[probe] < t);
        }
        const uint64_t c = mg_count(p, nlanes);          // the probes rise with the lane: the lanes that are still in front of the bound are the first c
        lo += c * step;
        if (c < (uint64_t)nlanes && lo + step - 1 < hi) hi = lo + step - 1;          // (the probe behind them was made and is at or past the bound, or lies at or past hi)
    }
    return lo;
}
// the same for one lane alone
RS_FN uint64_t mg_bound(const mg_ull *keys, uint64_t lo, uint64_t hi, mg_ull t, bool upper)
{
    while (hi > lo) {
        const uint64_t mid = lo + ((hi - lo) >> 1);
        if (upper ? keys[mid] <= t : keys[mid] < t) lo = mid + 1; else hi = mid;
    }
    return lo;
}

// the input of eligible record g: the i with ebeg[i] <= g < ebeg[i + 1] (inputs with nothing eligible are stepped over); g < ebeg[k]
RS_FN int mg_input_of(const MG_LDS uint32_t *ebeg, int k, uint64_t g)
{
    int a = 0, b = k;          // ebeg[a] <= g < ebeg[b]
    while (b - a > 1) {
        const int mid = (a + b) >> 1;
        if ((uint64_t)ebeg[mid] <= g) a = mid; else b = mid;
    }
    return a;
}

// ---- elig: how many of keys[0, n) lie below the bound (infinite: all of them).  One wave per input.
RS_FN uint32_t mg_elig(const mg_ull *keys, uint64_t n, bool finite, mg_ull bound, int lane, int nlanes)
{
    return (uint32_t)(finite ? mg_coop_bound(keys, 0, n, bound, false, lane, nlanes) : n);
}

// ---- rank: the wave whose first eligible record is g0 writes rank[g] for g in [g0, g0 + nlanes) below E = ebeg[k]
RS_FN void mg_rank_wave(const mg_ull *keys, const MG_LDS uint32_t *beg, const MG_LDS uint32_t *ebeg, int k, uint64_t g0, uint32_t *rank, int lane, int nlanes)
{
    const uint64_t E = ebeg[k];
    bool act[MG_SLOTS];
    int inp[MG_SLOTS];
    mg_ull key[MG_SLOTS], lo_k[MG_SLOTS], hi_k[MG_SLOTS], lo_i[MG_SLOTS], hi_i[MG_SLOTS];
    uint64_t r[MG_SLOTS];
    MG_EACH(l, nlanes) {
        const uint64_t g = g0 + (uint64_t)MG_ID(l, lane);
        act[l] = g < E;
        inp[l] = 0; key[l] = 0; r[l] = 0;
        if (act[l]) {
            inp[l] = mg_input_of(ebeg, k, g);
            r[l] = g - ebeg[inp[l]];
            key[l] = keys[(uint64_t)beg[inp[l]] + r[l]];
        }
        lo_k[l] = act[l] ? key[l] : MG_NONE; hi_k[l] = act[l] ? key[l] : 0;
        lo_i[l] = act[l] ? (mg_ull)inp[l] : MG_NONE; hi_i[l] = act[l] ? (mg_ull)inp[l] : 0;
    }
    if (g0 >= E) return;          // (the whole wave)
    const mg_ull kmin = mg_min(lo_k, nlanes), kmax = mg_max(hi_k, nlanes);
    const int i_first = (int)mg_min(lo_i, nlanes), i_last = (int)mg_max(hi_i, nlanes);
    for (int q = 0; q < k; ++q) {
        const uint64_t n = (uint64_t)ebeg[q + 1] - ebeg[q];
        if (n == 0 || (q == i_first && q == i_last)) continue;          // nothing eligible there, or the wave's own input: j is its share
        const mg_ull *kq = keys + beg[q];
        // every lane's bound lies in [lower_bound(kmin), upper_bound(kmax)]
        const uint64_t lo = mg_coop_bound(kq, 0, n, kmin, false, lane, nlanes);
        const uint64_t hi = mg_coop_bound(kq, lo, n, kmax, true, lane, nlanes);
        MG_EACH(l, nlanes) if (act[l] && inp[l] != q) r[l] += mg_bound(kq, lo, hi, key[l], q < inp[l]);
    }
    MG_EACH(l, nlanes) if (act[l]) rank[g0 + (uint64_t)MG_ID(l, lane)] = (uint32_t)r[l];
}

// ---- place: eligible record g to its rank.  The ranks are a permutation of [0, E); a rank that is not below E (it cannot be) stores nothing.
RS_FN void mg_place(const MG_LDS uint32_t *beg, const MG_LDS uint32_t *ebeg, int k, uint64_t g, const uint32_t *rank, const uint32_t *len, const mg_ull *src,
                    mg_ull *slen, mg_ull *ssrc, uint8_t *input)
{
    const int i = mg_input_of(ebeg, k, g);
    const uint64_t at = (uint64_t)beg[i] + (g - ebeg[i]);
    const uint32_t r = rank[g];
    if (r >= ebeg[k]) return;
    slen[r] = len[at]; ssrc[r] = src[at]; input[r] = (uint8_t)i;
}
