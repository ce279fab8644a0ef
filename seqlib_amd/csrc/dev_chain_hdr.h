// dev_chain_hdr.h -- what the extension walk (k_extend_reg, dev_ext_reg.h) needs of a chain before it takes its first seed, made by ONE lane.
// The walk replays mem_chain2aln chain by chain on a whole wave, and every chain begins with a string of dependent loads that 63 lanes
// only wait for: handle -> seed count and first seed -> seed list -> seeds -> wave min / max -> contig search -> contig bounds.  With
// walk_stage = 1 the wave makes the headers of 64 chains at a time instead, lane L for chain ci0 + L, so that 64 such strings are in flight
// at once, and leaves them in LDS where the walk picks them up:
//     the reference window [rmax0, rmax1) -- cal_max_gap on both sides of every seed, the l_pac straddle rule by the chain's first seed,
//     the clip to the first seed's contig on its strand (bns_fetch_seq) --
//     and the chain's top seed: the one mem_chain2aln takes first, the largest (score, list index).
// A chain of one seed needs nothing else: no sort, no sorted-seed scratch, and its seedcov is the containment test on that one seed
// (chain_hdr_seedcov1: the general loop of mem_chain2aln over a list of one, NOT the assumption that a region contains its seed).
// A lane whose chain has more than CHDR_MAX_SEEDS seeds leaves the header unmade and the wave computes it as before.
// Host-compilable (tests/cpp/chain_hdr_test.cpp): seeds and the gap table come in through two small policies.
#pragma once
#include <stdint.h>
#if defined(__HIPCC__)
#define CHDR_FN __host__ __device__ __forceinline__
#else
#define CHDR_FN static inline
#endif

#define CHDR_MAX_SEEDS 8        // seeds a lane walks for its chain's header (the walk of a lane is serial: the longest chain of the 64 sets the time)

struct ChainHdr {
    int64_t rmax0, rmax1;       // the chain's reference window, clipped
    int64_t top_rbeg;           // the top seed
    int top_qbeg, top_len, top_s;   // ... its query start, length and seed slot
    int rid;                    // contig of the chain's first seed (what the clip used)
};

// bns_pos2rid
CHDR_FN int chain_hdr_pos2rid(int64_t l_pac, int n_seqs, const int64_t *ann_off, int64_t pos_f)
{
    if (pos_f >= l_pac) return -1;
    int left = 0, mid = 0, right = n_seqs;
    while (left < right) {
        mid = (left + right) >> 1;
        if (pos_f >= ann_off[mid]) {
            if (mid == n_seqs - 1) break;
            if (pos_f < ann_off[mid + 1]) break;
            left = mid + 1;
        } else right = mid;
    }
    return mid;
}

// What follows the min / max over a chain's seeds: the clamps to the coordinate space, the l_pac straddle rule by the chain's first seed, and
// bns_fetch_seq's clip to that seed's contig on its strand.  Returns the contig.  (The wave's own window computation in k_extend_reg ends in this too.)
CHDR_FN int chain_hdr_clip(int64_t &rmax0, int64_t &rmax1, int64_t first_rbeg, int64_t l_pac, int n_seqs, const int64_t *ann_off, const int32_t *ann_len)
{
    rmax0 = rmax0 > 0 ? rmax0 : 0;
    rmax1 = rmax1 < l_pac << 1 ? rmax1 : l_pac << 1;
    if (rmax0 < l_pac && l_pac < rmax1) {
        if (first_rbeg < l_pac) rmax1 = l_pac; else rmax0 = l_pac;
    }
    const int is_rev = first_rbeg >= l_pac;
    const int rid = chain_hdr_pos2rid(l_pac, n_seqs, ann_off, is_rev ? (l_pac << 1) - 1 - first_rbeg : first_rbeg);
    int64_t far_beg = ann_off[rid], far_end = far_beg + ann_len[rid];
    if (is_rev) { const int64_t t = far_beg; far_beg = (l_pac << 1) - far_end; far_end = (l_pac << 1) - t; }
    rmax0 = rmax0 > far_beg ? rmax0 : far_beg;
    rmax1 = rmax1 < far_end ? rmax1 : far_end;
    return rid;
}

// S: the read's seeds by slot -- qbeg(s), len(s), rbeg(s), score(s) (mem_seed_t::score).  G: gap(q) = cal_max_gap(opt, q).
// cs[0 .. n): the chain's seed slots in list order.  false (header unmade) when n is outside 1 .. CHDR_MAX_SEEDS.
template <typename S, typename G>
CHDR_FN bool chain_hdr_make(ChainHdr &h, const int *cs, int n, const S &sd, const G &gap, int l_query, int64_t l_pac, int n_seqs,
                            const int64_t *ann_off, const int32_t *ann_len)
{
    if (n < 1 || n > CHDR_MAX_SEEDS) return false;
    int64_t rmax0 = l_pac << 1, rmax1 = 0, first_rbeg = 0;
    uint64_t best = 0;
    h.top_s = cs[0];
    for (int i = 0; i < n; ++i) {
        const int s = cs[i];
        const int qb = sd.qbeg(s), sl = sd.len(s);
        const int64_t rb = sd.rbeg(s);
        const int64_t b = rb - (qb + gap(qb));
        const int64_t e = rb + sl + ((l_query - qb - sl) + gap(l_query - qb - sl));
        rmax0 = rmax0 < b ? rmax0 : b;
        rmax1 = rmax1 > e ? rmax1 : e;
        if (i == 0) first_rbeg = rb;
        const uint64_t key = (uint64_t)(uint32_t)sd.score(s) << 32 | (uint64_t)(uint32_t)i;      // the sorted loop takes the largest (score, list index) first
        if (key >= best) { best = key; h.top_s = s; h.top_qbeg = qb; h.top_len = sl; h.top_rbeg = rb; }
    }
    h.rid = chain_hdr_clip(rmax0, rmax1, first_rbeg, l_pac, n_seqs, ann_off, ann_len);
    h.rmax0 = rmax0; h.rmax1 = rmax1;
    return true;
}

// seedcov of a region of a one-seed chain: mem_chain2aln's loop over the chain's seeds, for a list of one
CHDR_FN int chain_hdr_seedcov1(int s_qbeg, int s_len, int64_t s_rbeg, int a_qb, int a_qe, int64_t a_rb, int64_t a_re)
{
    return (s_qbeg >= a_qb && s_qbeg + s_len <= a_qe && s_rbeg >= a_rb && s_rbeg + s_len <= a_re) ? s_len : 0;
}
