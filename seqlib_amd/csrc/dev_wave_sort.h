// dev_wave_sort.h -- one wave sorts up to a few thousand slots of an LDS array with a compare-exchange network.
//
// The many-region reads' handle lists (dev_fin.h, sort_handles) and the many-hit reads' hit lists (k_hits_wave, dev_fin2.h) were ordered by
// counting, for every element, the elements before it: m * m / 64 steps per lane, each a chain of dependent LDS reads.  The network below
// needs log2(m) * (log2(m) + 1) / 2 stages of m / 128 exchanges per lane: 45 stages of 4 at m = 512, 66 of 16 at m = 2 048.
//
// It is the merge form of the bitonic sorter in which EVERY exchange is ascending: a block of k slots is merged from its two sorted halves
// by first pairing slot i of the lower half with its mirror in the upper half (block end - offset), then halving the stride inside each
// half as usual.  Because no exchange ever moves the larger element down, slots at or beyond m behave as +infinity without being there: an
// exchange whose upper partner is >= m is skipped, and m needs no padding to a power of two.  Nothing at or beyond m is read or written.
//
// The order is the caller's strict `less` over what `load` returns (a handle, or a whole record); a network is not stable, and the callers'
// serial sorts (klib's introsort, std::sort) are not either, so a result is only used when no two elements are equal: wave_sort_tie looks at
// the sorted neighbours, and with a tie the caller sorts again, serially, from the order it saved.
//
// Between stages the lanes must see each other's stores: `sync` is the caller's ordering for ONE wave (a block barrier in a 64-thread block;
// a workgroup fence + wave barrier where the wave runs inside a larger block).  Host-compilable (tests/cpp/wave_sort_test.cpp): there the 64
// lanes are a loop around wave_sort_stage, stage by stage.
#pragma once
#include <stdint.h>
#if defined(__HIPCC__)
#define WSORT_FN __host__ __device__ __forceinline__
#else
#define WSORT_FN static inline
#endif

#define WSORT_LANES 64
#ifndef WSORT_UNROLL
#define WSORT_UNROLL 4          // exchanges of a lane whose LDS reads are in flight together
#endif

// one stage of the network: blocks of 2 * j slots, slot `off` of the lower half against the mirror slot of the upper half (mirror) or against off + j
struct WaveSortStage { int k, j; };          // k = size of the blocks being merged, j = half the size of this stage's sub-blocks (j == k / 2: the mirror stage)

WSORT_FN WaveSortStage wave_sort_begin() { WaveSortStage s; s.k = 1; s.j = 0; return s; }
// advances to the next stage; false when slots [0, m) are sorted
WSORT_FN bool wave_sort_next(int m, WaveSortStage &s)
{
    if (s.j > 1) { s.j >>= 1; return true; }
    if (s.k >= m) return false;
    s.k <<= 1; s.j = s.k >> 1;
    return true;
}

// the exchanges of `lane` in stage s: pair t -> slots (i, p), i < p; a pair whose p is beyond the list is skipped (p holds +infinity)
template <typename LOAD, typename STORE, typename LESS>
WSORT_FN void wave_sort_stage(int m, WaveSortStage s, int lane, LOAD load, STORE store, LESS less)
{
    const int j = s.j, two_j = j << 1;
    const bool mirror = j == (s.k >> 1);
    const int lj = 31 - __builtin_clz((unsigned)j);
    typedef decltype(load(0)) V;
    // WSORT_UNROLL exchanges at a time: all their loads, then all their comparisons (which may read keys through what was loaded), then the
    // stores -- the pairs of a stage are disjoint, and a lane that waits for one LDS read at a time spends the stage waiting
    for (int t0 = lane;; t0 += WSORT_UNROLL * WSORT_LANES) {
        int i[WSORT_UNROLL], p[WSORT_UNROLL];
        bool on[WSORT_UNROLL], sw[WSORT_UNROLL];
        V a[WSORT_UNROLL] = {}, b[WSORT_UNROLL] = {};
#pragma unroll
        for (int u = 0; u < WSORT_UNROLL; ++u) {
            const int t = t0 + u * WSORT_LANES;
            const int base = (t >> lj) * two_j, off = t & (j - 1);
            i[u] = base + off;                              // (grows with t)
            p[u] = mirror ? base + two_j - 1 - off : i[u] + j;
            on[u] = p[u] < m;                               // (i < p)
        }
        if (i[0] >= m) break;
#pragma unroll
        for (int u = 0; u < WSORT_UNROLL; ++u) if (on[u]) { a[u] = load(i[u]); b[u] = load(p[u]); }
#pragma unroll
        for (int u = 0; u < WSORT_UNROLL; ++u) sw[u] = on[u] && less(b[u], a[u]);
#pragma unroll
        for (int u = 0; u < WSORT_UNROLL; ++u) if (sw[u]) { store(i[u], b[u]); store(p[u], a[u]); }
    }
}

// sorts slots [0, m) ascending by `less`; every lane of the wave calls it with the same m.  Ends with a sync: the order is there for every lane.
template <typename LOAD, typename STORE, typename LESS, typename SYNC>
WSORT_FN void wave_sort(int m, int lane, LOAD load, STORE store, LESS less, SYNC sync)
{
    for (WaveSortStage s = wave_sort_begin(); wave_sort_next(m, s);) {
        wave_sort_stage(m, s, lane, load, store, less);
        sync();
    }
}

// after the sort: does this lane see two neighbours of which neither is less than the other?  (The wave's answer is the OR over its lanes.)
template <typename LOAD, typename LESS>
WSORT_FN bool wave_sort_tie(int m, int lane, LOAD load, LESS less)
{
    bool tie = false;
    for (int i = lane; i + 1 < m; i += WSORT_LANES) {
        const auto a = load(i);
        const auto b = load(i + 1);
        if (!less(a, b) && !less(b, a)) tie = true;
    }
    return tie;
}
