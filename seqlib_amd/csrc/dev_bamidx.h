// dev_bamidx.h -- where the records of an inflated BAM stream start, without the serial walk: the per-chunk bodies of k_bam_guess, k_bam_round and
// k_bam_fill (slx_bam.hip).  A record's start is the previous start + 4 + block_size, one dependent chain over the whole file; the pattern is
// dev_ext_seg.h's: speculate, verify at the joins, recompute what fails.
//   guess   the stream is cut into chunks; every chunk but the first guesses its first record start: the first offset with a plausible header from which
//           three further plausible headers chain (or the stream ends); BIDX_NONE when no whole record starts in the chunk (it lies inside one long record)
//   walk    from an entry to the first start at or past the chunk's end: (exit, count)
//   round   chunk k compares the entry it was walked from with its predecessor's exit and walks again when they differ; rounds until nothing changes.
//           Chunk 0's entry is known, so after round r chunks 0..r hold the serial walk's values, and a state in which nothing changes has every chunk walked
//           from its predecessor's exit: by induction the serial walk's result.  The guess only decides how many rounds that takes.
// A record that the end of the stream cuts ends the walk: its start comes back with BIDX_CUT set and is carried to the next batch.
#pragma once
#include <stdint.h>
#if defined(__HIPCC__)
#define BIDX_FN __device__ __forceinline__
#define BIDX_HD __host__ __device__ __forceinline__
#else
#define BIDX_FN static inline
#define BIDX_HD static inline
#endif

#define BIDX_NONE 0xffffffffffffffffull
#define BIDX_CUT  0x8000000000000000ull

BIDX_HD uint32_t bidx_u32(const uint8_t *p) { return (uint32_t)p[0] | (uint32_t)p[1] << 8 | (uint32_t)p[2] << 16 | (uint32_t)p[3] << 24; }

// a plausible record header at off (off + 36 <= n): block_size covers what its fields imply, a name of at least the NUL, NUL-terminated where l_read_name
// says (when that byte is in the stream), both reference ids in [-1, n_ref)
BIDX_FN bool bidx_plausible(const uint8_t *s, uint64_t n, uint64_t off, int32_t n_ref, uint64_t &next)
{
    const uint8_t *h = s + off;
    const uint64_t bs = bidx_u32(h);
    const int32_t rid = (int32_t)bidx_u32(h + 4), mrid = (int32_t)bidx_u32(h + 24), l_seq = (int32_t)bidx_u32(h + 20);
    const uint32_t l_name = h[12], n_cig = (uint32_t)h[16] | (uint32_t)h[17] << 8;
    if (l_seq < 0 || l_name < 1) return false;
    if (rid < -1 || rid >= n_ref || mrid < -1 || mrid >= n_ref) return false;
    const uint64_t implied = 32ull + l_name + 4ull * n_cig + (((uint64_t)l_seq + 1) >> 1) + (uint64_t)l_seq;
    if (bs < implied) return false;
    const uint64_t nul = off + 36 + l_name - 1;
    if (nul < n && s[nul] != 0) return false;
    next = off + 4 + bs;
    return true;
}

BIDX_FN uint64_t bidx_guess(const uint8_t *s, uint64_t n, uint64_t cs, uint64_t ce, int32_t n_ref)
{
    for (uint64_t o = cs; o < ce && o + 36 <= n; ++o) {
        uint64_t q;
        if (!bidx_plausible(s, n, o, n_ref, q) || q > n) continue;          // the first record of the chain is whole: a lone header with a wild block_size proves nothing
        bool ok = true;
        for (int j = 0; j < 3 && ok; ++j) {
            if (q + 36 > n) break;              // the chain reaches the end of the stream
            ok = bidx_plausible(s, n, q, n_ref, q);
            if (ok && q > n) break;             // ... or the record that the end of the stream cuts
        }
        if (ok) return o;
    }
    return BIDX_NONE;
}

// records that start in [entry, ce): count, optionally their starts; returns the first start >= ce, or (start | BIDX_CUT) of the record the stream's end cuts.
// *bad: lowest start of a record whose block_size is below the 32 fixed bytes (malformed file), untouched otherwise.
BIDX_FN uint64_t bidx_walk(const uint8_t *s, uint64_t n, uint64_t entry, uint64_t ce, uint32_t &count, uint64_t *rec, uint64_t *bad)
{
    count = 0;
    if (entry & BIDX_CUT) return entry;
    uint64_t e = entry;
    while (e < ce) {
        if (e + 4 > n) return e | BIDX_CUT;
        const uint64_t bs = bidx_u32(s + e);
        if (e + 4 + bs > n) return e | BIDX_CUT;
        if (bs < 32 && bad && e < *bad) *bad = e;
        if (rec) rec[count] = e;
        ++count;
        e += 4 + bs;
    }
    return e;
}

// does the guess g of a chunk ending at ce agree with its true entry?  n_whole: whole records that start in the chunk ("none" = no whole record starts here:
// the chunk lies inside one long record, or holds only the start of the record that the end of the stream cuts)
BIDX_FN bool bidx_guess_right(uint64_t g, uint64_t entry, uint32_t n_whole)
{
    return g == entry || (g == BIDX_NONE && n_whole == 0);
}

// one round for chunk k >= 1: 1 when the chunk's state changed
BIDX_FN int bidx_round(const uint8_t *s, uint64_t n, uint64_t chunk, uint64_t k, uint64_t *used, const uint64_t *exit_prev, uint64_t *exit_next, uint32_t *count)
{
    const uint64_t e = exit_prev[k - 1];
    const uint64_t ce = (k + 1) * chunk < n ? (k + 1) * chunk : n;
    const uint64_t u = used[k];
    if (u == e || e == BIDX_NONE) { exit_next[k] = exit_prev[k]; return 0; }      // (BIDX_NONE as an exit: the predecessor is not resolved yet)
    if (u == BIDX_NONE && ((e & BIDX_CUT) || e >= ce)) {                            // "no record starts here" holds: the entry passes through
        const int ch = exit_prev[k] != e;
        exit_next[k] = e; count[k] = 0;
        return ch;
    }
    uint32_t c;
    used[k] = e;
    exit_next[k] = bidx_walk(s, n, e, ce, c, nullptr, nullptr);
    count[k] = c;
    return 1;
}
