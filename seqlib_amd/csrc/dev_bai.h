// dev_bai.h -- the per-record bodies of the BAI build and of the region filter (k_bai_rec, k_bai_heads, k_bai_chunks, k_bai_fill, k_bam_region_keep in
// slx_bam.hip), next to dev_bamidx.h whose record offsets they start from.  SAMv1 section 5.2 / 5.3; the rules are listed in include/seqlib_amd_bam.h.
//   end of a record   pos + reference length of the CIGAR (M D N = X), pos + 1 when that is 0 or the record carries 0x4.  One lane owns one record, which is
//                     right for the two or three ops of a short read and wrong for a long read's thousands: a lane whose record has more than
//                     BAI_COOP_OPS ops leaves it out, and the wave then takes those records one at a time, all 64 lanes striding over the ops with a
//                     shuffle reduction (bai_reflen_wave).  No queue, no second launch: the long records are found by a ballot inside the wave.
//   virtual offset    of whole-file inflated offset x: binary search in the exclusive ISIZE sum of the non-empty members (uploaded once)
// Every read of a record's variable part is checked against its block_size; the index (dev_bamidx.h) has already placed the whole record inside the stream.
#pragma once
#include "dev_bamidx.h"
#include "dev_lanes.h"

#define BAI_COOP_OPS   64u
#define BAI_COOP_WINS  64u
#define BAI_NOKEY      0xffffffffffffffffull
// error bits of a build / a region pass (state word): a record whose CIGAR passes its block_size, a reference id outside the header, a record past the
// windows of its reference
#define BAI_E_CIGAR 1ull
#define BAI_E_TID   2ull
#define BAI_E_SPAN  4ull

BIDX_HD uint32_t bai_reg2bin(int64_t beg, int64_t end)
{
    --end;
    if (beg >> 14 == end >> 14) return (uint32_t)(4681 + (beg >> 14));
    if (beg >> 17 == end >> 17) return (uint32_t)(585 + (beg >> 17));
    if (beg >> 20 == end >> 20) return (uint32_t)(73 + (beg >> 20));
    if (beg >> 23 == end >> 23) return (uint32_t)(9 + (beg >> 23));
    if (beg >> 26 == end >> 26) return (uint32_t)(1 + (beg >> 26));
    return 0;
}

// reference length of the ops first, first + stride, ... below n
BIDX_HD uint64_t bai_reflen_part(const uint8_t *cig, uint32_t first, uint32_t n, uint32_t stride)
{
    uint64_t sum = 0;
    for (uint32_t i = first; i < n; i += stride) {
        const uint32_t w = bidx_u32(cig + 4ull * i);
        if ((0x18du >> (w & 15u)) & 1u) sum += w >> 4;          // M D N = X
    }
    return sum;
}

struct bai_fields { int32_t tid, pos; uint32_t flag, n_cig; const uint8_t *cig; bool ok; };

// h: a whole record in the stream, its block_size word (>= 32) first.  ok = false (and no ops) when the name and the CIGAR do not fit the block_size.
BIDX_HD bai_fields bai_read(const uint8_t *h)
{
    bai_fields f;
    const uint64_t bs = bidx_u32(h);
    const uint32_t l_name = h[12];
    f.tid = (int32_t)bidx_u32(h + 4); f.pos = (int32_t)bidx_u32(h + 8);
    f.n_cig = (uint32_t)h[16] | (uint32_t)h[17] << 8; f.flag = (uint32_t)h[18] | (uint32_t)h[19] << 8;
    f.cig = h + 36 + l_name;
    f.ok = 32ull + l_name + 4ull * f.n_cig <= bs;
    if (!f.ok) f.n_cig = 0;
    return f;
}

BIDX_HD int64_t bai_end(int64_t pos, uint32_t flag, uint64_t reflen) { return pos + (int64_t)((flag & 4u) || reflen == 0 ? 1 : reflen); }

#if defined(__HIPCC__)
// the reference length of every lane's record.  All 64 lanes of the wave call it together (active = the lane has a record).
__device__ __forceinline__ uint64_t bai_reflen_wave(const uint8_t *cig, uint32_t n_cig, bool active, int lane)
{
    const bool big = active && n_cig > BAI_COOP_OPS;
    uint64_t len = active && !big ? bai_reflen_part(cig, 0, n_cig, 1) : 0;
    unsigned long long m = __ballot(big);
    while (m) {
        const int src = __ffsll(m) - 1;
        m &= m - 1;
        const uint8_t *c = (const uint8_t *)__shfl((unsigned long long)cig, src, 64);
        const uint32_t nc = (uint32_t)__shfl((int)n_cig, src, 64);
        const uint64_t part = wave_sum(bai_reflen_part(c, (uint32_t)lane, nc, 64));
        if (lane == src) len = part;
    }
    return len;
}

// virtual offset of whole-file inflated offset x; ne_start / ne_file: exclusive ISIZE sum and file offset of the nn non-empty members
__device__ __forceinline__ uint64_t bai_voff(const uint64_t *ne_start, const uint64_t *ne_file, uint64_t nn, uint64_t total, uint64_t behind, uint64_t x)
{
    if (x >= total || nn == 0) return behind << 16;
    uint64_t lo = 0, hi = nn;                                   // the last member with start <= x
    while (hi - lo > 1) {
        const uint64_t mid = (lo + hi) >> 1;
        if (ne_start[mid] <= x) lo = mid; else hi = mid;
    }
    return ne_file[lo] << 16 | (x - ne_start[lo]);
}
#endif
