// dev_recsort.h -- coordinate sort of BAM records in HBM: the bodies of k_sort_key and k_sort_gather (slx_sort.hip).  (dev_sort.h is something else: the
// introsort emulations of the aligner.)  Host-compilable like dev_rec.h and dev_deflate.h (`lane` of `nlanes`, the host build runs lane 0 of 1) so that
// tests/cpp/sort_host_test.cpp can hold both against a plain memcpy model under ASan + UBSan before they run on a GPU.
//
// Two steps:
//   key     per record: its block_size against the offset table, then the 64-bit key (uint32)tid << 32 | (uint32)pos ^ 0x80000000 -- tid ascending as
//           unsigned (-1, the unplaced tail, last), pos ascending as signed -- its length and its source address.  Nothing of a record is read before
//           its offsets are known to lie inside the segment.
//   gather  per TILE of RS_TILE output bytes, not per record (the shape of rec_fill_tile, dev_rec.h): a wave finds the first sorted record that overlaps
//           its tile (a search in dst_off that probes 64 places per step), describes the records of the tile in LDS, a lane each, brings their
//           shares into the tile's image in LDS, then stores the tile with aligned 16-byte vector stores; only the tail of the stream's last tile goes out byte by byte.  A record that crosses tiles is written by the waves of
//           both, each its own bytes; slabs are ranges of tiles, so a record may cross a slab join too.
//           The reads: sources are scattered and unaligned.  A share [sa, sb) of a record is read as the aligned 16-byte words that lie wholly inside
//           it and every word is placed in LDS at its shifted position; the up to 15 bytes before the first such word and after the last go byte by byte.
//           The words of all the tile's shares form one list with a lane per word, the edge bytes another: the wave waits for memory a handful of
//           times per tile, not several times per record.
// Memory safety: a share is a sub-range of one record, the key step has checked that every record lies inside its segment, and no word or byte outside
// the share is loaded -- so nothing outside a segment is touched, whatever its alignment and however exactly it is allocated.  Every LDS index is below
// RS_TILE (a share is cut to the tile), every store is below the slab's end (n_bytes, cut to the tile range).
#pragma once
#include <stdint.h>
#include <string.h>

#if defined(__HIPCC__)
#define RS_FN __device__ __forceinline__
#define RS_GLOBAL __attribute__((address_space(1)))
typedef uint32_t rs_v4 __attribute__((ext_vector_type(4)));
#define RS_SYNC() do { __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront"); __builtin_amdgcn_wave_barrier(); __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront"); } while (0)
#define RS_COUNT(p) ((uint32_t)__popcll(__ballot(p)))          // how many lanes of the (whole) wave see p
#else
#define RS_FN static inline
#define RS_SYNC() do { } while (0)
#define RS_COUNT(p) ((p) ? 1u : 0u)
#endif

#define RS_TILE 2048u           // output bytes per wave of k_sort_gather: 64 lanes x 2 x 16 bytes
#define RS_MIN_REC 36u          // block_size word + the 32 fixed bytes
#define RS_NO_BAD (~0ull)
#define RS_MAX_REC 64u          // more records than can overlap one tile (2 + 2047 / 36 = 58), and the lanes of a wave

RS_FN uint32_t rs_ld32(const uint8_t *p) { return (uint32_t)p[0] | (uint32_t)p[1] << 8 | (uint32_t)p[2] << 16 | (uint32_t)p[3] << 24; }

// a span of the offset table that can hold a record: rising, inside the stream, at least the 36 fixed bytes, a length of 32 bits
RS_FN bool rs_span_ok(uint64_t a, uint64_t b, uint64_t n_bytes) { return b > a && b <= n_bytes && b - a >= RS_MIN_REC && b - a <= 0xffffffffull; }

// Record i of the n in stream[0, n_bytes) with offsets off[0 .. n]: true and (key, length) when the table and the block_size words agree as far as lane i
// can tell, false when record i is the one to name:
//   off[0] is not 0;  record i does not start where the block_size of record i - 1 ends (an entry of the table is blamed on the record that starts there);
//   its own span cannot hold a record;  for the last record, off[n] is not n_bytes or its block_size does not fill its span.
// All n lanes true = every record lies inside the stream with block_size + 4 = its span (so block_size >= 32).  A block_size word is read only from a span
// that rs_span_ok has placed inside the stream.
RS_FN bool rs_key(const uint8_t *stream, uint64_t n_bytes, const uint64_t *off, uint64_t i, uint64_t n, uint64_t *key, uint32_t *len)
{
    const uint64_t a = off[i], b = off[i + 1];
    if (i == 0 && a != 0) return false;
    if (i > 0) {
        const uint64_t z = off[i - 1];
        if (rs_span_ok(z, a, n_bytes) && (uint64_t)rs_ld32(stream + z) + 4 != a - z) return false;
    }
    if (!rs_span_ok(a, b, n_bytes)) return false;
    const uint8_t *p = stream + a;
    if (i + 1 == n && (b != n_bytes || (uint64_t)rs_ld32(p) + 4 != b - a)) return false;
    *key = (uint64_t)rs_ld32(p + 4) << 32 | (uint64_t)(rs_ld32(p + 8) ^ 0x80000000u);
    *len = (uint32_t)(b - a);
    return true;
}

// what a tile needs of the records that overlap it, per wave, in LDS beside the tile's image
struct rs_desc {
    unsigned long long sp[RS_MAX_REC];                              // address of the first byte of the record's share of the tile
    uint16_t d[RS_MAX_REC], n[RS_MAX_REC], head[RS_MAX_REC];        // where the share goes in the tile, its length, its bytes before the first aligned 16-byte word
    uint16_t pw[RS_MAX_REC + 1], pe[RS_MAX_REC + 1];                // running sums over the records: whole words, edge bytes
};

// item i of a running sum p[0 .. cnt]: the record k with p[k] <= i < p[k + 1]
RS_FN uint32_t rs_find(const uint16_t *p, uint32_t cnt, uint32_t i)
{
    uint32_t k0 = 0, k1 = cnt;
    while (k1 - k0 > 1) {
        const uint32_t mid = (k0 + k1) >> 1;
        if (p[mid] <= i) k0 = mid; else k1 = mid;
    }
    return k0;
}

// Tile `tile` of the sorted stream: bytes [tile * RS_TILE, ...) of the n_bytes, stored at out + (tile * RS_TILE - out_base) -- out is the slab, out_base the
// stream offset of its first byte (a multiple of RS_TILE), out is 16-byte aligned.  dst_off: n + 1 offsets of the sorted records in the stream, src: the address of
// each sorted record's first byte.  lds: RS_TILE bytes, 16-byte aligned, and D: both this wave's own.
// The steps, each one round trip to memory for the whole wave, not one per record:
//   search   the last record that starts at or before the tile, by a search in dst_off that probes nlanes places per step (a binary search on the host build)
//   describe lane l takes record lo + l: its share [a, b) of the tile, the share's source address, the bytes before its first aligned word
//   words    the whole aligned 16-byte words of all shares as ONE list, a lane per word: a global_load_dwordx4 each, placed in LDS at the shifted position
//   edges    the up to 15 bytes before a share's first word and after its last, as one list too, a lane per byte
// Nothing outside a share is loaded.
RS_FN void rs_gather_tile(const unsigned long long *dst_off, const unsigned long long *src, int64_t n, uint64_t n_bytes, uint64_t tile, uint8_t *lds, rs_desc *D,
                          uint8_t *out, uint64_t out_base, int lane, int nlanes)
{
    const uint64_t t0 = tile * RS_TILE;
    if (t0 >= n_bytes || n <= 0) return;
    const uint64_t t1 = t0 + RS_TILE < n_bytes ? t0 + RS_TILE : n_bytes;
    int64_t lo = 0, hi = n;          // dst_off[lo] <= t0 < dst_off[hi]: dst_off rises strictly (a record has 36 bytes at least) and dst_off[0] = 0
    while (hi - lo > 1) {
        const int64_t step = (hi - lo + nlanes) / (nlanes + 1);          // the probes lo + step, lo + 2 step, ...: those below hi count
        const int64_t probe = lo + (int64_t)(lane + 1) * step;
        const bool le = probe < hi && dst_off[probe] <= t0;
        const int64_t c = (int64_t)RS_COUNT(le);                         // the probes rise with the lane: the lanes that see <= t0 are the first c
        lo += c * step;
        if (c < nlanes && lo + step < hi) hi = lo + step;                // (the probe behind them was made, and saw > t0)
    }
    uint32_t cnt = 0;                // records that overlap the tile: at most 2 + 2047 / 36 < RS_MAX_REC
    for (uint32_t l = (uint32_t)lane; l < RS_MAX_REC; l += (uint32_t)nlanes) {
        const int64_t k = lo + (int64_t)l;
        const bool v = k < n && dst_off[k] < t1;
        if (v) {
            const uint64_t r0 = dst_off[k], r1 = dst_off[k + 1];
            const uint64_t a = r0 > t0 ? r0 : t0, b = r1 < t1 ? r1 : t1;
            const uint64_t sp = src[k] + (a - r0);
            const uint32_t nn = (uint32_t)(b - a);
            uint32_t h = (16u - (uint32_t)(sp & 15u)) & 15u;
            if (h > nn) h = nn;
            D->sp[l] = sp; D->d[l] = (uint16_t)(a - t0); D->n[l] = (uint16_t)nn; D->head[l] = (uint16_t)h;
        }
        cnt += RS_COUNT(v);
    }
    RS_SYNC();
    for (uint32_t l = (uint32_t)lane; l <= cnt; l += (uint32_t)nlanes) {
        uint32_t w = 0, e = 0;
        for (uint32_t j = 0; j < l; ++j) { const uint32_t nw = ((uint32_t)D->n[j] - D->head[j]) >> 4; w += nw; e += (uint32_t)D->n[j] - (nw << 4); }
        D->pw[l] = (uint16_t)w; D->pe[l] = (uint16_t)e;
    }
    RS_SYNC();
    const uint32_t W = D->pw[cnt], E = D->pe[cnt];
#pragma unroll 2
    for (uint32_t i = (uint32_t)lane; i < W; i += (uint32_t)nlanes) {
        const uint32_t k = rs_find(D->pw, cnt, i), o = (uint32_t)D->head[k] + ((i - D->pw[k]) << 4);
        const uint8_t *s = (const uint8_t *)(uintptr_t)D->sp[k];
        uint8_t *d = lds + D->d[k];
#if defined(__HIPCC__)
        const rs_v4 v = *(const RS_GLOBAL rs_v4 *)(s + o);          // (sources are segments of HBM: a global load, not a flat one)
        __builtin_memcpy(d + o, &v, 16);
#else
        memcpy(d + o, s + o, 16);
#endif
    }
    for (uint32_t i = (uint32_t)lane; i < E; i += (uint32_t)nlanes) {
        const uint32_t k = rs_find(D->pe, cnt, i), j = i - D->pe[k], h = D->head[k];
        const uint32_t o = j < h ? j : h + ((((uint32_t)D->n[k] - h) >> 4) << 4) + (j - h);
        const uint8_t *s = (const uint8_t *)(uintptr_t)D->sp[k];
#if defined(__HIPCC__)
        lds[D->d[k] + o] = *(const RS_GLOBAL uint8_t *)(s + o);
#else
        lds[D->d[k] + o] = s[o];
#endif
    }
    RS_SYNC();
    const uint32_t nb = (uint32_t)(t1 - t0), n16 = nb & ~15u;
    uint8_t *o8 = out + (t0 - out_base);
    for (uint32_t o = (uint32_t)lane << 4; o < n16; o += (uint32_t)nlanes << 4) {
#if defined(__HIPCC__)
        *reinterpret_cast<uint4 *>(o8 + o) = *reinterpret_cast<const uint4 *>(lds + o);
#else
        memcpy(o8 + o, lds + o, 16);
#endif
    }
    for (uint32_t o = n16 + (uint32_t)lane; o < nb; o += (uint32_t)nlanes) o8[o] = lds[o];          // the ragged tail of the stream's last tile
    RS_SYNC();
}
