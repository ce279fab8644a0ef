// dev_win.h -- the assembly-window collector's text movers: the bodies of k_win_extract and k_win_gather (slx_win.hip).  Host-compilable like dev_edit.h
// (`lane` of `nlanes`, the host build runs lane 0 of 1): tests/cpp/win_host_test.cpp runs them under ASan + UBSan with every block exactly sized.
// The rules are the header comment of include/seqlib_amd_win.h; DESIGN.md 9.14.
//
//   extract  the kept stretch of every selected record of a batch goes into an arena segment: bases at seg, qualities at seg + seg_bytes, a read at
//            aoff[i] (a multiple of 16, wn_padded).  A wave takes WN_TILE bytes of the segment, a lane a 16-byte word at a time: it finds the word's record by
//            binary search in aoff, turns 16 nibbles into ASCII through a 16-entry table (in LDS on the device; the complement table under the strand
//            flip), adds 33 to 16 qualities and stores two aligned words.  Bytes behind a read's end up to its last word are 0.
//   gather   the reads in window order: a wave takes WN_TILE bytes of the OUTPUT, finds its first read by binary search in offs, brings the pieces of the reads
//            that overlap the tile together in LDS -- aligned 16-byte loads from the arena, four reads at a time, 16 lanes each -- and stores the tile with
//            aligned 16-byte stores (only the last partial tile goes byte by byte).
//
// Memory safety.  extract: a word lies below seg_bytes = aoff[n]; the record found holds it, so p0 < wn_padded(klen); source bytes are read at k0 + p with
// p < klen only, inside the sequence and quality arrays wn_select has checked against the span.  gather: the loads are whole words below wn_padded(len) of an
// entry, which the extract wrote; an LDS index is d0 + (byte - s0) with the byte inside the piece, so below the tile's bytes; stores are below `total`.
#pragma once
#include <stdint.h>
#include <string.h>
#include "win_host.h"

#define WN_TILE 2048u           // bytes per wave of k_win_extract and k_win_gather: 64 lanes x 2 x 16 bytes

// an entry: one read of one window.  b, q: the addresses of its bases and qualities in the arena (16-byte aligned, wn_padded(len) bytes each)
struct wn_entry {
    unsigned long long b, q;
    long long ord;              // the record's global ordinal
    uint32_t win, len;
};

#define WN_SEQ_FWD "=ACMGRSVTWYHKDBN"
#define WN_SEQ_REV "=TGKCYSBAWRDMHVN"          // the IUPAC complement of each code (the code's four bits reversed)

// the last k in [0, n) with a[k] <= x (a[0] <= x < a[n], a rises)
template <class T> ED_FN uint64_t wn_find(const T *a, uint64_t n, uint64_t x)
{
    uint64_t lo = 0, hi = n;
    while (hi - lo > 1) {
        const uint64_t mid = (lo + hi) >> 1;
        if ((uint64_t)a[mid] <= x) lo = mid; else hi = mid;
    }
    return lo;
}

// Word w of a segment (bytes [16 w, 16 w + 16) of seg_bytes = aoff[n]).  stream, off: the batch; M: the measure step's records; lut: 32 bytes, WN_SEQ_FWD then
// WN_SEQ_REV.  ob, oq: the segment's bases and qualities, 16-byte aligned.
template <class PL> ED_FN void wn_extract_word(const uint8_t *stream, const uint64_t *off, const unsigned long long *aoff, const wn_rec *M, uint64_t n, uint64_t w, PL lut, uint8_t *ob,
                                               uint8_t *oq)
{
    const uint64_t pos = w << 4;
    const uint64_t k = wn_find(aoff, n, pos);          // (records without text have aoff[k] == aoff[k + 1]: the last k with aoff[k] <= pos is the one that holds it)
    const wn_rec R = M[k];
    const uint8_t *rec = stream + (off[k] - off[0]), *seq = rec + R.seq_at, *qual = seq + ((R.l_seq + 1) >> 1);
    const uint32_t p0 = (uint32_t)(pos - aoff[k]);
    uint32_t vb[4] = {0, 0, 0, 0}, vq[4] = {0, 0, 0, 0};
#if defined(__HIPCC__)
#pragma unroll
#endif
    for (uint32_t j = 0; j < 16; ++j) {
        const uint32_t p = p0 + j;
        if (p < R.klen) {
            const uint32_t s = R.k0 + (R.flip ? R.klen - 1 - p : p);
            const uint32_t nib = (seq[s >> 1] >> ((s & 1) ? 0 : 4)) & 15u;
            vb[j >> 2] |= (uint32_t)lut[nib + (R.flip ? 16u : 0u)] << (8 * (j & 3));
            vq[j >> 2] |= (uint32_t)(uint8_t)(qual[s] + 33u) << (8 * (j & 3));
        }
    }
#if defined(__HIP_DEVICE_COMPILE__)
    ed_v4 b4, q4;
    b4.x = vb[0]; b4.y = vb[1]; b4.z = vb[2]; b4.w = vb[3]; q4.x = vq[0]; q4.y = vq[1]; q4.z = vq[2]; q4.w = vq[3];
    *(ED_GLOBAL ed_v4 *)(ob + pos) = b4;
    *(ED_GLOBAL ed_v4 *)(oq + pos) = q4;
#else
    for (uint32_t j = 0; j < 16; ++j) { ob[pos + j] = (uint8_t)(vb[j >> 2] >> (8 * (j & 3))); oq[pos + j] = (uint8_t)(vq[j >> 2] >> (8 * (j & 3))); }
#endif
}

// Tile `tile` of the output text: bytes [tile * WN_TILE, ...) of the `total`, stored at out + tile * WN_TILE; out is 16-byte aligned.  offs: n_reads + 1 offsets
// of the reads in output order (rising strictly: a read holds a base at least); ent[idx[r]] is read r's entry; quals: take the entries' q, not b.
// lds: WN_TILE bytes, 16-byte aligned, this wave's own.
template <class PB> ED_FN void wn_gather_tile(const unsigned long long *offs, const wn_entry *ent, const uint32_t *idx, uint64_t n_reads, uint64_t total, uint64_t tile, int quals,
                                              PB lds, uint8_t *out, int lane, int nlanes)
{
    const uint64_t t0 = tile * WN_TILE;
    if (t0 >= total || n_reads == 0) return;
    const uint64_t t1 = t0 + WN_TILE < total ? t0 + WN_TILE : total;
    const uint64_t lo = wn_find(offs, n_reads, t0);
    const uint32_t groups = nlanes >= 64 ? 4u : 1u, per = (uint32_t)nlanes / groups, g = (uint32_t)lane / per, sub = (uint32_t)lane % per;
    for (uint64_t r = lo + g; r < n_reads && offs[r] < t1; r += groups) {
        const uint64_t ra = offs[r], rb = offs[r + 1];
        const uint64_t a = ra > t0 ? ra : t0, b = rb < t1 ? rb : t1;
        const wn_entry E = ent[idx[r]];
        const uint8_t *src = (const uint8_t *)(uintptr_t)(quals ? E.q : E.b);
        const uint32_t s0 = (uint32_t)(a - ra), s1 = (uint32_t)(b - ra), d0 = (uint32_t)(a - t0);          // the piece: source bytes [s0, s1) go to lds[d0 ...)
        for (uint32_t wi = (s0 >> 4) + sub; wi <= ((s1 - 1) >> 4); wi += per) {
            const uint32_t wa = wi << 4, x0 = wa > s0 ? wa : s0, x1 = wa + 16 < s1 ? wa + 16 : s1;
#if defined(__HIP_DEVICE_COMPILE__)
            const ed_v4 v = *(const ED_GLOBAL ed_v4 *)(src + wa);
            if (x1 - x0 == 16) __builtin_memcpy(lds + d0 + (wa - s0), &v, 16);          // (the shifted position has no alignment: the compiler picks the stores)
            else for (uint32_t x = x0; x < x1; ++x) { const uint32_t j = x - wa, word = j < 4 ? v.x : j < 8 ? v.y : j < 12 ? v.z : v.w; lds[d0 + (x - s0)] = (uint8_t)(word >> (8 * (j & 3))); }
#else
            for (uint32_t x = x0; x < x1; ++x) lds[d0 + (x - s0)] = src[x];
#endif
        }
    }
    ED_SYNC();
    const uint32_t nb = (uint32_t)(t1 - t0), n16 = nb & ~15u;
    uint8_t *o8 = out + t0;
    for (uint32_t o = (uint32_t)lane << 4; o < n16; o += (uint32_t)nlanes << 4) {
#if defined(__HIP_DEVICE_COMPILE__)
        *(ED_GLOBAL ed_v4 *)(o8 + o) = *(const ED_LDS ed_v4 *)(lds + o);
#else
        memcpy(o8 + o, lds + o, 16);
#endif
    }
    for (uint32_t o = n16 + (uint32_t)lane; o < nb; o += (uint32_t)nlanes) o8[o] = lds[o];          // the ragged tail of the last tile
    ED_SYNC();
}
