// dev_edit.h -- BAM records edited in HBM: the bodies of k_edit_size, k_edit_size_long and k_edit_gather (slx_edit.hip).  Host-compilable like dev_recsort.h
// (`lane` of `nlanes`, the host build runs lane 0 of 1): slx_edit_record and tests/cpp/edit_host_test.cpp run these same bodies on the CPU, the latter under
// ASan + UBSan with every stream and column in a heap block of exactly its size.  The rules are the header comment of include/seqlib_amd_edit.h; DESIGN.md 9.13.
//
// Two steps around a scan:
//   size    per record: its span against the offset table (the test of rs_key, dev_recsort.h), its fixed fields against block_size, then a walk over its aux
//           area that must end exactly at the record's end.  The walk finds the first occurrence of every name that is to be cut -- the dropped names in plan
//           order, then the names of the adds that replace and take effect for this record -- and leaves a descriptor: the cut ranges in rising order, where
//           the head ends, which adds take effect, and the new length.  A lane walks a record; a whole wave walks one whose aux area reaches long_aux bytes
//           and looks for the NUL of a Z / H value 64 bytes per ballot.
//   gather  per TILE of ED_TILE output bytes (the shape of rs_gather_tile): a wave finds the tile's first record, describes the tile's records in LDS and
//           numbers their SLOTS: the kept source ranges between the cuts (cuts + 1 of them, the head is the front of the first), then one per added tag.
//           Slots are taken in rounds of one per lane.  A slot yields at most one PIECE of source bytes -- a kept range, or a Z value out of the constants or
//           the column's text -- cut to the tile; the whole aligned 16-byte words of a round's pieces form one list with a lane per word, the edge bytes a
//           second one.  What is made up rather than copied (a tag's three header bytes, an int value, a NUL, the block_size word, l_seq under clear_seq_qual)
//           is written straight into the tile's image.  The tile leaves with aligned 16-byte stores; only the stream's last partial tile goes byte by byte.
//
// Memory safety.  size: nothing of record i is read before [off[i], off[i + 1]) is known to lie inside the stream and to hold 36 bytes; the fixed fields are
// checked against the span before the aux area is entered, and inside it every header (3 bytes), value, B header (8 bytes) and B payload is compared with the
// record's end BEFORE it is read; the NUL search reads below the record's end only.  A Z column's offsets are read at i and i + 1 (the caller's table holds
// n + 1) and must rise and end inside n_text; an int column is read at i.  gather: a piece is a sub-range of a kept range of a validated record, of the
// constants (offsets fixed when the plan was built) or of a column value whose offsets the size step has checked, and no word or byte outside the piece is
// loaded -- whatever its alignment and however exactly its block is allocated.  Every LDS index is below ED_TILE: a piece and every made-up byte is cut to the
// record's window of the tile, [max(0, -r0), min(len, tile bytes - r0)), before it is placed at r0 + offset.  Every store is below n_bytes of the output.
#pragma once
#include <stdint.h>
#include <string.h>
#include "dev_lanes.h"

#if defined(__HIPCC__)
#define ED_FN __host__ __device__ __forceinline__
#else
#define ED_FN static inline
#endif
#if defined(__HIP_DEVICE_COMPILE__)
#define ED_LDS __attribute__((address_space(3)))
#define ED_GLOBAL __attribute__((address_space(1)))
typedef uint32_t ed_v4 __attribute__((ext_vector_type(4)));
#define ED_SYNC() do { __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront"); __builtin_amdgcn_wave_barrier(); __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront"); } while (0)
#define ED_BALLOT(p) ((uint64_t)__ballot(p))          // (of the whole wave)
#else
#define ED_LDS
#define ED_GLOBAL
#define ED_SYNC() do { } while (0)
#define ED_BALLOT(p) ((p) ? 1ull : 0ull)
#endif

#define ED_TILE 2048u           // output bytes per wave of k_edit_gather: 64 lanes x 2 x 16 bytes
#define ED_MIN_REC 36u          // block_size word + the 32 fixed bytes
#define ED_MAX_REC 64u          // more records than can overlap one tile (2 + 2047 / 36 = 58), and the lanes of a wave
#define ED_MAX_DROP 8u
#define ED_MAX_ADD 8u
#define ED_MAX_CUT (ED_MAX_DROP + ED_MAX_ADD)          // every dropped name and every replacing add can cut one field
#define ED_MAX_CONST 4096u
#define ED_LONG_AUX 256u        // the default of "long_aux"
#define ED_NONE (~0ull)

enum { ED_INT = 0, ED_Z = 1, ED_INT_COL = 2, ED_Z_COL = 3 };
enum { ED_OK = 0, ED_E_RECORD = 1, ED_E_COLUMN = 2, ED_E_SIZE = 3 };

// Every field of the plan is a whole 32-bit word, a tag is its two bytes in the low half of one (ED_TAG).  The plan is a kernel argument, read with scalar loads.
// With tag, kind and replace as bytes the size kernel took a Z constant's length as 0 on gfx950, and the assembly walked the adds with a base of kernarg + 34 (the
// address of add[0].kind) and loaded clen at base + 0xa.  The supposition, not pinned by a reproducer in this tree: the scalar load drops the base's low bits
// before it adds the offset, so the word in front came back.  With whole words no such base can form, whatever the cause.
#define ED_TAG(a, b) ((uint32_t)(uint8_t)(a) | (uint32_t)(uint8_t)(b) << 8)
// one add.  ED_INT: ival.  ED_Z: consts[coff, coff + clen).  ED_INT_COL: vals[i], ival is `absent`.  ED_Z_COL: text[toff[i], toff[i + 1]), inside n_text.
struct ed_add {
    uint32_t tag, kind, replace;
    int32_t ival;
    uint32_t coff, clen;
    const int32_t *vals;
    const uint8_t *text;
    const uint64_t *toff;
    uint64_t n_text;
};
struct ed_plan {
    uint32_t n_drop, n_add, drop_all, clear;
    uint32_t drop[ED_MAX_DROP];
    ed_add add[ED_MAX_ADD];
    const uint8_t *consts;
};
// what the size step leaves of a record: the source bytes kept are [0, aux_end) without the cuts (rising, inside [head, aux_end)); head is where the head ends
// (the aux area's start, the sequence's under clear_seq_qual); aux_end == head when no aux byte stays; bit a of addmask: add a takes effect
struct ed_desc {
    uint32_t head, aux_end, ncut, addmask;
    uint32_t cut_off[ED_MAX_CUT], cut_len[ED_MAX_CUT];
};

ED_FN uint32_t ed_ld32(const uint8_t *p) { return (uint32_t)p[0] | (uint32_t)p[1] << 8 | (uint32_t)p[2] << 16 | (uint32_t)p[3] << 24; }
ED_FN uint32_t ed_popc(uint32_t m) { uint32_t c = 0; for (; m; m &= m - 1) ++c; return c; }
ED_FN uint32_t ed_ctz64(uint64_t m) { uint32_t c = 0; while (!(m & 1)) { m >>= 1; ++c; } return c; }          // m != 0

ED_FN bool ed_span_ok(uint64_t a, uint64_t b, uint64_t n_bytes) { return b > a && b <= n_bytes && b - a >= ED_MIN_REC && b - a <= 0xffffffffull; }

// Record i of the n in stream[0, n_bytes) with offsets off[0 .. n], by the test of rs_key (dev_recsort.h).  The offsets count from off[0], which stands for
// the stream's first byte: the table may be the tail of a larger batch's (a reader's batch that Next() has begun to serve), with the stream pointer moved up
// by as much.  False when record i is the one to name -- one of its offsets lies below off[0]; it does not start where the block_size of record i - 1 ends; its own
// span cannot hold a record; for the last record, its end is not n_bytes or its block_size does not fill its span.  True with *span, and *own = its own block_size fills its span (when not, record i + 1 is the one named and record i is
// left alone).  A block_size word is read only from a span that ed_span_ok has placed inside the stream.
ED_FN bool ed_span(const uint8_t *stream, uint64_t n_bytes, const uint64_t *off, uint64_t i, uint64_t n, uint32_t *span, bool *own)
{
    const uint64_t base = off[0], a = off[i] - base, b = off[i + 1] - base;          // (an offset below off[0] wraps to a span no stream holds)
    if (off[i] < base || off[i + 1] < base) return false;
    if (i > 0) {
        const uint64_t z = off[i - 1] - base;
        if (ed_span_ok(z, a, n_bytes) && (uint64_t)ed_ld32(stream + z) + 4 != a - z) return false;
    }
    if (!ed_span_ok(a, b, n_bytes)) return false;
    *own = (uint64_t)ed_ld32(stream + a) + 4 == b - a;
    if (i + 1 == n && (b != n_bytes || !*own)) return false;
    *span = (uint32_t)(b - a);
    return true;
}

// the fixed fields of a record of `span` >= 36 bytes whose block_size fills it: where the sequence and the aux area start; false when they pass the span
ED_FN bool ed_fixed(const uint8_t *rec, uint32_t span, uint32_t *seq_at, uint32_t *aux_at)
{
    const uint32_t l_name = rec[12], n_cig = (uint32_t)rec[16] | (uint32_t)rec[17] << 8;
    const int32_t l_seq = (int32_t)ed_ld32(rec + 20);
    if (l_seq < 0) return false;
    const uint64_t s = 36ull + l_name + 4ull * n_cig, a = s + (((uint64_t)l_seq + 1) >> 1) + (uint64_t)l_seq;
    if (a > span) return false;
    *seq_at = (uint32_t)s; *aux_at = (uint32_t)a;
    return true;
}

// whether add `a` takes effect for record i, and the bytes of its value behind the three header bytes (a Z value's NUL included); false: the column is broken
ED_FN bool ed_add_of(const ed_add &a, uint64_t i, bool *active, uint32_t *vlen)
{
    *active = true; *vlen = 4;
    if (a.kind == ED_Z) *vlen = a.clen + 1;
    else if (a.kind == ED_INT_COL) *active = a.vals[i] != a.ival;
    else if (a.kind == ED_Z_COL) {
        const uint64_t t0 = a.toff[i], t1 = a.toff[i + 1];
        if (t1 < t0 || t1 > a.n_text || t1 - t0 > 0x7fffffffull) return false;
        *active = t1 > t0; *vlen = (uint32_t)(t1 - t0) + 1;
    }
    return true;
}

// the first NUL in rec[at, end), or end.  WAVE: 64 bytes per ballot, every lane of the wave with the same arguments
template <bool WAVE> ED_FN uint32_t ed_find_nul(const uint8_t *rec, uint32_t at, uint32_t end, int lane, int nlanes)
{
    if (!WAVE) {
        while (at < end && rec[at]) ++at;
        return at;
    }
    for (uint64_t base = at; base < end; base += (uint32_t)nlanes) {
        const uint64_t p = base + (uint32_t)lane;
        const uint64_t m = ED_BALLOT(p < end && rec[p] == 0);
        if (m) return (uint32_t)base + ed_ctz64(m);
    }
    return end;
}

// The aux walk of record i (rec, span bytes, fixed fields checked: seq_at, aux_at): ED_OK with the descriptor and the new length, or the refusal.  WAVE: every
// lane of a wave with the same arguments; all return the same, all write the same descriptor.
template <bool WAVE> ED_FN uint32_t ed_size_record(const ed_plan &P, const uint8_t *rec, uint32_t span, uint32_t seq_at, uint32_t aux_at, uint64_t i, ed_desc *D, uint64_t *newlen,
                                                   int lane, int nlanes)
{
    const bool no_aux = P.drop_all || P.clear;
    uint32_t pending = 0, addmask = 0;          // bit j < 8: dropped name j; bit 8 + a: the name of add a, to be cut before it is appended
    uint64_t added = 0;
    if (!no_aux) pending = (1u << P.n_drop) - 1u;
    for (uint32_t a = 0; a < P.n_add; ++a) {
        bool active; uint32_t vlen;
        if (!ed_add_of(P.add[a], i, &active, &vlen)) return ED_E_COLUMN;
        if (!active) continue;
        addmask |= 1u << a; added += 3ull + vlen;
        const bool z = P.add[a].kind == ED_Z || P.add[a].kind == ED_Z_COL;
        if (!no_aux && (z || P.add[a].replace)) pending |= 1u << (8 + a);
    }
    uint32_t ncut = 0, at = aux_at;
    uint64_t cut_bytes = 0;
    while (at < span) {
        if (span - at < 3) return ED_E_RECORD;
        const uint8_t t = rec[at + 2];
        uint64_t e;
        if (t == 'A' || t == 'c' || t == 'C') e = (uint64_t)at + 4;
        else if (t == 's' || t == 'S') e = (uint64_t)at + 5;
        else if (t == 'i' || t == 'I' || t == 'f') e = (uint64_t)at + 7;
        else if (t == 'd') e = (uint64_t)at + 11;
        else if (t == 'Z' || t == 'H') {
            const uint32_t z = ed_find_nul<WAVE>(rec, at + 3, span, lane, nlanes);
            if (z >= span) return ED_E_RECORD;
            e = (uint64_t)z + 1;
        } else if (t == 'B') {
            if (span - at < 8) return ED_E_RECORD;
            const uint8_t et = rec[at + 3];
            const uint32_t es = (et == 'c' || et == 'C') ? 1u : (et == 's' || et == 'S') ? 2u : (et == 'i' || et == 'I' || et == 'f') ? 4u : 0u;
            if (!es) return ED_E_RECORD;
            e = (uint64_t)at + 8 + (uint64_t)es * ed_ld32(rec + at + 4);
        } else return ED_E_RECORD;
        if (e > span) return ED_E_RECORD;
        for (uint32_t m = pending; m; m &= m - 1) {          // the first request in plan order that still waits for this name
            const uint32_t j = (uint32_t)ed_ctz64(m);
            if ((j < 8 ? P.drop[j] : P.add[j - 8].tag) == ED_TAG(rec[at], rec[at + 1])) {
                if (!WAVE || lane == 0) { D->cut_off[ncut] = at; D->cut_len[ncut] = (uint32_t)e - at; }
                ++ncut; cut_bytes += e - at; pending &= ~(1u << j);
                break;
            }
        }
        at = (uint32_t)e;
    }
    const uint32_t head = P.clear ? seq_at : aux_at, aux_end = no_aux ? head : span;
    const uint64_t len = (uint64_t)aux_end - cut_bytes + added;
    if (len - 4 > 0xffffffffull) return ED_E_SIZE;
    if (!WAVE || lane == 0) { D->head = head; D->aux_end = aux_end; D->ncut = ncut; D->addmask = addmask; }
    *newlen = len;
    return ED_OK;
}

// ---------------------------------------------------------------- the gather
#define ED_ROUND 64u          // slots per round: the lanes of a wave (the host build takes one)
// per wave, in LDS beside the tile's image
struct ed_tile {
    unsigned long long src[ED_MAX_REC];          // address of the record's first source byte
    unsigned long long sp[ED_ROUND];             // the pieces of a round: address of the first byte
    long long r0[ED_MAX_REC];                    // where the record starts, counted from the tile's start (negative: before it)
    uint32_t len[ED_MAX_REC];                    // its new length
    uint16_t ps[ED_MAX_REC + 1];                 // running sum of the records' slots
    uint16_t d[ED_ROUND], n[ED_ROUND], head[ED_ROUND];          // a piece: where it goes in the tile, its length, its bytes before the first aligned 16-byte word
    uint16_t pw[ED_ROUND + 1], pe[ED_ROUND + 1];                // running sums over the pieces: whole words, edge bytes
};

// item i of a running sum p[0 .. cnt]: the last k with p[k] <= i (i < p[cnt]: an entry that holds something)
template <class PU16> ED_FN uint32_t ed_find(PU16 p, uint32_t cnt, uint32_t i)
{
    uint32_t k0 = 0, k1 = cnt;
    while (k1 - k0 > 1) {
        const uint32_t mid = (k0 + k1) >> 1;
        if (p[mid] <= i) k0 = mid; else k1 = mid;
    }
    return k0;
}

// v summed over the lanes in front of this one, and over all of them
ED_FN uint32_t ed_excl_scan(uint32_t v, int lane, uint32_t *total)
{
#if defined(__HIP_DEVICE_COMPILE__)
    (void)lane;
    return wave_scan_excl(v, total);
#else
    (void)lane;
    *total = v;
    return 0;
#endif
}

// byte b of the record at offset o, when o lies in the record's window [wa, wb) of the tile
template <class PB> ED_FN void ed_put(PB lds, long long r0, long long wa, long long wb, long long o, uint8_t b) { if (o >= wa && o < wb) lds[r0 + o] = b; }

// Tile `tile` of the edited stream: bytes [tile * ED_TILE, ...) of the n_bytes, stored at out + tile * ED_TILE; out is 16-byte aligned.  stream, off: the
// source batch; new_off: n + 1 offsets of the edited records; desc: the size step's descriptors.  lds: ED_TILE bytes, 16-byte aligned, and T: this wave's own.
// PB, PT: pointers to bytes and to ed_tile; the kernel passes them with LDS in their type (ED_LDS), so that the image and the tables are addressed as LDS (dev_as.h).
template <class PB, class PT>
ED_FN void ed_gather_tile(const ed_plan &P, const uint8_t *stream, const uint64_t *off, const unsigned long long *new_off, const ed_desc *desc, int64_t n, uint64_t n_bytes, uint64_t tile,
                          PB lds, PT T, uint8_t *out, int lane, int nlanes)
{
    const uint64_t t0 = tile * ED_TILE;
    if (t0 >= n_bytes || n <= 0) return;
    const uint64_t t1 = t0 + ED_TILE < n_bytes ? t0 + ED_TILE : n_bytes;
    int64_t lo = 0, hi = n;          // new_off[lo] <= t0 < new_off[hi]: new_off rises strictly (a record keeps its 36 bytes at least) and new_off[0] = 0
    while (hi - lo > 1) {
        const int64_t step = (hi - lo + nlanes) / (nlanes + 1);
        const int64_t probe = lo + (int64_t)(lane + 1) * step;
        const bool le = probe < hi && new_off[probe] <= t0;
        const uint64_t seen = ED_BALLOT(le);                             // the probes rise with the lane: the lanes that see <= t0 are the first c
        const int64_t c = (int64_t)ed_popc((uint32_t)seen) + (int64_t)ed_popc((uint32_t)(seen >> 32));
        lo += c * step;
        if (c < nlanes && lo + step < hi) hi = lo + step;
    }
    uint32_t cnt = 0, S = 0;         // records that overlap the tile (at most 2 + 2047 / 36 < ED_MAX_REC), their slots
    for (uint32_t l = (uint32_t)lane; l < ED_MAX_REC; l += (uint32_t)nlanes) {
        const int64_t k = lo + (int64_t)l;
        const bool v = k < n && new_off[k] < t1;
        uint32_t slots = 0;
        if (v) {
            T->src[l] = (unsigned long long)(uintptr_t)(stream + (off[k] - off[0]));
            T->r0[l] = (long long)new_off[k] - (long long)t0;
            T->len[l] = (uint32_t)(new_off[k + 1] - new_off[k]);
            slots = desc[k].ncut + 1 + ed_popc(desc[k].addmask);
        }
        uint32_t tot;
        const uint32_t ex = ed_excl_scan(slots, lane, &tot);
        if (v) T->ps[l] = (uint16_t)(S + ex);
        S += tot;
        const uint64_t m = ED_BALLOT(v);
        cnt += ed_popc((uint32_t)m) + ed_popc((uint32_t)(m >> 32));
    }
    if (lane == 0) T->ps[cnt] = (uint16_t)S;
    ED_SYNC();
    const long long tb = (long long)(t1 - t0);
    for (uint32_t base = 0; base < S; base += (uint32_t)nlanes) {
        const uint32_t s = base + (uint32_t)lane;
        unsigned long long sp = 0;
        uint32_t pn = 0, pd = 0;
        if (s < S) {
            const uint32_t k = ed_find(T->ps, cnt, s), j = s - T->ps[k];
            const uint64_t r = (uint64_t)lo + k;
            const ed_desc *D = desc + r;
            const long long r0 = T->r0[k], wa = r0 < 0 ? -r0 : 0, wb = (long long)T->len[k] < tb - r0 ? (long long)T->len[k] : tb - r0;
            const uint32_t ncut = D->ncut;
            long long dst = 0, plen = 0;          // the piece in the edited record, before it is cut to the window
            const uint8_t *ps = nullptr;
            if (j <= ncut) {          // the kept range in front of cut j (behind the last cut: up to aux_end)
                uint32_t gone = 0;
                for (uint32_t c = 0; c < j; ++c) gone += D->cut_len[c];
                const uint32_t sb = j ? D->cut_off[j - 1] + D->cut_len[j - 1] : 0u, se = j < ncut ? D->cut_off[j] : D->aux_end;
                ps = (const uint8_t *)(uintptr_t)T->src[k] + sb; dst = (long long)sb - gone; plen = (long long)se - sb;
            } else {                  // the (j - ncut)th add that takes effect
                uint32_t gone = 0, a = 0, left = j - ncut - 1;
                for (uint32_t c = 0; c < ncut; ++c) gone += D->cut_len[c];
                dst = (long long)D->aux_end - gone;
                const uint32_t mask = D->addmask;
                for (;; ++a) {
                    if (!(mask >> a & 1u)) continue;
                    if (!left) break;
                    bool act; uint32_t vl;
                    (void)ed_add_of(P.add[a], r, &act, &vl);
                    dst += 3 + (long long)vl; --left;
                }
                const ed_add &A = P.add[a];
                const bool z = A.kind == ED_Z || A.kind == ED_Z_COL;
                ed_put(lds, r0, wa, wb, dst, (uint8_t)A.tag); ed_put(lds, r0, wa, wb, dst + 1, (uint8_t)(A.tag >> 8)); ed_put(lds, r0, wa, wb, dst + 2, z ? (uint8_t)'Z' : (uint8_t)'i');
                dst += 3;
                if (!z) {
                    const uint32_t v = (uint32_t)(A.kind == ED_INT ? A.ival : A.vals[r]);
                    for (int b = 0; b < 4; ++b) ed_put(lds, r0, wa, wb, dst + b, (uint8_t)(v >> (8 * b)));
                } else {
                    if (A.kind == ED_Z) { ps = P.consts + A.coff; plen = A.clen; }
                    else { ps = A.text + A.toff[r]; plen = (long long)(A.toff[r + 1] - A.toff[r]); }
                    ed_put(lds, r0, wa, wb, dst + plen, 0);
                }
            }
            const long long a0 = dst > wa ? dst : wa, b0 = dst + plen < wb ? dst + plen : wb;
            if (b0 > a0) { sp = (unsigned long long)(uintptr_t)(ps + (a0 - dst)); pn = (uint32_t)(b0 - a0); pd = (uint32_t)(r0 + a0); }
        }
        uint32_t ph = (16u - (uint32_t)(sp & 15u)) & 15u;
        if (ph > pn) ph = pn;
        const uint32_t nw = (pn - ph) >> 4, ne = pn - (nw << 4);
        uint32_t W, E;
        const uint32_t xw = ed_excl_scan(nw, lane, &W), xe = ed_excl_scan(ne, lane, &E);
        T->sp[lane] = sp; T->d[lane] = (uint16_t)pd; T->n[lane] = (uint16_t)pn; T->head[lane] = (uint16_t)ph; T->pw[lane] = (uint16_t)xw; T->pe[lane] = (uint16_t)xe;
        if (lane == 0) { T->pw[nlanes] = (uint16_t)W; T->pe[nlanes] = (uint16_t)E; }
        ED_SYNC();
#if defined(__HIPCC__)
#pragma unroll 2
#endif
        for (uint32_t i = (uint32_t)lane; i < W; i += (uint32_t)nlanes) {
            const uint32_t k = ed_find(T->pw, (uint32_t)nlanes, i), o = (uint32_t)T->head[k] + ((i - T->pw[k]) << 4);
            const uint8_t *sw = (const uint8_t *)(uintptr_t)T->sp[k];
            const PB dw = lds + T->d[k] + o;
#if defined(__HIP_DEVICE_COMPILE__)
            const ed_v4 v = *(const ED_GLOBAL ed_v4 *)(sw + o);          // (sources are blocks of HBM: a global load, not a flat one)
            __builtin_memcpy(dw, &v, 16);          // (the shifted position has no alignment: the compiler picks the stores)
#else
            memcpy(dw, sw + o, 16);
#endif
        }
        for (uint32_t i = (uint32_t)lane; i < E; i += (uint32_t)nlanes) {
            const uint32_t k = ed_find(T->pe, (uint32_t)nlanes, i), q = i - T->pe[k], h = T->head[k];
            const uint32_t o = q < h ? q : h + ((((uint32_t)T->n[k] - h) >> 4) << 4) + (q - h);
            const uint8_t *se = (const uint8_t *)(uintptr_t)T->sp[k];
#if defined(__HIP_DEVICE_COMPILE__)
            lds[T->d[k] + o] = *(const ED_GLOBAL uint8_t *)(se + o);
#else
            lds[T->d[k] + o] = se[o];
#endif
        }
        ED_SYNC();
    }
    // behind the copies: block_size of every record of the tile, and l_seq = 0 where the sequence went
    for (uint32_t l = (uint32_t)lane; l < cnt; l += (uint32_t)nlanes) {
        const long long r0 = T->r0[l], wa = r0 < 0 ? -r0 : 0, wb = (long long)T->len[l] < tb - r0 ? (long long)T->len[l] : tb - r0;
        const uint32_t bs = T->len[l] - 4;
        for (int b = 0; b < 4; ++b) {
            ed_put(lds, r0, wa, wb, b, (uint8_t)(bs >> (8 * b)));
            if (P.clear) ed_put(lds, r0, wa, wb, 20 + b, 0);
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
    for (uint32_t o = n16 + (uint32_t)lane; o < nb; o += (uint32_t)nlanes) o8[o] = lds[o];          // the ragged tail of the stream's last tile
    ED_SYNC();
}
