// dev_rec.h -- BAM records from a device-resident slx_hits: the bodies of k_rec_owner, k_rec_size, k_rec_size_wide and k_rec_fill (slx_rec.hip).
// Host-compilable like dev_deflate.h (`lane` of `nlanes`, the host build runs lane 0 of 1) so that tests/cpp/rec_host_test.cpp can hold the bytes against
// the record layout under ASan + UBSan before they are built on a GPU.  The specification is BWAAligner::make_record followed by BamWriter::put_record
// (include/SeqLib): block_size, the eight fixed words, name + NUL, the CIGAR words as they stand, the 4-bit sequence of the hard-clip window, 0xff + zeros
// for the qualities, NA:i NM:i AS:i.
//
// Two steps:
//   size   per hit: the hard-clip window (tstart, clen), the reference span -> end -> reg2bin(pos, end), the record's byte length, a refusal code.
//          rec_cigar_part sums a strided share of the CIGAR (lane of nlanes); one lane walks a short CIGAR whole, a wave shares a contig's.
//   fill   per TILE of REC_TILE output bytes, not per record: a wave finds the records that overlap its tile (binary search in rec_off), writes their
//          bytes of the tile into LDS -- lanes stride over the bytes, so names, CIGAR words and bases are read side by side -- and stores the tile with
//          aligned 16-byte vector stores; only the tail of the stream's last tile goes out byte by byte.  A record that crosses tiles is written by the
//          waves of both, each its own bytes: a contig's 500 KB record is spread over 250 waves by the same code, there is no long form.
// Memory safety: every read of hits, names and bases is inside the arrays the size step has checked the window against; every store is below n_bytes.
#pragma once
#include <stdint.h>
#include <string.h>

#if defined(__HIPCC__)
#include "dev_wave.h"
#define REC_FN __device__ __forceinline__
#define REC_UNIFORM(x) ((int64_t)rfl_u64((uint64_t)(x)))          // a value every lane of the wave holds alike, moved to scalar registers: what is indexed by it is loaded once per wave
#define REC_SYNC() do { __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront"); __builtin_amdgcn_wave_barrier(); __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront"); } while (0)
#else
#define REC_FN static inline
#define REC_UNIFORM(x) (x)
#define REC_SYNC() do { } while (0)
#endif

enum {
    REC_OK = 0,
    REC_E_NAME = 1,         // a name longer than 254 bytes: l_read_name is one byte
    REC_E_NCIGAR = 2,       // more than 65 535 CIGAR operations: n_cigar_op is 16 bits
    REC_E_WINDOW = 3,       // hardclip: an empty window or one that passes the read (the host path asserts)
    REC_E_HOST = 4,         // the result is host-resident
    REC_E_REG2SAM = 5       // a SLX_F_REG2SAM result: XA / SA / MD are host-built strings
};

// what is known of a result before any kernel runs, and the C-ABI's code for each refusal (seqlib_amd.h: SLX_EINVAL -1, SLX_EUNSUPPORTED -5)
static inline int rec_check_result(int on_device, const void *xa_parent) { return !on_device ? REC_E_HOST : xa_parent ? REC_E_REG2SAM : REC_OK; }
static inline int rec_slx_code(int code) { return code == REC_OK ? 0 : (code == REC_E_WINDOW || code == REC_E_HOST) ? -1 : -5; }

#define REC_TILE 2048u          // output bytes per wave of k_rec_fill: 64 lanes x 2 x 16 bytes
#define REC_WIDE_OPS 256        // a hit with more CIGAR operations than this is sized by a wave
#define REC_MAX_NAME 254
#define REC_MAX_NCIGAR 65535
#define REC_NO_REFUSAL (~0ull)

struct rec_in {
    // the result (slx_hits, seqlib_amd.h)
    int64_t n_reads, n_hits;
    const int64_t *hit_off;
    const int32_t *rid;
    const int64_t *pos;
    const uint16_t *flag;
    const uint8_t *mapq;
    const int32_t *score, *nm, *na, *n_cigar_ops;
    const int64_t *cig_off;
    const uint32_t *cigar;
    // the reads as the aligner was given them
    const uint8_t *bases;
    const uint64_t *offs;
    // the names: laid out like the reads (names, name_offs), or -- bam_stream != nullptr -- the read_name of record rec_of_read[i] of a BAM batch
    const uint8_t *names;
    const uint64_t *name_offs;
    const uint8_t *bam_stream;
    const uint64_t *bam_rec_off;
    const int64_t *rec_of_read;
    int hardclip;
};

struct rec_meta { uint32_t tstart, clen, bin, pad; };      // per hit, from the size step to the fill step

struct rec_part { uint64_t tstart, qlen, rlen; uint32_t any_ref; };

REC_FN uint32_t rec_cigar_type(uint32_t op) { return 0x3C1A7u >> (op << 1) & 3u; }      // bit 0: consumes the query, bit 1: the reference (htslib's BAM_CIGAR_TYPE)

REC_FN uint32_t rec_ld32(const uint8_t *p) { return (uint32_t)p[0] | (uint32_t)p[1] << 8 | (uint32_t)p[2] << 16 | (uint32_t)p[3] << 24; }

// the name of read i: where it starts and its length (no terminator)
REC_FN const uint8_t *rec_name(const rec_in &in, int64_t i, uint32_t &l_name)
{
    if (in.bam_stream) {
        const uint8_t *p = in.bam_stream + in.bam_rec_off[in.rec_of_read[i]];
        l_name = p[12] ? (uint32_t)p[12] - 1 : 0;          // l_read_name counts the NUL
        return p + 36;
    }
    l_name = (uint32_t)(in.name_offs[i + 1] - in.name_offs[i]);
    return in.names + in.name_offs[i];
}

// lane's share of hit k's CIGAR: operations lane, lane + nlanes, ...  The shares add up (rec_part_add) to what make_record and bam_endpos walk.
REC_FN rec_part rec_cigar_part(const rec_in &in, int64_t k, int lane, int nlanes)
{
    rec_part p = {0, 0, 0, 0};
    const uint32_t *cig = in.cigar + in.cig_off[k];
    const int n = in.n_cigar_ops[k];
    for (int c = lane; c < n; c += nlanes) {
        const uint32_t op = cig[c] & 15u, len = cig[c] >> 4, t = rec_cigar_type(op);
        if (c == 0 && op == 5) p.tstart = len;
        else if (op != 5 && (t & 1)) p.qlen += len;
        if (t & 2) { p.rlen += len; p.any_ref = 1; }
    }
    return p;
}
REC_FN void rec_part_add(rec_part &a, const rec_part &b) { a.tstart += b.tstart; a.qlen += b.qlen; a.rlen += b.rlen; a.any_ref |= b.any_ref; }

REC_FN uint32_t rec_reg2bin(int64_t beg, int64_t end)          // SAMv1 5.3, as BamWriter::reg2bin states it
{
    --end;
    if (beg >> 14 == end >> 14) return (uint32_t)(((1 << 15) - 1) / 7 + (beg >> 14));
    if (beg >> 17 == end >> 17) return (uint32_t)(((1 << 12) - 1) / 7 + (beg >> 17));
    if (beg >> 20 == end >> 20) return (uint32_t)(((1 << 9) - 1) / 7 + (beg >> 20));
    if (beg >> 23 == end >> 23) return (uint32_t)(((1 << 6) - 1) / 7 + (beg >> 23));
    if (beg >> 26 == end >> 26) return (uint32_t)(((1 << 3) - 1) / 7 + (beg >> 26));
    return 0;
}

// hit k of read i from the whole CIGAR's sums: its meta, its length in the stream (block_size word included) and its refusal code
REC_FN uint32_t rec_size_finish(const rec_in &in, int64_t k, int64_t i, const rec_part &p, rec_meta *meta, unsigned long long *len)
{
    const uint64_t read_len = in.offs[i + 1] - in.offs[i];
    uint64_t tstart = 0, clen = read_len;
    uint32_t code = REC_OK;
    if (in.hardclip) {
        tstart = p.tstart; clen = p.qlen;
        if (clen == 0 || tstart + clen > read_len) code = REC_E_WINDOW;
    }
    const int64_t n_cig = in.n_cigar_ops[k];
    if (n_cig > REC_MAX_NCIGAR || n_cig < 0) code = REC_E_NCIGAR;
    uint32_t l_name;
    (void)rec_name(in, i, l_name);
    if (l_name > REC_MAX_NAME) code = REC_E_NAME;
    if (code != REC_OK) { tstart = 0; clen = 0; }          // (a refused batch is never filled; the figures stay inside the read all the same)
    const int64_t pos = in.pos[k], end = p.any_ref ? pos + (int64_t)p.rlen : pos + 1;          // bam_endpos
    meta[k].tstart = (uint32_t)tstart; meta[k].clen = (uint32_t)clen; meta[k].bin = rec_reg2bin(pos, end) & 0xffffu; meta[k].pad = 0;
    len[k] = 4ull + 32 + l_name + 1 + 4ull * (uint64_t)(n_cig < 0 ? 0 : n_cig) + ((clen + 1) >> 1) + clen + 21;
    return code;
}

// ---- fill
struct rec_hit {                // what a tile needs of one record: wave-uniform
    uint32_t w0, w1, w2, w3, w4, w5;      // block_size and the first five fixed words (mtid = mpos = -1 and isize = 0 are constants)
    const uint8_t *name, *cig, *seq;      // seq: first base of the clip window
    uint32_t l_name, cig_bytes, sl, seq_bytes;
    uint32_t rev;
    uint32_t na, nm, as;
};

REC_FN void rec_hit_load(const rec_in &in, const rec_meta *meta, const int64_t *owner, const unsigned long long *rec_off, int64_t k, rec_hit &h)
{
    const int64_t i = owner[k];
    h.name = rec_name(in, i, h.l_name);
    const uint32_t n_cig = (uint32_t)in.n_cigar_ops[k];
    h.cig = (const uint8_t *)(in.cigar + in.cig_off[k]);
    h.cig_bytes = n_cig << 2;
    h.sl = meta[k].clen;
    h.seq_bytes = (h.sl + 1) >> 1;
    h.seq = in.bases + in.offs[i] + meta[k].tstart;
    const uint32_t flag = in.flag[k];
    h.rev = flag & 16u;
    h.na = (uint32_t)in.na[k]; h.nm = (uint32_t)in.nm[k]; h.as = (uint32_t)in.score[k];
    h.w0 = (uint32_t)(rec_off[k + 1] - rec_off[k]) - 4;
    h.w1 = (uint32_t)in.rid[k];
    h.w2 = (uint32_t)in.pos[k];
    h.w3 = meta[k].bin << 16 | (uint32_t)in.mapq[k] << 8 | ((h.l_name + 1) & 0xffu);
    h.w4 = flag << 16 | (n_cig & 0xffffu);
    h.w5 = h.sl;
}

REC_FN uint32_t rec_code4(uint8_t c, uint32_t rev)          // src/BWAAligner.cpp:208-220: on the reverse strand only A and T change places
{
    return c == 'A' ? (rev ? 8u : 1u) : c == 'C' ? 2u : c == 'G' ? 4u : c == 'T' ? (rev ? 1u : 8u) : 15u;
}

REC_FN uint32_t rec_mask(bool c) { return 0u - (uint32_t)c; }

// byte j of the record (0 = first byte of block_size)
REC_FN uint8_t rec_byte(const rec_hit &h, uint32_t j)
{
    if (j < 36) {
        const uint32_t q = j >> 2;
        // (masks, not a chain of selects: the compiler turns such a chain over the fields into an indexed load of a copy in scratch memory)
        const uint32_t w = (h.w0 & rec_mask(q == 0)) | (h.w1 & rec_mask(q == 1)) | (h.w2 & rec_mask(q == 2)) | (h.w3 & rec_mask(q == 3)) | (h.w4 & rec_mask(q == 4)) | (h.w5 & rec_mask(q == 5)) |
                           rec_mask(q == 6 || q == 7);
        return (uint8_t)(w >> ((j & 3) << 3));
    }
    j -= 36;
    if (j <= h.l_name) return j < h.l_name ? h.name[j] : 0;
    j -= h.l_name + 1;
    if (j < h.cig_bytes) return h.cig[j];
    j -= h.cig_bytes;
    if (j < h.seq_bytes) {
        const uint32_t x = j << 1;
        const uint32_t hi = rec_code4(h.rev ? h.seq[h.sl - 1 - x] : h.seq[x], h.rev);
        const uint32_t lo = x + 1 < h.sl ? rec_code4(h.rev ? h.seq[h.sl - 2 - x] : h.seq[x + 1], h.rev) : 0;
        return (uint8_t)(hi << 4 | lo);
    }
    j -= h.seq_bytes;
    if (j < h.sl) return j == 0 ? 0xff : 0;
    j -= h.sl;
    // NA:i NM:i AS:i, 7 bytes each
    const uint32_t t = j / 7, b = j - t * 7;
    if (b == 0) return t == 1 ? 'N' : t == 0 ? 'N' : 'A';
    if (b == 1) return t == 0 ? 'A' : t == 1 ? 'M' : 'S';
    if (b == 2) return 'i';
    const uint32_t v = (h.na & rec_mask(t == 0)) | (h.nm & rec_mask(t == 1)) | (h.as & rec_mask(t == 2));
    return (uint8_t)(v >> ((b - 3) << 3));
}

// Tile `tile` of the stream: bytes [tile * REC_TILE, ...) of the n_bytes.  lds: REC_TILE bytes, 16-byte aligned, this wave's own.  rec_off: n_hits + 1 offsets.
REC_FN void rec_fill_tile(const rec_in &in, const rec_meta *meta, const int64_t *owner, const unsigned long long *rec_off, uint64_t n_bytes, uint64_t tile,
                          uint8_t *lds, uint8_t *out, int lane, int nlanes)
{
    const uint64_t t0 = tile * REC_TILE;
    if (t0 >= n_bytes) return;
    const uint64_t t1 = t0 + REC_TILE < n_bytes ? t0 + REC_TILE : n_bytes;
    int64_t lo = 0, hi = in.n_hits;          // the last record that starts at or before t0: rec_off rises strictly (a record has 58 bytes at least) and rec_off[0] = 0
    while (hi - lo > 1) {
        const int64_t mid = lo + ((hi - lo) >> 1);
        if (rec_off[mid] <= t0) lo = mid; else hi = mid;
    }
    for (int64_t k = REC_UNIFORM(lo); k < in.n_hits && rec_off[k] < t1; ++k) {
        rec_hit h;
        rec_hit_load(in, meta, owner, rec_off, k, h);
        const uint64_t r0 = rec_off[k], r1 = rec_off[k + 1];
        const uint64_t a = r0 > t0 ? r0 : t0, b = r1 < t1 ? r1 : t1;
        for (uint64_t x = a + (uint64_t)lane; x < b; x += (uint64_t)nlanes) lds[x - t0] = rec_byte(h, (uint32_t)(x - r0));
    }
    REC_SYNC();
    const uint32_t n = (uint32_t)(t1 - t0), n16 = n & ~15u;
    for (uint32_t o = (uint32_t)lane << 4; o < n16; o += (uint32_t)nlanes << 4) {
#if defined(__HIPCC__)
        *reinterpret_cast<uint4 *>(out + t0 + o) = *reinterpret_cast<const uint4 *>(lds + o);
#else
        memcpy(out + t0 + o, lds + o, 16);
#endif
    }
    for (uint32_t o = n16 + (uint32_t)lane; o < n; o += (uint32_t)nlanes) out[t0 + o] = lds[o];          // the ragged tail of the stream's last tile
    REC_SYNC();
}
