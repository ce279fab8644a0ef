// dev_inflate.h -- DEFLATE (RFC 1951) of one BGZF member and the CRC32 (RFC 1952) of its output: the per-member bodies of k_bgzf_inflate and
// k_bgzf_crc (slx_bam.hip), kept apart and host-compilable so that tests/cpp/inflate_host_test.cpp can hold them against zlib under ASan + UBSan
// before they ever run on a GPU.  Restated from the RFCs; no library decompressor.
//
// Work split inside a wave (`lane` of `nlanes`; the host build runs it as lane 0 of 1, and tests/cpp/inflate_lanes_test.cpp as 7 and 64 threads under ThreadSanitizer):
//   * the bit stream is decoded redundantly by every lane: one address per load (a broadcast), wave-uniform control flow, no cross-lane traffic per symbol;
//   * the decode tables live in LDS, built per deflate block: lane 0 counts and sorts the code lengths (the canonical order), then all lanes fill the
//     first-level lookup tables (10 bits literal/length, 8 bits distance), each entry by a canonical decode of its own index;
//   * a literal is stored by lane 0; a match is copied by the whole wave, out[p + i] = out[p - dist + i % dist] (exact for dist < len), a stored block likewise.
// Memory safety: every read is checked against the member's compressed size (bits past its end read as zero and end the member with INF_E_EOF at the next
// check), every write against its ISIZE; a malformed stream ends the member with a code below and never loops: each turn of each loop consumes input or ends.
#pragma once
#include <stdint.h>
#if defined(__HIPCC__)
#define INF_FN __device__ __forceinline__
#define INF_TAB __device__ const
// lanes of one wave exchange data through LDS / the member's own output: order the accesses (no instruction on this target, a barrier to the compiler)
#define INF_SYNC() do { __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront"); __builtin_amdgcn_wave_barrier(); __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront"); } while (0)
#else
#define INF_FN static inline
#define INF_TAB static const
#ifndef INF_SYNC        // tests/cpp/inflate_lanes_test.cpp runs the lanes as threads and makes this a barrier
#define INF_SYNC() do { } while (0)
#endif
#endif

enum {
    INF_OK = 0,
    INF_E_EOF = 1,      // the compressed bytes end inside the stream
    INF_E_BTYPE = 2,    // block type 3
    INF_E_STORED = 3,   // stored block: LEN != ~NLEN, or its bytes pass the end of the input
    INF_E_CODE = 4,     // over-subscribed or incomplete code, bad repeat in the code lengths, no end-of-block code, a bit pattern no code has
    INF_E_SYM = 5,      // length symbol 286/287 or distance symbol 30/31
    INF_E_DIST = 6,     // distance reaches before the start of the member's output
    INF_E_OUT = 7,      // output would pass ISIZE
    INF_E_ISIZE = 8,    // stream ended with fewer than ISIZE bytes
    INF_E_CRC = 9,      // CRC32 of the output differs from the trailer (set by k_bgzf_crc)
    INF_E_DESC = 10     // the member's descriptor points outside the buffers (set by the kernels)
};

#define INF_FAST_L 10
#define INF_FAST_D 8

struct inf_tables {                 // 3 664 bytes of LDS per wave
    uint16_t fast_l[1 << INF_FAST_L];   // (symbol << 4) | code length, 0 = longer than INF_FAST_L bits (or no code): canonical decode
    uint16_t fast_d[1 << INF_FAST_D];
    uint16_t sym_l[288], sym_d[32];     // symbols in canonical order
    uint16_t cnt_l[16], cnt_d[16];      // codes per length
    uint16_t offs[16];
    uint8_t  lens[320];
    int32_t  status;
};

struct inf_bits {
    const uint8_t *in;
    uint32_t n, pos;
    uint64_t buf;
    int cnt;                            // valid bits in buf; negative = the decoder took bits that the input does not have
};

INF_TAB uint16_t inf_lbase[29] = {3, 4, 5, 6, 7, 8, 9, 10, 11, 13, 15, 17, 19, 23, 27, 31, 35, 43, 51, 59, 67, 83, 99, 115, 131, 163, 195, 227, 258};
INF_TAB uint8_t  inf_lext[29] = {0, 0, 0, 0, 0, 0, 0, 0, 1, 1, 1, 1, 2, 2, 2, 2, 3, 3, 3, 3, 4, 4, 4, 4, 5, 5, 5, 5, 0};
INF_TAB uint16_t inf_dbase[30] = {1, 2, 3, 4, 5, 7, 9, 13, 17, 25, 33, 49, 65, 97, 129, 193, 257, 385, 513, 769, 1025, 1537, 2049, 3073, 4097, 6145, 8193, 12289, 16385, 24577};
INF_TAB uint8_t  inf_dext[30] = {0, 0, 0, 0, 1, 1, 2, 2, 3, 3, 4, 4, 5, 5, 6, 6, 7, 7, 8, 8, 9, 9, 10, 10, 11, 11, 12, 12, 13, 13};
INF_TAB uint8_t  inf_clorder[19] = {16, 17, 18, 0, 8, 7, 9, 6, 10, 5, 11, 4, 12, 3, 13, 2, 14, 1, 15};

// tops the bit buffer up to at least 56 bits while the input lasts
INF_FN void inf_refill(inf_bits &b)
{
    if (b.pos + 8 <= b.n) {
        typedef uint64_t __attribute__((aligned(1))) u64u;
        b.buf |= *(const u64u *)(b.in + b.pos) << b.cnt;            // bits above cnt are the stream's next ones: OR-ing them again later is idempotent
        const int adv = (63 - b.cnt) >> 3;
        b.pos += (uint32_t)adv;
        b.cnt += adv << 3;
    } else {
        while (b.cnt <= 56 && b.pos < b.n) { b.buf |= (uint64_t)b.in[b.pos++] << b.cnt; b.cnt += 8; }
    }
}
INF_FN uint32_t inf_take(inf_bits &b, int n)            // n <= 16
{
    const uint32_t v = (uint32_t)b.buf & ((1u << n) - 1u);
    b.buf >>= n; b.cnt -= n;
    return v;
}

// canonical Huffman decode of the code that starts at bit 0 of `bits`, codes of up to maxlen bits: symbol, or -1
INF_FN int inf_decode_slow(uint32_t bits, const uint16_t *cnt, const uint16_t *sym, int maxlen, int &len_out)
{
    int code = 0, first = 0, index = 0;
    for (int len = 1; len <= maxlen; ++len) {
        code |= (int)(bits & 1u); bits >>= 1;
        const int c = cnt[len];
        if (code - c < first) { len_out = len; return sym[index + (code - first)]; }
        index += c; first += c; first <<= 1; code <<= 1;
    }
    len_out = 0;
    return -1;
}

// tables of one code from the n code lengths in lens[]: INF_OK, or INF_E_CODE for an over-subscribed code or an incomplete one of more than one symbol
INF_FN int inf_build(inf_tables *t, const uint8_t *lens, int n, uint16_t *cnt, uint16_t *sym, uint16_t *fast, int fast_bits, int lane, int nlanes)
{
    if (lane == 0) {
        for (int i = 0; i < 16; ++i) cnt[i] = 0;
        for (int s = 0; s < n; ++s) cnt[lens[s] & 15]++;
        int left = 1, bad = 0;
        for (int len = 1; len <= 15; ++len) { left <<= 1; left -= cnt[len]; if (left < 0) { bad = 1; break; } }
        if (!bad && left > 0 && n != cnt[0] + cnt[1]) bad = 1;          // incomplete: only a single one-bit code may be
        t->offs[1] = 0;
        for (int len = 1; len < 15; ++len) t->offs[len + 1] = (uint16_t)(t->offs[len] + cnt[len]);
        if (!bad)
            for (int s = 0; s < n; ++s) { const int l = lens[s] & 15; if (l) sym[t->offs[l]++] = (uint16_t)s; }
        t->status = bad;
    }
    INF_SYNC();
    if (t->status) return INF_E_CODE;
    for (int i = lane; i < (1 << fast_bits); i += nlanes) {
        int l;
        const int s = inf_decode_slow((uint32_t)i, cnt, sym, fast_bits, l);
        fast[i] = s >= 0 ? (uint16_t)((s << 4) | l) : (uint16_t)0;
    }
    INF_SYNC();
    return INF_OK;
}

// one symbol of a code off the bit buffer (at least 15 bits topped up, zero bits past the end of the input); -1 = no code has this pattern
INF_FN int inf_sym(inf_bits &b, const uint16_t *fast, int fast_bits, const uint16_t *cnt, const uint16_t *sym)
{
    const uint32_t e = fast[(uint32_t)b.buf & ((1u << fast_bits) - 1u)];
    int s, l;
    if (e) { s = (int)(e >> 4); l = (int)(e & 15u); }
    else {
        s = inf_decode_slow((uint32_t)b.buf & 0x7fffu, cnt, sym, 15, l);
        if (s < 0) return -1;
    }
    b.buf >>= l; b.cnt -= l;
    return s;
}

// literal/length + distance symbols of one block into out[p..); leaves at the end-of-block symbol
INF_FN int inf_codes(inf_bits &b, inf_tables *t, uint8_t *out, uint32_t out_len, uint32_t &p, int lane, int nlanes)
{
    for (;;) {
        inf_refill(b);                                  // >= 56 bits while input lasts; one turn takes at most 15 + 5 + 15 + 13
        int s = inf_sym(b, t->fast_l, INF_FAST_L, t->cnt_l, t->sym_l);
        if (s < 0) return INF_E_CODE;
        if (s < 256) {
            if (b.cnt < 0) return INF_E_EOF;
            if (p >= out_len) return INF_E_OUT;
            if (lane == 0) out[p] = (uint8_t)s;
            ++p;
            continue;
        }
        if (s == 256) return b.cnt < 0 ? INF_E_EOF : INF_OK;
        s -= 257;
        if (s >= 29) return INF_E_SYM;
        const uint32_t len = inf_lbase[s] + inf_take(b, inf_lext[s]);
        const int ds = inf_sym(b, t->fast_d, INF_FAST_D, t->cnt_d, t->sym_d);
        if (ds < 0) return INF_E_CODE;
        if (ds >= 30) return INF_E_SYM;
        const uint32_t dist = inf_dbase[ds] + inf_take(b, inf_dext[ds]);
        if (b.cnt < 0) return INF_E_EOF;
        if (dist > p) return INF_E_DIST;
        if (len > out_len - p) return INF_E_OUT;
        INF_SYNC();                                     // the bytes behind p were stored by other lanes
        const uint8_t *src = out + (p - dist);
        uint8_t *dst = out + p;
        if (dist >= len) { for (uint32_t i = (uint32_t)lane; i < len; i += (uint32_t)nlanes) dst[i] = src[i]; }
        else if (dist == 1) { const uint8_t v = src[0]; for (uint32_t i = (uint32_t)lane; i < len; i += (uint32_t)nlanes) dst[i] = v; }
        else { for (uint32_t i = (uint32_t)lane; i < len; i += (uint32_t)nlanes) dst[i] = src[i % dist]; }
        p += len;
    }
}

// The deflate stream in[0, in_len) of one member into out[0, out_len); out_len is the member's ISIZE.  Returns INF_OK or an INF_E_* code, the same in every lane.
INF_FN int inf_member(const uint8_t *in, uint32_t in_len, uint8_t *out, uint32_t out_len, inf_tables *t, int lane, int nlanes)
{
    inf_bits b;
    b.in = in; b.n = in_len; b.pos = 0; b.buf = 0; b.cnt = 0;
    uint32_t p = 0;
    for (;;) {
        inf_refill(b);
        const uint32_t last = inf_take(b, 1), type = inf_take(b, 2);
        if (b.cnt < 0) return INF_E_EOF;
        if (type == 0) {
            inf_take(b, b.cnt & 7);
            inf_refill(b);
            if (b.cnt < 32) return INF_E_EOF;
            const uint32_t len = inf_take(b, 16), nlen = inf_take(b, 16);
            if (len != (~nlen & 0xffffu)) return INF_E_STORED;
            const uint32_t at = b.pos - (uint32_t)(b.cnt >> 3);         // whole bytes still in the buffer go back to the input
            b.buf = 0; b.cnt = 0;
            if (len > in_len - at) return INF_E_STORED;
            if (len > out_len - p) return INF_E_OUT;
            for (uint32_t i = (uint32_t)lane; i < len; i += (uint32_t)nlanes) out[p + i] = in[at + i];
            p += len;
            b.pos = at + len;
        } else if (type == 1) {
            INF_SYNC();                                                 // (tables of the block before are no longer read)
            for (int i = lane; i < 288; i += nlanes) t->lens[i] = (uint8_t)(i < 144 ? 8 : i < 256 ? 9 : i < 280 ? 7 : 8);
            for (int i = lane; i < 32; i += nlanes) t->lens[288 + i] = 5;          // (30 and 31 take part in the code and are refused as symbols)
            INF_SYNC();
            int e = inf_build(t, t->lens, 288, t->cnt_l, t->sym_l, t->fast_l, INF_FAST_L, lane, nlanes);
            if (e) return e;
            e = inf_build(t, t->lens + 288, 32, t->cnt_d, t->sym_d, t->fast_d, INF_FAST_D, lane, nlanes);
            if (e) return e;
            e = inf_codes(b, t, out, out_len, p, lane, nlanes);
            if (e) return e;
        } else if (type == 2) {
            const int nl = (int)inf_take(b, 5) + 257, nd = (int)inf_take(b, 5) + 1, nc = (int)inf_take(b, 4) + 4;
            if (b.cnt < 0) return INF_E_EOF;
            if (nl > 286 || nd > 30) return INF_E_CODE;
            INF_SYNC();
            if (lane == 0) for (int i = 0; i < 19; ++i) t->lens[i] = 0;
            for (int i = 0; i < nc; ++i) {
                if ((i & 7) == 0) { if (b.cnt < 0) return INF_E_EOF; inf_refill(b); }
                const uint32_t v = inf_take(b, 3);
                if (lane == 0) t->lens[inf_clorder[i]] = (uint8_t)v;
            }
            if (b.cnt < 0) return INF_E_EOF;
            INF_SYNC();
            int e = inf_build(t, t->lens, 19, t->cnt_d, t->sym_d, t->fast_d, 7, lane, nlanes);     // the code-length code borrows the distance tables
            if (e) return e;
            int idx = 0, prev = 0, has_eob = 0;
            while (idx < nl + nd) {
                inf_refill(b);
                const int s = inf_sym(b, t->fast_d, 7, t->cnt_d, t->sym_d);
                if (s < 0) return INF_E_CODE;
                int rep = 1, v = s;
                if (s == 16) { if (idx == 0) return INF_E_CODE; v = prev; rep = 3 + (int)inf_take(b, 2); }
                else if (s == 17) { v = 0; rep = 3 + (int)inf_take(b, 3); }
                else if (s == 18) { v = 0; rep = 11 + (int)inf_take(b, 7); }
                if (b.cnt < 0) return INF_E_EOF;
                if (idx + rep > nl + nd) return INF_E_CODE;
                if (v && idx <= 256 && idx + rep > 256) has_eob = 1;
                if (lane == 0) for (int k = 0; k < rep; ++k) t->lens[idx + k] = (uint8_t)v;
                idx += rep;
                prev = v;
            }
            if (!has_eob) return INF_E_CODE;
            INF_SYNC();
            e = inf_build(t, t->lens, nl, t->cnt_l, t->sym_l, t->fast_l, INF_FAST_L, lane, nlanes);
            if (e) return e;
            e = inf_build(t, t->lens + nl, nd, t->cnt_d, t->sym_d, t->fast_d, INF_FAST_D, lane, nlanes);
            if (e) return e;
            e = inf_codes(b, t, out, out_len, p, lane, nlanes);
            if (e) return e;
        } else return INF_E_BTYPE;
        if (last) break;
    }
    return p == out_len ? INF_OK : INF_E_ISIZE;
}

// ---- CRC32 (reflected 0xedb88320), a member split into one slice per lane: crc(A ++ B) = crc(A) * x^(8|B|) mod P  xor  crc(B) (zlib's crc32_combine) ----
#define INF_CRC_POLY 0xedb88320u
INF_FN uint32_t inf_crc_entry(uint32_t i)
{
    for (int k = 0; k < 8; ++k) i = (i & 1u) ? (i >> 1) ^ INF_CRC_POLY : i >> 1;
    return i;
}
INF_FN uint32_t inf_crc_bytes(const uint32_t *tab, const uint8_t *p, uint32_t n)
{
    uint32_t c = 0xffffffffu;
    for (uint32_t i = 0; i < n; ++i) c = tab[(c ^ p[i]) & 0xffu] ^ (c >> 8);
    return ~c;
}
INF_FN uint32_t inf_gf_mul(uint32_t a, uint32_t b)      // a * b mod P, polynomials with x^0 in bit 31
{
    uint32_t p = 0;
    for (uint32_t m = 0x80000000u; m; m >>= 1) {
        if (a & m) p ^= b;
        b = (b & 1u) ? (b >> 1) ^ INF_CRC_POLY : b >> 1;
    }
    return p;
}
INF_FN uint32_t inf_crc_shift(uint32_t crc, uint32_t nbytes)      // crc * x^(8 nbytes) mod P
{
    uint32_t sq = 0x00800000u;      // x^8
    while (nbytes) {
        if (nbytes & 1u) crc = inf_gf_mul(sq, crc);
        sq = inf_gf_mul(sq, sq);
        nbytes >>= 1;
    }
    return crc;
}
// lane's share of the CRC32 of p[0, n): the xor over all lanes is the member's CRC32
INF_FN uint32_t inf_crc_part(const uint32_t *tab, const uint8_t *p, uint32_t n, int lane, int nlanes)
{
    const uint32_t per = (n + (uint32_t)nlanes - 1u) / (uint32_t)nlanes;
    const uint32_t a = (uint32_t)lane * per < n ? (uint32_t)lane * per : n;
    const uint32_t e = a + per < n ? a + per : n;
    if (e == a) return 0;
    return inf_crc_shift(inf_crc_bytes(tab, p + a, e - a), n - e);
}

#if defined(__HIPCC__)
// ---- members of a mapped BGZF file staged, inflated by k_bgzf_inflate and checked by k_bgzf_crc (slx_bam.hip): for every reader of BGZF (slx_bam.hip, slx_fastq.hip) ----
#include "slx_hip.h"
#include "seqlib_amd_bam.h"
// one member: its deflate stream lies at comp + in_off (in_len bytes), its isize bytes go to out + out_off, crc is its trailer's
struct bam_mdesc { uint64_t in_off, out_off; uint32_t in_len, isize, crc, pad; };
// what a reader keeps for the call below: the members' compressed bytes, their descriptors and their error words, pinned and in HBM (1/4 + 256: kept as found)
struct bgzf_stage {
    SlxPinBuf<SlxMargin<4, 256>> h_comp, h_desc, h_err;
    SlxDevBuf<SlxMargin<4, 256>> d_comp, d_desc, d_err;
    void release() { h_comp.release(); h_desc.release(); h_err.release(); d_comp.release(); d_desc.release(); d_err.release(); }
};
// Members [a, b) of mem, whose bytes lie in the mapped file `map`, inflated to d_out[dst_off ..) one behind the other and CRC-checked, one wave per member; d_out
// holds out_bytes (SLX_EINTERNAL when the members do not fit).  Returns after st has drained; SLX_EIO names the first member that does not inflate (path is the
// file's name in that message).  us[0] += the inflate kernel's microseconds (ev0 .. ev_mid), us[1] += the CRC kernel's (ev_mid .. ev1); without ev_mid us[0] takes both.
int slx_bgzf_inflate_members(const uint8_t *map, const char *path, const slx_bam_member *mem, int64_t a, int64_t b, bgzf_stage &S, uint8_t *d_out, uint64_t dst_off,
                             uint64_t out_bytes, hipStream_t st, hipEvent_t ev0, hipEvent_t ev_mid, hipEvent_t ev1, float us[2]);
#endif
