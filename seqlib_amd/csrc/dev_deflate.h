// dev_deflate.h -- the encoder side of dev_inflate.h: one BGZF member (at most 0xff00 bytes) into one DEFLATE stream (RFC 1951), the per-member body of
// k_bgzf_deflate (slx_bgzf.hip).  Host-compilable like the inflater (`lane` of `nlanes`, the host build runs lane 0 of 1) so that
// tests/cpp/deflate_host_test.cpp can hold it against zlib under ASan + UBSan before it runs on a GPU.  Restated from the RFC; no library compressor, and
// the member's CRC32 is dev_inflate.h's inf_crc_part.
//
// One wave per member, four phases:
//   1. parse    windows of DEF_WIN positions in input order.  Per window every position looks its 3-byte hash up in a table of 16-bit positions in LDS and
//               extends the candidate (a position of an earlier window: the table is filled after the look-ups); then the window's positions enter the table,
//               the highest position of a slot wins (def_insert: a rule, not arrival order); then the greedy chain "a match at p skips to p + len" is
//               walked over the window's lengths in LDS, the same in every lane, and the chosen positions write their tokens side by side.
//               Literal/length and distance frequencies are counted in LDS as the tokens are written.
//   2. codes    code lengths limited to 15 (7 for the code-length code) by def_code_lengths, every code complete (two symbols at least, zlib's rule);
//               the lengths run-length coded (16/17/18); the exact size in bits.  A stored block when that is not below 5 + n bytes.
//   3. header   lane 0 writes HLIT, HDIST, HCLEN, the code-length code in inf_clorder and the coded lengths.
//   4. tokens   DEF_WIN tokens at a time: bits per token, an exclusive prefix sum over the wave, each lane ORs its bits into a staging buffer in LDS,
//               whole bytes go out; the odd bits are carried into the next turn.
// Deterministic: nothing depends on which lane arrives first (max-insert, counters and ORs commute).  Memory safety: every read of the input is below n,
// every token index below n (a token covers at least one byte), every write of the output is checked against cap.
#pragma once
#include <stdint.h>
#include "dev_inflate.h"

#if defined(__HIPCC__)
#define DEF_ADD(p, v) atomicAdd((p), (v))
#define DEF_OR(p, v) atomicOr((p), (v))
#define DEF_ANY(x) (__ballot((x) ? 1 : 0) != 0ull)
#else
#define DEF_ADD(p, v) (*(p) += (v))
#define DEF_OR(p, v) (*(p) |= (v))
#define DEF_ANY(x) (x)
#endif

enum {
    DEF_OK = 0,
    DEF_E_SPACE = 1,        // the stream does not fit cap bytes
    DEF_E_INTERNAL = 2      // the emitted size differs from the computed one
};

#define DEF_MEMBER 0xff00u      // input bytes of a full BGZF member
#define DEF_WIN 64              // positions per parse window = tokens per emission turn
#define DEF_HASH_BITS 13
#define DEF_MIN_MATCH 3
#define DEF_MAX_MATCH 258
#define DEF_MAX_DIST 32768u     // a member holds up to 65 280 bytes: the cap is explicit
#define DEF_FAR 4096u           // a match of 3 further away than this costs more than its literals (zlib's TOO_FAR)
#define DEF_NL 286
#define DEF_ND 30

struct def_huff {               // work area of def_code_lengths and of the run-length coding; shares its LDS with the hash table, which phase 1 is done with
    uint32_t key[288], iw[288];
    uint16_t ord[288], lpar[288], ipar[288], idep[288];
    uint16_t cnt[16];
    uint16_t cls[DEF_NL + DEF_ND];      // the coded lengths: symbol | extra bits << 5
    int32_t nu;
};

struct def_state {              // 19.8 KiB of LDS per wave
    union { uint16_t tab[1 << DEF_HASH_BITS]; def_huff h; } u;     // position + 1 of the latest string with this hash; 0 = none
    uint32_t lf[DEF_NL + 2], df[DEF_ND + 2], cf[20];                // frequencies: literal/length, distance, code-length code
    uint16_t lcode[DEF_NL], dcode[DEF_ND], ccode[19];               // codes, bit-reversed: as they go into the stream
    uint8_t  llen[DEF_NL + DEF_ND], clen[19];                       // code lengths: literal/length then distance in one row, as the header codes them
    uint16_t wl[DEF_WIN], wd[DEF_WIN];                              // the window's match lengths (0 = literal) and distances - 1
    uint16_t wn[DEF_WIN];                                           // bits per token of an emission turn
    uint32_t obuf[DEF_WIN * 48 / 32 + 8];                           // bits of an emission turn
    uint32_t bits, ncls, opos, carry, bo;
};

// length 3..258 -> symbol - 257, extra bits
INF_FN int def_len_sym(uint32_t len, uint32_t &extra, int &nextra)
{
    const uint32_t x = len - 3;
    if (len == 258) { extra = 0; nextra = 0; return 28; }
    if (x < 8) { extra = 0; nextra = 0; return (int)x; }
    const int nb = 31 - __builtin_clz(x);
    const int s = 4 * (nb - 1) + (int)((x >> (nb - 2)) & 3u);
    nextra = nb - 2;
    extra = x & ((1u << nextra) - 1u);
    return s;
}
// distance 1..32768 -> symbol, extra bits
INF_FN int def_dist_sym(uint32_t dist, uint32_t &extra, int &nextra)
{
    const uint32_t x = dist - 1;
    if (x < 4) { extra = 0; nextra = 0; return (int)x; }
    const int nb = 31 - __builtin_clz(x);
    const int s = 2 * nb + (int)((x >> (nb - 1)) & 1u);
    nextra = nb - 1;
    extra = x & ((1u << nextra) - 1u);
    return s;
}

INF_FN uint32_t def_hash(const uint8_t *p)
{
    const uint32_t v = (uint32_t)p[0] | (uint32_t)p[1] << 8 | (uint32_t)p[2] << 16;
    return (v * 0x9e3779b1u) >> (32 - DEF_HASH_BITS);
}

// bytes that in[a..) and in[b..) share, at most max (b + max <= n, a < b)
INF_FN uint32_t def_match_len(const uint8_t *in, uint32_t a, uint32_t b, uint32_t max)
{
    typedef uint64_t __attribute__((aligned(1), may_alias)) u64u;
    uint32_t k = 0;
    while (k + 8 <= max) {
        const uint64_t x = *(const u64u *)(in + a + k) ^ *(const u64u *)(in + b + k);
        if (x) return k + (uint32_t)(__builtin_ctzll(x) >> 3);
        k += 8;
    }
    while (k < max && in[a + k] == in[b + k]) ++k;
    return k;
}

// Code lengths of at most `limit` bits for the n frequencies freq[] into len[]: a Huffman code over the used symbols (two at least: unused ones of the lowest
// index are drafted, zlib's rule, so the code is complete), depths above the limit folded onto it and the Kraft sum brought back to exactly 1 by moving
// leaves one level down, then the lengths dealt out by weight.  A zero frequency keeps length 0 unless drafted.  n <= 288, 2^limit >= n.
INF_FN void def_code_lengths(const uint32_t *freq, int n, int limit, uint8_t *len, def_huff *h, int lane, int nlanes)
{
    for (int s = lane; s < n; s += nlanes) { h->key[s] = freq[s]; len[s] = 0; }
    INF_SYNC();
    if (lane == 0) {
        int nu = 0;
        for (int s = 0; s < n; ++s) nu += h->key[s] != 0;
        for (int s = 0; s < n && nu < 2; ++s) if (h->key[s] == 0) { h->key[s] = 1; ++nu; }
        h->nu = nu;
        for (int i = 0; i < 16; ++i) h->cnt[i] = 0;
    }
    INF_SYNC();
    const int nu = h->nu;
    // rank sort by (weight, symbol), ascending: each symbol counts the ones before it
    for (int s = lane; s < n; s += nlanes) {
        const uint32_t k = h->key[s];
        if (!k) continue;
        int r = 0;
        for (int t = 0; t < n; ++t) { const uint32_t kt = h->key[t]; r += kt && (kt < k || (kt == k && t < s)); }
        h->ord[r] = (uint16_t)s;
    }
    INF_SYNC();
    if (lane == 0) {
        // Huffman's tree over the sorted leaves with two queues: the leaves, and the internal nodes in the order they are made (their weights ascend)
        int li = 0, ii = 0;
        for (int k = 0; k < nu - 1; ++k) {
            uint32_t w = 0;
            for (int two = 0; two < 2; ++two) {
                if (li < nu && (ii >= k || h->key[h->ord[li]] <= h->iw[ii])) { w += h->key[h->ord[li]]; h->lpar[li++] = (uint16_t)k; }
                else { w += h->iw[ii]; h->ipar[ii++] = (uint16_t)k; }
            }
            h->iw[k] = w;
        }
        h->idep[nu - 2] = 0;
        for (int j = nu - 3; j >= 0; --j) h->idep[j] = (uint16_t)(h->idep[h->ipar[j]] + 1);
        for (int i = 0; i < nu; ++i) { const int d = h->idep[h->lpar[i]] + 1; h->cnt[d < limit ? d : limit]++; }
        uint32_t total = 0;
        for (int i = 1; i <= limit; ++i) total += (uint32_t)h->cnt[i] << (limit - i);
        while (total > (1u << limit)) {             // each turn takes exactly one unit of 2^-limit off the sum
            h->cnt[limit]--;
            for (int i = limit - 1; i > 0; --i) if (h->cnt[i]) { h->cnt[i]--; h->cnt[i + 1] += 2; break; }
            --total;
        }
        int idx = 0;
        for (int l = limit; l >= 1; --l) for (int c = h->cnt[l]; c > 0; --c) len[h->ord[idx++]] = (uint8_t)l;
    }
    INF_SYNC();
}

// canonical codes of the lengths, bit-reversed (Huffman codes enter the stream from their most significant bit)
INF_FN void def_codes(const uint8_t *len, int n, uint16_t *code, int lane)
{
    if (lane != 0) return;
    uint32_t cnt[16], next[16];
    for (int i = 0; i < 16; ++i) cnt[i] = 0;
    for (int s = 0; s < n; ++s) cnt[len[s]]++;
    cnt[0] = 0;
    uint32_t c = 0;
    for (int l = 1; l < 16; ++l) { c = (c + cnt[l - 1]) << 1; next[l] = c; }
    for (int s = 0; s < n; ++s) {
        const int l = len[s];
        uint32_t v = l ? next[l]++ : 0, r = 0;
        for (int i = 0; i < l; ++i) { r = r << 1 | (v & 1u); v >>= 1; }
        code[s] = (uint16_t)r;
    }
}

struct def_bitw { uint8_t *out; uint32_t cap, pos; uint64_t buf; int cnt; int full; };
INF_FN void def_put(def_bitw &w, uint32_t v, int k)     // k <= 16
{
    w.buf |= (uint64_t)v << w.cnt; w.cnt += k;
    while (w.cnt >= 8) {
        if (w.pos < w.cap) w.out[w.pos] = (uint8_t)w.buf; else w.full = 1;
        ++w.pos; w.buf >>= 8; w.cnt -= 8;
    }
}

// bits of token tk (or of the end-of-block symbol) in stream order, at most 48
INF_FN uint64_t def_token_bits(const def_state *t, uint32_t tk, int is_eob, int &nbits)
{
    if (is_eob) { nbits = t->llen[256]; return t->lcode[256]; }
    if (!(tk & 0x80000000u)) { nbits = t->llen[tk]; return t->lcode[tk]; }
    uint32_t e; int ne;
    const int ls = def_len_sym(((tk >> 16) & 0xffu) + 3, e, ne) + 257;
    uint64_t v = t->lcode[ls]; int k = t->llen[ls];
    v |= (uint64_t)e << k; k += ne;
    const int ds = def_dist_sym((tk & 0xffffu) + 1, e, ne);
    v |= (uint64_t)t->dcode[ds] << k; k += t->llen[DEF_NL + ds];
    v |= (uint64_t)e << k; k += ne;
    nbits = k;
    return v;
}

// exclusive prefix sum of t->wn[0, DEF_WIN) in place; returns the total.  Device: one entry per lane (nlanes == DEF_WIN), a shuffle scan; host: a loop.
INF_FN uint32_t def_scan(def_state *t, int lane)
{
#if defined(__HIPCC__)
    const uint32_t own = t->wn[lane];
    uint32_t inc = own;
    for (int o = 1; o < DEF_WIN; o <<= 1) { const uint32_t up = __shfl_up(inc, o, DEF_WIN); if (lane >= o) inc += up; }
    t->wn[lane] = (uint16_t)(inc - own);
    return __shfl(inc, DEF_WIN - 1, DEF_WIN);
#else
    (void)lane;
    uint32_t s = 0;
    for (int i = 0; i < DEF_WIN; ++i) { const uint32_t c = t->wn[i]; t->wn[i] = (uint16_t)s; s += c; }
    return s;
#endif
}

// The table's slots take the window's positions; where several share a slot the highest stays.  Lanes racing for a slot write again until nobody is below
// what the slot holds, so the outcome does not depend on which store the hardware lets through.
INF_FN void def_insert(def_state *t, const uint8_t *in, uint32_t n, uint32_t base, int lane, int nlanes)
{
    for (;;) {
        int wrote = 0;
        for (int i = lane; i < DEF_WIN; i += nlanes) {
            const uint32_t p = base + (uint32_t)i;
            if (p + DEF_MIN_MATCH > n) continue;
            const uint32_t h = def_hash(in + p);
            if (t->u.tab[h] < p + 1) { t->u.tab[h] = (uint16_t)(p + 1); wrote = 1; }
        }
        INF_SYNC();
        if (!DEF_ANY(wrote) || nlanes == 1) break;
    }
}

// in[0, n), n <= DEF_MEMBER, into one DEFLATE stream out[0, *out_len), *out_len <= cap; tok: n words of scratch (one token per input byte at most).
// *stored = 1 when the stream is a stored block.  Returns DEF_OK or a DEF_E_* code, the same in every lane.
INF_FN int def_member(const uint8_t *in, uint32_t n, uint8_t *out, uint32_t cap, uint32_t *tok, def_state *t, int lane, int nlanes, uint32_t *out_len, uint32_t *stored)
{
    // ---- 1. parse
    for (int i = lane; i < (1 << DEF_HASH_BITS); i += nlanes) t->u.tab[i] = 0;
    for (int i = lane; i < DEF_NL + 2; i += nlanes) t->lf[i] = 0;
    for (int i = lane; i < DEF_ND + 2; i += nlanes) t->df[i] = 0;
    for (int i = lane; i < 20; i += nlanes) t->cf[i] = 0;
    if (lane == 0) { t->bits = 0; t->ncls = 0; }
    INF_SYNC();
    uint32_t ntok = 0, start = 0;
    for (uint32_t base = 0; base < n; base += DEF_WIN) {
        const uint32_t wend = base + DEF_WIN < n ? base + DEF_WIN : n;
        if (start < wend) {
            for (int i = lane; i < DEF_WIN; i += nlanes) {
                const uint32_t p = base + (uint32_t)i;
                uint32_t len = 0, dm1 = 0;
                if (p >= start && p + DEF_MIN_MATCH <= n) {
                    const uint32_t c1 = t->u.tab[def_hash(in + p)];
                    if (c1 && p - (c1 - 1) <= DEF_MAX_DIST) {          // c1 - 1 < base <= p: never before the member's first byte, never the position itself
                        const uint32_t c = c1 - 1, room = n - p;
                        len = def_match_len(in, c, p, room < DEF_MAX_MATCH ? room : DEF_MAX_MATCH);
                        dm1 = p - c - 1;
                        if (len < DEF_MIN_MATCH || (len == DEF_MIN_MATCH && dm1 >= DEF_FAR)) len = 0;
                    }
                }
                t->wl[i] = (uint16_t)len; t->wd[i] = (uint16_t)dm1;
            }
            INF_SYNC();
        }
        def_insert(t, in, n, base, lane, nlanes);
        if (start >= wend) continue;
        uint64_t sel = 0;                               // the greedy chain through the window, walked alike by every lane
        uint32_t cur = start;
        while (cur < wend) { const uint32_t i = cur - base, l = t->wl[i]; sel |= 1ull << i; cur += l ? l : 1u; }
        start = cur;
        for (int i = lane; i < DEF_WIN; i += nlanes) {
            if (!((sel >> i) & 1ull)) continue;
            const uint32_t at = ntok + (uint32_t)__builtin_popcountll(sel & ((1ull << i) - 1ull));       // < n: every token before it covers a byte before base + i
            const uint32_t l = t->wl[i];
            uint32_t e; int ne;
            if (l) {
                tok[at] = 0x80000000u | (l - 3) << 16 | t->wd[i];
                DEF_ADD(&t->lf[257 + def_len_sym(l, e, ne)], 1u);
                DEF_ADD(&t->df[def_dist_sym((uint32_t)t->wd[i] + 1, e, ne)], 1u);
            } else {
                const uint32_t b = in[base + (uint32_t)i];
                tok[at] = b;
                DEF_ADD(&t->lf[b], 1u);
            }
        }
        ntok += (uint32_t)__builtin_popcountll(sel);
        INF_SYNC();                                     // wl / wd are written again by the next window
    }
    if (lane == 0) t->lf[256] = 1;
    INF_SYNC();

    // ---- 2. codes and the size
    def_huff *h = &t->u.h;
    def_code_lengths(t->lf, DEF_NL, 15, t->llen, h, lane, nlanes);
    def_code_lengths(t->df, DEF_ND, 15, t->llen + DEF_NL, h, lane, nlanes);
    int nl = DEF_NL, nd = DEF_ND;
    while (nl > 257 && t->llen[nl - 1] == 0) --nl;
    while (nd > 1 && t->llen[DEF_NL + nd - 1] == 0) --nd;
    if (lane == 0) {
        // the nl + nd lengths as one row, run-length coded: 16 = the length before 3..6 times, 17 = 3..10 zeros, 18 = 11..138 zeros
        uint32_t k = 0;
        const int tot = nl + nd;
        int i = 0;
        while (i < tot) {
            const int v = i < nl ? t->llen[i] : t->llen[DEF_NL + i - nl];
            int run = 1;
            while (i + run < tot && (i + run < nl ? t->llen[i + run] : t->llen[DEF_NL + i + run - nl]) == v) ++run;
            i += run;
            if (v == 0) {
                while (run >= 11) { const int r = run < 138 ? run : 138; h->cls[k++] = (uint16_t)(18 | (r - 11) << 5); t->cf[18]++; run -= r; }
                if (run >= 3) { h->cls[k++] = (uint16_t)(17 | (run - 3) << 5); t->cf[17]++; run = 0; }
                while (run-- > 0) { h->cls[k++] = 0; t->cf[0]++; }
            } else {
                h->cls[k++] = (uint16_t)v; t->cf[v]++; --run;
                while (run >= 3) { const int r = run < 6 ? run : 6; h->cls[k++] = (uint16_t)(16 | (r - 3) << 5); t->cf[16]++; run -= r; }
                while (run-- > 0) { h->cls[k++] = (uint16_t)v; t->cf[v]++; }
            }
        }
        t->ncls = k;
    }
    INF_SYNC();
    // (the coded lengths in h->cls lie behind the fields def_code_lengths works in)
    def_code_lengths(t->cf, 19, 7, t->clen, h, lane, nlanes);
    int nc = 19;
    while (nc > 4 && t->clen[inf_clorder[nc - 1]] == 0) --nc;
    const uint32_t ncls = t->ncls;
    {
        uint32_t b = 0;
        for (int s = lane; s < DEF_NL; s += nlanes) b += t->lf[s] * (uint32_t)(t->llen[s] + (s >= 257 ? inf_lext[s - 257] : 0));
        for (int s = lane; s < DEF_ND; s += nlanes) b += t->df[s] * (uint32_t)(t->llen[DEF_NL + s] + inf_dext[s]);
        for (int s = lane; s < 19; s += nlanes) b += t->cf[s] * (uint32_t)(t->clen[s] + (s == 16 ? 2 : s == 17 ? 3 : s == 18 ? 7 : 0));
        if (lane == 0) b += 3 + 5 + 5 + 4 + 3 * (uint32_t)nc;
        DEF_ADD(&t->bits, b);
    }
    def_codes(t->llen, DEF_NL, t->lcode, lane);
    def_codes(t->llen + DEF_NL, DEF_ND, t->dcode, lane);
    def_codes(t->clen, 19, t->ccode, lane);
    INF_SYNC();
    const uint32_t bytes = (t->bits + 7) >> 3;

    if (bytes >= 5 + n) {                               // stored: BFINAL = 1, BTYPE = 00, LEN, ~LEN, the bytes
        *stored = 1; *out_len = 5 + n;
        if (5 + n > cap) return DEF_E_SPACE;
        if (lane == 0) { out[0] = 1; out[1] = (uint8_t)n; out[2] = (uint8_t)(n >> 8); out[3] = (uint8_t)~n; out[4] = (uint8_t)(~n >> 8); }
        for (uint32_t i = (uint32_t)lane; i < n; i += (uint32_t)nlanes) out[5 + i] = in[i];
        return DEF_OK;
    }
    *stored = 0; *out_len = bytes;
    if (bytes > cap) return DEF_E_SPACE;

    // ---- 3. the block header
    if (lane == 0) {
        def_bitw w; w.out = out; w.cap = bytes; w.pos = 0; w.buf = 0; w.cnt = 0; w.full = 0;
        def_put(w, 1, 1); def_put(w, 2, 2);
        def_put(w, (uint32_t)(nl - 257), 5); def_put(w, (uint32_t)(nd - 1), 5); def_put(w, (uint32_t)(nc - 4), 4);
        for (int i = 0; i < nc; ++i) def_put(w, t->clen[inf_clorder[i]], 3);
        for (uint32_t i = 0; i < ncls; ++i) {
            const uint32_t s = h->cls[i] & 31u, e = h->cls[i] >> 5;
            def_put(w, t->ccode[s], t->clen[s]);
            if (s >= 16) def_put(w, e, s == 16 ? 2 : s == 17 ? 3 : 7);
        }
        t->opos = w.full ? 0xffffffffu : w.pos; t->carry = (uint32_t)w.buf & 0xffu; t->bo = (uint32_t)w.cnt;
    }
    INF_SYNC();
    uint32_t opos = t->opos, carry = t->carry, bo = t->bo;
    if (opos == 0xffffffffu) return DEF_E_INTERNAL;

    // ---- 4. the tokens and the end-of-block symbol
    const int nob = (int)(sizeof t->obuf / sizeof t->obuf[0]);
    for (uint32_t b0 = 0; b0 <= ntok; b0 += DEF_WIN) {
        for (int i = lane; i < nob; i += nlanes) t->obuf[i] = i == 0 ? carry : 0u;
        INF_SYNC();
        for (int i = lane; i < DEF_WIN; i += nlanes) {
            const uint32_t k = b0 + (uint32_t)i;
            int nb = 0;
            if (k <= ntok) (void)def_token_bits(t, k < ntok ? tok[k] : 0u, k == ntok, nb);
            t->wn[i] = (uint16_t)nb;
        }
        INF_SYNC();
        const uint32_t total = def_scan(t, lane);
        INF_SYNC();
        for (int i = lane; i < DEF_WIN; i += nlanes) {
            const uint32_t k = b0 + (uint32_t)i;
            if (k > ntok) continue;
            int nb;
            const uint64_t v = def_token_bits(t, k < ntok ? tok[k] : 0u, k == ntok, nb);
            const uint32_t at = bo + t->wn[i], wi = at >> 5, sh = at & 31u;
            DEF_OR(&t->obuf[wi], (uint32_t)(v << sh));
            const uint64_t hi = sh ? v >> (32 - sh) : v >> 32;      // what the first word did not take
            if ((uint32_t)hi) DEF_OR(&t->obuf[wi + 1], (uint32_t)hi);
            if (hi >> 32) DEF_OR(&t->obuf[wi + 2], (uint32_t)(hi >> 32));
        }
        INF_SYNC();
        const uint32_t full = (bo + total) >> 3;
        if (opos + full > bytes) return DEF_E_INTERNAL;         // bytes <= cap
        for (uint32_t i = (uint32_t)lane; i < full; i += (uint32_t)nlanes) out[opos + i] = (uint8_t)(t->obuf[i >> 2] >> (8 * (i & 3u)));
        carry = (t->obuf[full >> 2] >> (8 * (full & 3u))) & 0xffu;
        opos += full; bo = (bo + total) & 7u;
        INF_SYNC();                                             // obuf is cleared by the next turn
    }
    if (bo) {
        if (opos + 1 > bytes) return DEF_E_INTERNAL;
        if (lane == 0) out[opos] = (uint8_t)carry;
        ++opos;
    }
    return opos == bytes ? DEF_OK : DEF_E_INTERNAL;
}

// the 18 bytes before the DEFLATE stream of a BGZF member of `total` bytes in all (RFC 1952 with the "BC" extra field, SAMv1 4.1)
INF_FN void def_bgzf_header(uint8_t *m, uint32_t total)
{
    const uint8_t head[16] = {0x1f, 0x8b, 8, 4, 0, 0, 0, 0, 0, 0xff, 6, 0, 'B', 'C', 2, 0};
    for (int i = 0; i < 16; ++i) m[i] = head[i];
    m[16] = (uint8_t)(total - 1); m[17] = (uint8_t)((total - 1) >> 8);
}
// the 8 bytes behind it
INF_FN void def_bgzf_trailer(uint8_t *m, uint32_t crc, uint32_t isize)
{
    for (int i = 0; i < 4; ++i) { m[i] = (uint8_t)(crc >> (8 * i)); m[4 + i] = (uint8_t)(isize >> (8 * i)); }
}
