// dev_sam.h -- one SAM line -> one block_size-prefixed BAM record (SAMv1 sections 1.4, 1.5, 4.2; the rules are listed in include/seqlib_amd_sam.h).  The per-line body
// compiles for the GPU (k_sam_size, k_sam_fill of slx_sam.hip) and for the host (sam_host.h, tests/cpp/sam_host_test.cpp): there is ONE statement of the grammar in C,
// and the host parser is this body with a floating-point reader plugged in.  A line is taken in two steps:
//   sam_fields    where the eleven mandatory fields start, where the optional ones begin, and whether a QUAL byte lies outside [33, 126]   (the kernel's version of this
//                 step is wave-cooperative: sam_fields_wave in slx_sam.hip; both fill the same sam_fld)
//   sam_record    every rule of the grammar over the short fields; with out == nullptr the record's size only, otherwise the record.  `lane` of `nl` lanes call it with the
//                 same arguments: the bulk (QNAME, SEQ two bases per byte, QUAL - 33) is spread over the lanes, everything else is written by lane 0.
// Verdicts: SAM_FAST the record is decided here; SAM_SLOW the line carries an f, d or B:f field and FL cannot read floating-point text (the GPU); SAM_ERROR with *err.
#pragma once
#include <stdint.h>
#if defined(__HIPCC__)
#define SAM_FN __host__ __device__ __forceinline__
#define SAM_MEMBER __host__ __device__
#else
#define SAM_FN static inline
#define SAM_MEMBER
#endif

enum { SAM_FAST = 0, SAM_SLOW = 1, SAM_ERROR = 2 };
enum {
    SAM_E_NONE = 0, SAM_E_EMPTY, SAM_E_AT, SAM_E_FIELDS, SAM_E_EMPTY_FIELD, SAM_E_QNAME, SAM_E_FLAG, SAM_E_RNAME, SAM_E_POS, SAM_E_MAPQ, SAM_E_CIGAR, SAM_E_CIGAR_LEN,
    SAM_E_CIGAR_OPS, SAM_E_RNEXT, SAM_E_PNEXT, SAM_E_TLEN, SAM_E_CIGAR_SEQ, SAM_E_QUAL_LEN, SAM_E_QUAL_BYTE, SAM_E_AUX_FORM, SAM_E_AUX_A, SAM_E_AUX_I, SAM_E_AUX_H,
    SAM_E_AUX_F, SAM_E_AUX_B_SUB, SAM_E_AUX_B_ELEM, SAM_E_AUX_TYPE, SAM_E_CR, SAM_E_LONG, SAM_E_COUNT
};
#define SAM_MAX_LINE (1u << 30)          // a longer line is SAM_E_LONG: its record could pass block_size's int32

// the header's reference names, sorted by bytes (a shorter name before its extensions), one entry per distinct name (the first @SQ line that carries it)
struct sam_refs {
    const uint8_t *names;          // the names one behind the other
    const uint32_t *off;           // n + 1 offsets into names
    const int32_t *tid;            // n
    int32_t n;
};

struct sam_fld {
    uint32_t f[12];                // f[i], i < 11: first byte of mandatory field i; f[11]: the byte behind QUAL (a tab, or the line's end)
    uint32_t nf;                   // fields found, at most 12 (12 = there are optional fields)
    uint32_t flags;                // 1: a byte of QUAL lies outside [33, 126]
};

SAM_FN int sam_fields(const uint8_t *s, uint32_t n, sam_fld *F)
{
    uint32_t k = 1;
    F->f[0] = 0; F->flags = 0;
    for (uint32_t i = 0; i < n; ++i)
        if (s[i] == '\t') {
            if (k <= 10) F->f[k++] = i + 1;
            else { F->f[11] = i; k = 12; break; }
        }
    if (k == 11) F->f[11] = n;
    F->nf = k;
    if (k >= 11)
        for (uint32_t i = F->f[10]; i < F->f[11]; ++i)
            if (s[i] < 33 || s[i] > 126) { F->flags = 1; break; }
    return (int)k;
}

// line k of the L lines whose starts are off[0 .. L] (off[k + 1] - 1 = the line feed, or with virt, for the last line, the end of the input): its first byte and its
// length without the one CR before the line feed.  A line longer than SAM_MAX_LINE gives SAM_MAX_LINE + 1; *cr: the input ends in a CR without a line feed.
SAM_FN void sam_line_span(const uint8_t *text, const unsigned long long *off, uint64_t k, uint64_t L, int virt, uint64_t *beg, uint32_t *n, bool *cr)
{
    const uint64_t b = off[k];
    uint64_t e = off[k + 1] - 1;
    *cr = false;
    if (e > b && text[e - 1] == '\r') { if (virt && k + 1 == L) *cr = true; else --e; }
    *beg = b;
    *n = e - b > SAM_MAX_LINE ? SAM_MAX_LINE + 1u : (uint32_t)(e - b);
}

SAM_FN int32_t sam_ref_find(const sam_refs &R, const uint8_t *s, uint32_t len)          // the tid, or -2
{
    int32_t lo = 0, hi = R.n;
    while (lo < hi) {
        const int32_t mid = (lo + hi) >> 1;
        const uint8_t *m = R.names + R.off[mid];
        const uint32_t ml = R.off[mid + 1] - R.off[mid];
        int c = 0;
        for (uint32_t i = 0; i < ml && i < len && !c; ++i) c = (int)m[i] - (int)s[i];
        if (!c) c = ml < len ? -1 : ml > len ? 1 : 0;
        if (!c) return R.tid[mid];
        if (c < 0) lo = mid + 1; else hi = mid;
    }
    return -2;
}

// s[a, b): one digit or more, value <= max
SAM_FN bool sam_uint(const uint8_t *s, uint32_t a, uint32_t b, uint64_t max, uint64_t *v)
{
    if (a >= b) return false;
    uint64_t x = 0;
    for (uint32_t i = a; i < b; ++i) {
        const uint32_t d = (uint32_t)s[i] - '0';
        if (d > 9) return false;
        x = x * 10 + d;
        if (x > max) return false;          // (max < 2^60: x never wraps)
    }
    *v = x;
    return true;
}
// s[a, b): [-+]?digits, lo <= value <= hi (lo <= 0 <= hi)
SAM_FN bool sam_int(const uint8_t *s, uint32_t a, uint32_t b, int64_t lo, int64_t hi, int64_t *v)
{
    bool neg = false;
    if (a < b && (s[a] == '-' || s[a] == '+')) { neg = s[a] == '-'; ++a; }
    uint64_t x = 0;
    if (!sam_uint(s, a, b, neg ? (uint64_t)(-lo) : (uint64_t)hi, &x)) return false;
    *v = neg ? -(int64_t)x : (int64_t)x;
    return true;
}

SAM_FN uint32_t sam_base_code(uint8_t c)
{
    if (c >= 'a' && c <= 'z') c = (uint8_t)(c - 32);
    switch (c) {
    case '=': return 0; case 'A': return 1; case 'C': return 2; case 'M': return 3; case 'G': return 4; case 'R': return 5; case 'S': return 6; case 'V': return 7;
    case 'T': return 8; case 'W': return 9; case 'Y': return 10; case 'H': return 11; case 'K': return 12; case 'D': return 13; case 'B': return 14;
    }
    return 15;
}

SAM_FN int sam_reg2bin(int64_t beg, int64_t end)
{
    --end;
    if (beg >> 14 == end >> 14) return (int)(4681 + (beg >> 14));
    if (beg >> 17 == end >> 17) return (int)(585 + (beg >> 17));
    if (beg >> 20 == end >> 20) return (int)(73 + (beg >> 20));
    if (beg >> 23 == end >> 23) return (int)(9 + (beg >> 23));
    if (beg >> 26 == end >> 26) return (int)(1 + (beg >> 26));
    return 0;
}

SAM_FN void sam_put(uint8_t *o, uint64_t v, int bytes) { for (int i = 0; i < bytes; ++i) o[i] = (uint8_t)(v >> (8 * i)); }
SAM_FN bool sam_alpha(uint8_t c) { return (c >= 'A' && c <= 'Z') || (c >= 'a' && c <= 'z'); }
SAM_FN bool sam_digit(uint8_t c) { return c >= '0' && c <= '9'; }

// what the GPU plugs in: no floating-point text is read there
struct sam_no_float {
    static constexpr bool has = false;
    SAM_MEMBER bool f32(const uint8_t *, uint32_t, uint8_t *) const { return false; }
    SAM_MEMBER bool f64(const uint8_t *, uint32_t, uint8_t *) const { return false; }
};

#define SAM_FAIL(e) do { *err = (e); return SAM_ERROR; } while (0)

// s[0, n): the line without its line feed (and without the CR before it); F from sam_fields.  out: nullptr, or *size bytes as an earlier call gave them.
template <class FL>
SAM_FN int sam_record(const uint8_t *s, uint32_t n, const sam_fld &F, const sam_refs &R, uint8_t *out, uint32_t *size, int *err, uint32_t lane, uint32_t nl, const FL &fl)
{
    *err = SAM_E_NONE;
    if (n == 0) SAM_FAIL(SAM_E_EMPTY);
    if (n > SAM_MAX_LINE) SAM_FAIL(SAM_E_LONG);
    if (s[0] == '@') SAM_FAIL(SAM_E_AT);
    if (F.nf < 11) SAM_FAIL(SAM_E_FIELDS);
    uint32_t a[11], b[11];
    for (int i = 0; i < 11; ++i) {
        a[i] = F.f[i]; b[i] = i < 10 ? F.f[i + 1] - 1 : F.f[11];
        if (a[i] >= b[i]) SAM_FAIL(SAM_E_EMPTY_FIELD);
    }
    const bool w0 = out && lane == 0;
    const uint32_t qn = b[0] - a[0];
    if (qn > 254) SAM_FAIL(SAM_E_QNAME);
    uint64_t u = 0;
    int64_t iv = 0;
    if (!sam_uint(s, a[1], b[1], 65535, &u)) SAM_FAIL(SAM_E_FLAG);
    const uint32_t flag = (uint32_t)u;
    int32_t tid = -1;
    if (!(b[2] - a[2] == 1 && s[a[2]] == '*')) { tid = sam_ref_find(R, s + a[2], b[2] - a[2]); if (tid < 0) SAM_FAIL(SAM_E_RNAME); }
    if (!sam_uint(s, a[3], b[3], 0x7fffffffull, &u)) SAM_FAIL(SAM_E_POS);
    const int64_t pos = (int64_t)u - 1;
    if (!sam_uint(s, a[4], b[4], 255, &u)) SAM_FAIL(SAM_E_MAPQ);
    const uint32_t mapq = (uint32_t)u;
    // CIGAR
    const uint32_t o_cig = 36 + qn + 1;
    uint32_t n_cig = 0;
    uint64_t qlen = 0, rlen = 0;
    if (!(b[5] - a[5] == 1 && s[a[5]] == '*')) {
        uint32_t p = a[5];
        while (p < b[5]) {
            uint32_t e = p;
            while (e < b[5] && sam_digit(s[e])) ++e;
            if (e == p || e == b[5]) SAM_FAIL(SAM_E_CIGAR);
            if (!sam_uint(s, p, e, (1u << 28) - 1, &u)) SAM_FAIL(SAM_E_CIGAR_LEN);
            uint32_t op;
            switch (s[e]) {
            case 'M': op = 0; break; case 'I': op = 1; break; case 'D': op = 2; break; case 'N': op = 3; break; case 'S': op = 4; break;
            case 'H': op = 5; break; case 'P': op = 6; break; case '=': op = 7; break; case 'X': op = 8; break;
            default: SAM_FAIL(SAM_E_CIGAR);
            }
            if (n_cig == 65535) SAM_FAIL(SAM_E_CIGAR_OPS);
            if ((0x193u >> op) & 1u) qlen += u;          // M I S = X
            if ((0x18du >> op) & 1u) rlen += u;          // M D N = X
            if (w0) sam_put(out + o_cig + 4 * n_cig, u << 4 | op, 4);
            ++n_cig;
            p = e + 1;
        }
    }
    int32_t mtid = -1;
    if (b[6] - a[6] == 1 && s[a[6]] == '=') mtid = tid;
    else if (!(b[6] - a[6] == 1 && s[a[6]] == '*')) { mtid = sam_ref_find(R, s + a[6], b[6] - a[6]); if (mtid < 0) SAM_FAIL(SAM_E_RNEXT); }
    if (!sam_uint(s, a[7], b[7], 0x7fffffffull, &u)) SAM_FAIL(SAM_E_PNEXT);
    const int64_t mpos = (int64_t)u - 1;
    if (!sam_int(s, a[8], b[8], -2147483648ll, 2147483647ll, &iv)) SAM_FAIL(SAM_E_TLEN);
    const int64_t tlen = iv;
    const bool seq_star = b[9] - a[9] == 1 && s[a[9]] == '*', qual_star = b[10] - a[10] == 1 && s[a[10]] == '*';
    const uint32_t l_seq = seq_star ? 0 : b[9] - a[9];
    if (n_cig && !seq_star && qlen != l_seq) SAM_FAIL(SAM_E_CIGAR_SEQ);
    if (!qual_star) {
        if (b[10] - a[10] != l_seq) SAM_FAIL(SAM_E_QUAL_LEN);
        if (F.flags & 1u) SAM_FAIL(SAM_E_QUAL_BYTE);
    }
    const uint32_t o_seq = o_cig + 4 * n_cig, o_qual = o_seq + (l_seq + 1) / 2, o_aux = o_qual + l_seq;
    // optional fields
    uint32_t o = o_aux, p = F.f[11];
    while (p < n) {                                       // s[p] is the tab in front of the field
        const uint32_t fa = p + 1;
        uint32_t e = fa;
        while (e < n && s[e] != '\t') ++e;
        if (e - fa < 5 || s[fa + 2] != ':' || s[fa + 4] != ':' || !sam_alpha(s[fa]) || !(sam_alpha(s[fa + 1]) || sam_digit(s[fa + 1]))) SAM_FAIL(SAM_E_AUX_FORM);
        const uint8_t t = s[fa + 3];
        const uint32_t v = fa + 5, vl = e - v;
        if (w0) { out[o] = s[fa]; out[o + 1] = s[fa + 1]; }
        o += 2;
        if (t == 'A') {
            if (vl != 1 || s[v] < 33 || s[v] > 126) SAM_FAIL(SAM_E_AUX_A);
            if (w0) { out[o] = 'A'; out[o + 1] = s[v]; }
            o += 2;
        } else if (t == 'i') {
            if (!sam_int(s, v, e, -2147483648ll, 4294967295ll, &iv)) SAM_FAIL(SAM_E_AUX_I);
            const int nb = iv >= 0 ? (iv <= 255 ? 1 : iv <= 65535 ? 2 : 4) : (iv >= -128 ? 1 : iv >= -32768 ? 2 : 4);
            if (w0) { out[o] = iv >= 0 ? (nb == 1 ? 'C' : nb == 2 ? 'S' : 'I') : (nb == 1 ? 'c' : nb == 2 ? 's' : 'i'); sam_put(out + o + 1, (uint64_t)iv, nb); }
            o += 1 + nb;
        } else if (t == 'Z' || t == 'H') {
            if (t == 'H') {
                if (vl & 1u) SAM_FAIL(SAM_E_AUX_H);
                for (uint32_t i = v; i < e; ++i) { const uint8_t c = s[i]; if (!(sam_digit(c) || (c >= 'A' && c <= 'F') || (c >= 'a' && c <= 'f'))) SAM_FAIL(SAM_E_AUX_H); }
            }
            if (w0) { out[o] = t; for (uint32_t i = 0; i < vl; ++i) out[o + 1 + i] = s[v + i]; out[o + 1 + vl] = 0; }
            o += 2 + vl;
        } else if (t == 'f' || t == 'd') {
            if (!FL::has) return SAM_SLOW;
            uint8_t tmp[8];
            if (!(t == 'f' ? fl.f32(s + v, vl, tmp) : fl.f64(s + v, vl, tmp))) SAM_FAIL(SAM_E_AUX_F);
            const int nb = t == 'f' ? 4 : 8;
            if (w0) { out[o] = t; for (int i = 0; i < nb; ++i) out[o + 1 + i] = tmp[i]; }
            o += 1 + nb;
        } else if (t == 'B') {
            if (vl < 1) SAM_FAIL(SAM_E_AUX_B_SUB);
            const uint8_t sub = s[v];
            int nb; int64_t lo, hi;
            switch (sub) {
            case 'c': nb = 1; lo = -128; hi = 127; break;                 case 'C': nb = 1; lo = 0; hi = 255; break;
            case 's': nb = 2; lo = -32768; hi = 32767; break;             case 'S': nb = 2; lo = 0; hi = 65535; break;
            case 'i': nb = 4; lo = -2147483648ll; hi = 2147483647ll; break; case 'I': nb = 4; lo = 0; hi = 4294967295ll; break;
            case 'f': nb = 4; lo = hi = 0; break;
            default: SAM_FAIL(SAM_E_AUX_B_SUB);
            }
            if (sub == 'f' && !FL::has) return SAM_SLOW;
            if (w0) { out[o] = 'B'; out[o + 1] = sub; }
            const uint32_t o_cnt = o + 2;
            o += 6;
            uint32_t cnt = 0, q = v + 1;
            while (q < e) {
                if (s[q] != ',') SAM_FAIL(SAM_E_AUX_B_ELEM);
                uint32_t r = q + 1;
                while (r < e && s[r] != ',') ++r;
                if (sub == 'f') {
                    uint8_t tmp[4];
                    if (!fl.f32(s + q + 1, r - q - 1, tmp)) SAM_FAIL(SAM_E_AUX_F);
                    if (w0) for (int i = 0; i < 4; ++i) out[o + i] = tmp[i];
                } else {
                    if (!sam_int(s, q + 1, r, lo, hi, &iv)) SAM_FAIL(SAM_E_AUX_B_ELEM);
                    if (w0) sam_put(out + o, (uint64_t)iv, nb);
                }
                o += (uint32_t)nb; ++cnt;
                q = r;
            }
            if (w0) sam_put(out + o_cnt, cnt, 4);
        } else SAM_FAIL(SAM_E_AUX_TYPE);
        p = e;
    }
    *size = o;
    if (!out) return SAM_FAST;
    // the fixed bytes, by lane 0
    if (w0) {
        int bin = 4680;
        if (pos >= 0) bin = sam_reg2bin(pos, pos + (rlen && !(flag & 4u) ? (int64_t)rlen : 1)) & 0xffff;
        sam_put(out, o - 4, 4); sam_put(out + 4, (uint32_t)tid, 4); sam_put(out + 8, (uint32_t)(int32_t)pos, 4);
        out[12] = (uint8_t)(qn + 1); out[13] = (uint8_t)mapq; sam_put(out + 14, (uint32_t)bin, 2); sam_put(out + 16, n_cig, 2); sam_put(out + 18, flag, 2);
        sam_put(out + 20, l_seq, 4); sam_put(out + 24, (uint32_t)mtid, 4); sam_put(out + 28, (uint32_t)(int32_t)mpos, 4); sam_put(out + 32, (uint32_t)(int32_t)tlen, 4);
        out[36 + qn] = 0;
    }
    // the bulk, over the lanes
    for (uint32_t i = lane; i < qn; i += nl) out[36 + i] = s[a[0] + i];
    for (uint32_t j = lane; j < (l_seq + 1) / 2; j += nl) {
        const uint32_t hi4 = sam_base_code(s[a[9] + 2 * j]), lo4 = 2 * j + 1 < l_seq ? sam_base_code(s[a[9] + 2 * j + 1]) : 0u;
        out[o_seq + j] = (uint8_t)(hi4 << 4 | lo4);
    }
    for (uint32_t i = lane; i < l_seq; i += nl) out[o_qual + i] = qual_star ? (uint8_t)0xff : (uint8_t)(s[a[10] + i] - 33);
    return SAM_FAST;
}
