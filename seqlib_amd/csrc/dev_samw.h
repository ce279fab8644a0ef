// dev_samw.h -- one block_size-prefixed BAM record -> one SAM line (the rules are listed in include/seqlib_amd_samw.h; the definition is BamWriter::format_sam of
// include/SeqLib/BamWriter.h).  The per-record body compiles for the GPU (k_samw_size, k_samw_fill of slx_samw.hip) and for the host (samw_host.h,
// tests/cpp/samw_host_test.cpp): there is ONE statement of the grammar in C, and the host formatter is this body with printf's %g plugged in.
//   samw_line   `lane` of `nl` lanes call it with the same arguments.  out == nullptr: every refusal rule, the line's length and the field table F (text offsets of
//               CIGAR, SEQ, QUAL and the optional fields).  out != nullptr: the line, from F: the short fields by lane 0, QNAME, Z / H strings, CIGAR ops and B elements
//               over the lanes (their places from the lanes' scan, nl at a time).  WV carries what the lanes share: the kernel plugs in the wave's cross-lane
//               operations (dev_lanes.h: lanes_group<64>, all 64 lanes call together), the host and a single lane of the size kernel lanes_one (lane 0 of 1).
//   samw_bulk   SEQ (two bases per packed byte) and QUAL + 33 of a sized record, over any number of lanes: a long record takes several waves for it.
// Verdicts: SAMW_FAST the line is decided here; SAMW_SLOW the record carries an f, d or B:f field and FL cannot print floating-point text (the GPU); SAMW_ERROR with
// *err; SAMW_DEFER (sizing only) the record has more than `defer` CIGAR ops or B elements: the caller sizes it again with more lanes.
// Nothing outside r[0, n) is read, and out is written only for a record that an out == nullptr call has taken.
#pragma once
#include <stdint.h>
#include "dev_lanes.h"
#if defined(__HIPCC__)
#define SAMW_FN __host__ __device__ __forceinline__
#else
#define SAMW_FN static inline
#endif

enum { SAMW_FAST = 0, SAMW_SLOW = 1, SAMW_ERROR = 2, SAMW_DEFER = 3 };
enum { SAMW_E_NONE = 0, SAMW_E_SPAN, SAMW_E_FIELDS, SAMW_E_TID, SAMW_E_MTID, SAMW_E_QNAME, SAMW_E_AUX_END, SAMW_E_AUX_NUL, SAMW_E_AUX_TYPE, SAMW_E_AUX_B_SUB, SAMW_E_COUNT };
#define SAMW_NO_DEFER 0xffffffffu
#define SAMW_FLOAT_MAX 32          // bytes a %g text takes at most, NUL included

// the header's reference names in tid order
struct samw_refs {
    const uint8_t *names;          // one behind the other
    const uint32_t *off;           // n + 1 offsets into names
    int32_t n;
};

struct samw_fld {
    uint64_t t_cig, t_seq, t_qual, t_aux;          // text offsets: first byte of CIGAR, of SEQ, of QUAL, and of the tab in front of the first optional field (or the line feed)
    uint32_t b_seq, b_aux;                         // record offsets: the packed sequence, the first optional field
    uint32_t qn, l_seq;                            // QNAME's printed length; l_seq
};

// what the GPU plugs in: no floating-point text is printed there
struct samw_no_float {
    static constexpr bool has = false;
    LANES_MEMBER int f32(const uint8_t *, char *) const { return 0; }
    LANES_MEMBER int f64(const uint8_t *, char *) const { return 0; }
};

SAMW_FN uint32_t samw_le16(const uint8_t *p) { return (uint32_t)p[0] | (uint32_t)p[1] << 8; }
SAMW_FN uint32_t samw_le32(const uint8_t *p) { return (uint32_t)p[0] | (uint32_t)p[1] << 8 | (uint32_t)p[2] << 16 | (uint32_t)p[3] << 24; }
// decimal digits of v, by comparison
SAMW_FN uint32_t samw_w32(uint32_t v)
{
    return v < 10u ? 1 : v < 100u ? 2 : v < 1000u ? 3 : v < 10000u ? 4 : v < 100000u ? 5 : v < 1000000u ? 6 : v < 10000000u ? 7 : v < 100000000u ? 8 : v < 1000000000u ? 9 : 10;
}
// ... of a signed value whose magnitude fits 32 bits (every number of a BAM record plus one)
SAMW_FN uint32_t samw_wi(int64_t v) { return v < 0 ? 1 + samw_w32((uint32_t)(-v)) : samw_w32((uint32_t)v); }
SAMW_FN uint32_t samw_put_i(uint8_t *o, int64_t v)
{
    const uint32_t w = samw_wi(v);
    uint32_t m = (uint32_t)(v < 0 ? -v : v);
    if (v < 0) o[0] = '-';
    for (uint32_t i = w; i-- > (v < 0 ? 1u : 0u);) { o[i] = (uint8_t)('0' + m % 10u); m /= 10u; }
    return w;
}
// bytes of an integer optional field's value, 0 for another type; its value
SAMW_FN uint32_t samw_int_bytes(uint8_t t) { return t == 'c' || t == 'C' ? 1 : t == 's' || t == 'S' ? 2 : t == 'i' || t == 'I' ? 4 : 0; }
SAMW_FN int64_t samw_int_value(uint8_t t, const uint8_t *p)
{
    switch (t) {
    case 'c': return (int8_t)p[0];
    case 'C': return p[0];
    case 's': return (int16_t)samw_le16(p);
    case 'S': return samw_le16(p);
    case 'i': return (int32_t)samw_le32(p);
    }
    return samw_le32(p);
}

#define SAMW_FAIL(e) do { *err = (e); return SAMW_ERROR; } while (0)

// r[0, n): the record with its block_size, n its extent in the stream.  F: written when out == nullptr, read otherwise.  *size: the line's bytes, line feed included.
template <class WV, class FL>
SAMW_FN int samw_line(const uint8_t *r, uint64_t n, const samw_refs &R, samw_fld *F, uint8_t *out, uint64_t *size, int *err, uint32_t lane, uint32_t nl, const WV &wv, const FL &fl,
                      uint32_t defer)
{
    *err = SAMW_E_NONE; *size = 0;
    if (n < 36 || (uint64_t)samw_le32(r) + 4 != n) SAMW_FAIL(SAMW_E_SPAN);
    const int32_t tid = (int32_t)samw_le32(r + 4), mtid = (int32_t)samw_le32(r + 24);
    const int64_t pos1 = (int64_t)(int32_t)samw_le32(r + 8) + 1, mpos1 = (int64_t)(int32_t)samw_le32(r + 28) + 1, tlen = (int32_t)samw_le32(r + 32);
    const uint32_t l_name = r[12], mapq = r[13], n_cig = samw_le16(r + 16), flag = samw_le16(r + 18), l_seq = samw_le32(r + 20);
    const uint64_t o_cig = 36 + (uint64_t)l_name, o_seq = o_cig + 4 * (uint64_t)n_cig, o_qual = o_seq + ((uint64_t)l_seq + 1) / 2, o_aux = o_qual + l_seq;
    if (l_seq > 0x7fffffffu || o_aux > n) SAMW_FAIL(SAMW_E_FIELDS);
    if (tid >= R.n) SAMW_FAIL(SAMW_E_TID);
    if (mtid >= R.n) SAMW_FAIL(SAMW_E_MTID);
    const bool w0 = out && lane == 0;
    uint32_t qn;
    if (!out) {
        qn = 0;
        while (qn < l_name && r[36 + qn]) ++qn;
        if (qn == l_name) SAMW_FAIL(SAMW_E_QNAME);
        if (n_cig > defer) return SAMW_DEFER;
    } else qn = F->qn;
    const uint32_t w_rname = tid < 0 ? 1 : R.off[tid + 1] - R.off[tid], w_rnext = mtid < 0 || mtid == tid ? 1 : R.off[mtid + 1] - R.off[mtid];
    uint64_t t;          // the text offset the walk has reached
    if (!out) {
        t = (uint64_t)qn + 1 + samw_w32(flag) + 1 + w_rname + 1 + samw_wi(pos1) + 1 + samw_w32(mapq) + 1;
        F->t_cig = t;
        uint64_t cw = 0;
        for (uint32_t i = lane; i < n_cig; i += nl) cw += samw_w32(samw_le32(r + o_cig + 4 * (uint64_t)i) >> 4) + 1;
        t += n_cig ? wv.sum(cw) : 1;
        t += 1 + w_rnext + 1 + samw_wi(mpos1) + 1 + samw_wi(tlen) + 1;
        F->t_seq = t;
        t += (l_seq ? l_seq : 1) + 1;
        F->t_qual = t;
        t += l_seq && r[o_qual] != 0xff ? l_seq : 1;
        F->t_aux = t;
        F->b_seq = (uint32_t)o_seq; F->b_aux = (uint32_t)o_aux; F->qn = qn; F->l_seq = l_seq;
    } else {
        for (uint32_t i = lane; i < qn; i += nl) out[i] = r[36 + i];
        if (w0) {
            uint8_t *o = out + qn;
            *o++ = '\t'; o += samw_put_i(o, flag); *o++ = '\t';
            if (tid < 0) *o++ = '*'; else for (uint32_t i = 0; i < w_rname; ++i) *o++ = R.names[R.off[tid] + i];
            *o++ = '\t'; o += samw_put_i(o, pos1); *o++ = '\t'; o += samw_put_i(o, mapq); *o++ = '\t';
            if (!n_cig) *o = '*';
        }
        uint64_t c = F->t_cig;
        for (uint32_t base = 0; base < n_cig; base += nl) {          // (every lane takes every turn: the scan is the lanes' together)
            const uint32_t i = base + lane;
            const uint32_t word = i < n_cig ? samw_le32(r + o_cig + 4 * (uint64_t)i) : 0;
            const uint32_t w = i < n_cig ? samw_w32(word >> 4) + 1 : 0;
            uint32_t total;
            const uint32_t ex = wv.scan(w, &total);
            if (i < n_cig) { samw_put_i(out + c + ex, word >> 4); out[c + ex + w - 1] = (uint8_t)"MIDNSHP=XB??????"[word & 15u]; }
            c += total;
        }
        if (w0) {
            uint8_t *o = out + F->t_seq - (1 + w_rnext + 1 + samw_wi(mpos1) + 1 + samw_wi(tlen) + 1);
            *o++ = '\t';
            if (mtid < 0) *o++ = '*'; else if (mtid == tid) *o++ = '='; else for (uint32_t i = 0; i < w_rnext; ++i) *o++ = R.names[R.off[mtid] + i];
            *o++ = '\t'; o += samw_put_i(o, mpos1); *o++ = '\t'; o += samw_put_i(o, tlen); *o++ = '\t';
            out[F->t_qual - 1] = '\t';
        }
        t = F->t_aux;
    }
    // optional fields: "\tTG:t:value"
    bool slow = false;
    uint64_t p = o_aux;
    while (n - p >= 4) {
        const uint8_t ty = r[p + 2];
        if (w0) { out[t] = '\t'; out[t + 1] = r[p]; out[t + 2] = r[p + 1]; out[t + 3] = ':'; out[t + 5] = ':'; }
        p += 3;
        const uint32_t ib = samw_int_bytes(ty);
        if (ty == 'A') {
            if (w0) { out[t + 4] = 'A'; out[t + 6] = r[p]; }
            p += 1; t += 7;
        } else if (ib) {
            if (n - p < ib) SAMW_FAIL(SAMW_E_AUX_END);
            const int64_t v = samw_int_value(ty, r + p);
            if (w0) { out[t + 4] = 'i'; samw_put_i(out + t + 6, v); }
            p += ib; t += 6 + samw_wi(v);
        } else if (ty == 'f' || ty == 'd') {
            const uint32_t nb = ty == 'f' ? 4 : 8;
            if (n - p < nb) SAMW_FAIL(SAMW_E_AUX_END);
            if (!FL::has) slow = true;
            else {
                char buf[SAMW_FLOAT_MAX];
                const int len = ty == 'f' ? fl.f32(r + p, buf) : fl.f64(r + p, buf);
                if (w0) { out[t + 4] = ty; for (int i = 0; i < len; ++i) out[t + 6 + i] = (uint8_t)buf[i]; }
                t += 6 + (uint64_t)len;
            }
            p += nb;
        } else if (ty == 'Z' || ty == 'H') {
            uint64_t e = n;
            for (uint64_t i = p + lane; i < n; i += nl) if (!r[i]) { e = i; break; }
            e = wv.min(e);
            if (e == n) SAMW_FAIL(SAMW_E_AUX_NUL);
            if (w0) out[t + 4] = ty;
            if (out) for (uint64_t i = p + lane; i < e; i += nl) out[t + 6 + (i - p)] = r[i];
            t += 6 + (e - p); p = e + 1;
        } else if (ty == 'B') {
            if (n - p < 5) SAMW_FAIL(SAMW_E_AUX_END);
            const uint8_t sub = r[p];
            const uint32_t cnt = samw_le32(r + p + 1), es = sub == 'f' ? 4 : samw_int_bytes(sub);
            if (!es) SAMW_FAIL(SAMW_E_AUX_B_SUB);
            if ((uint64_t)cnt * es > n - p - 5) SAMW_FAIL(SAMW_E_AUX_END);
            if (!out && cnt > defer) return SAMW_DEFER;
            if (w0) { out[t + 4] = 'B'; out[t + 6] = sub; }
            p += 5; t += 7;
            if (sub == 'f') {
                if (!FL::has) slow = true;
                else
                    for (uint32_t i = 0; i < cnt; ++i) {
                        char buf[SAMW_FLOAT_MAX];
                        const int len = fl.f32(r + p + 4 * (uint64_t)i, buf);
                        if (w0) { out[t] = ','; for (int j = 0; j < len; ++j) out[t + 1 + j] = (uint8_t)buf[j]; }
                        t += 1 + (uint64_t)len;
                    }
            } else if (!out) {
                uint64_t bw = 0;
                for (uint32_t i = lane; i < cnt; i += nl) bw += 1 + samw_wi(samw_int_value(sub, r + p + (uint64_t)i * es));
                t += wv.sum(bw);
            } else {
                for (uint32_t base = 0; base < cnt; base += nl) {
                    const uint32_t i = base + lane;
                    const int64_t v = i < cnt ? samw_int_value(sub, r + p + (uint64_t)i * es) : 0;
                    const uint32_t w = i < cnt ? 1 + samw_wi(v) : 0;
                    uint32_t total;
                    const uint32_t ex = wv.scan(w, &total);
                    if (i < cnt) { out[t + ex] = ','; samw_put_i(out + t + ex + 1, v); }
                    t += total;
                }
            }
            p += (uint64_t)cnt * es;
        } else SAMW_FAIL(SAMW_E_AUX_TYPE);
    }
    if (slow) return SAMW_SLOW;
    if (w0) out[t] = '\n';
    *size = t + 1;
    return SAMW_FAST;
}

// SEQ and QUAL of a record that samw_line has sized, lane of nl (any number of lanes: all the waves that share the record)
SAMW_FN void samw_bulk(const uint8_t *r, const samw_fld &F, uint8_t *out, uint64_t lane, uint64_t nl)
{
    const uint64_t l_seq = F.l_seq;
    if (!l_seq) { if (lane == 0) { out[F.t_seq] = '*'; out[F.t_qual] = '*'; } return; }
    const uint8_t *s = r + F.b_seq, *q = s + (l_seq + 1) / 2;
    for (uint64_t i = lane; i < l_seq; i += nl) out[F.t_seq + i] = (uint8_t)"=ACMGRSVTWYHKDBN"[(s[i >> 1] >> ((~i & 1u) << 2)) & 15u];
    if (q[0] == 0xff) { if (lane == 0) out[F.t_qual] = '*'; }
    else for (uint64_t i = lane; i < l_seq; i += nl) out[F.t_qual + i] = (uint8_t)(q[i] + 33);
}
