// dev_ref.h -- the bodies of the reference genome unit (include/seqlib_amd_ref.h has the rules; slx_ref.hip launches the kernels).  Host-compilable like
// dev_stats.h: ref_host.h runs the same bodies line by line and record by record, and tests/cpp/ref_host_test.cpp holds them against the Python statement of
// the rules (tests/ref_util.py) under ASan + UBSan before they run on a GPU.
//   rg_line_of      one line of FASTA text: its class, its bases, its width, whether a byte of it is no base
//   rg_check_line   a sequence line against its contig's first line
//   rg_nt16         the nt16 code of a reference byte
//   rg_eligible     whether a record gets an NM and an MD at all
//   rg_nm_md        the CIGAR walk of one record, base by base, into a sink that counts or writes the MD bytes
// Memory safety: a line is read inside [a, min(b, n)); a record through rf_fixed (dev_rfilter.h), its read bases below l_seq, the contig below its length.
#pragma once
#include <stdint.h>
#include <string.h>
#include "dev_rfilter.h"

#define RG_BLANK  0u
#define RG_HEADER 1u
#define RG_SEQ    2u
// what a sequence line can do wrong; the smallest (line << 3 | code) of a window is its first error
#define RG_E_BYTE        1u          // a space, a tab or another byte outside 33..126 inside a sequence line
#define RG_E_RAGGED      2u          // not the contig's last sequence line and not of its first line's bases and width, or the last one and longer
#define RG_E_AFTER_BLANK 3u          // a sequence line directly behind a blank line
#define RG_MAX_CONTIG 0x7fffffffll

struct rg_line { uint32_t cls, nb, width, bad, name_len, pad; };

// The line text[a, b): b is the start of the next line, or n + 1 behind a last line without a line feed.  nb: the bytes in front of the terminator (LF, or CR LF;
// a CR at the very end of an unterminated last line counts as one too); width: all of them.  A line of no such bytes is blank, one that starts with '>' a header
// (name_len: the bytes behind '>' up to the first space or tab), every other one a sequence line.
RF_HD void rg_line_of(const uint8_t *text, uint64_t n, uint64_t a, uint64_t b, rg_line *o)
{
    const uint64_t e = b < n ? b : n;
    uint64_t end = e;
    if (end > a && text[end - 1] == '\n') --end;
    if (end > a && text[end - 1] == '\r') --end;
    const uint64_t nb = end - a, w = e - a;
    o->width = w > 0xffffffffull ? 0xffffffffu : (uint32_t)w;
    o->nb = nb > 0xffffffffull ? 0xffffffffu : (uint32_t)nb;
    o->bad = w > 0xffffffffull ? 1u : 0u; o->name_len = 0; o->pad = 0;
    if (nb == 0) { o->cls = RG_BLANK; return; }
    if (text[a] == '>') {
        uint64_t k = a + 1;
        while (k < end && text[k] != ' ' && text[k] != '\t') ++k;
        o->cls = RG_HEADER; o->name_len = (uint32_t)(k - a - 1);
        return;
    }
    o->cls = RG_SEQ;
    for (uint64_t k = a; k < end; ++k) if (text[k] < 33 || text[k] > 126) { o->bad = 1; break; }
}

// 0 or the RG_E_* of a sequence line of nb bases and width w in a contig whose first sequence line has lb and lw; is_last: the next line is no sequence line
RF_HD uint32_t rg_check_line(uint32_t nb, uint32_t w, uint32_t bad, uint32_t lb, uint32_t lw, bool is_last, bool prev_blank)
{
    if (prev_blank) return RG_E_AFTER_BLANK;
    if (bad) return RG_E_BYTE;
    if (is_last ? nb > lb : (nb != lb || w != lw)) return RG_E_RAGGED;
    return 0;
}

RF_HD uint8_t rg_upper(uint8_t c) { return c >= 'a' && c <= 'z' ? (uint8_t)(c - 32) : c; }
// "=ACMGRSVTWYHKDBN": the 15 IUPAC letters take their places in it, in either case; every other byte ('=' and U too) is 15
RF_HD uint32_t rg_nt16(uint8_t c)
{
    c = rg_upper(c);
    if (c < 'A' || c > 'Z') return 15u;
    const uint32_t k = (uint32_t)(c - 'A');
    return (uint32_t)((k < 16 ? 0xFFF3FCFFB4FFD2E1ull >> (4 * k) : 0xFAF97F865Full >> (4 * (k - 16))) & 15u);
}
RF_HD uint32_t rg_read_code(const uint8_t *seq, uint64_t y) { return (uint32_t)(seq[y >> 1] >> ((~y & 1u) << 2)) & 15u; }
RF_HD bool rg_match(uint32_t c1, uint32_t c2) { return (c1 == c2 && c1 != 15u) || c1 == 0u; }
RF_HD uint32_t rg_digits(uint32_t u) { uint32_t d = 1; while (u >= 10u) { u /= 10u; ++d; } return d; }

// the contig a record is walked against: -1 when it gets no NM and no MD (flag 0x4, tid out of range or mapped to -1, pos < 0, no CIGAR, no bases)
RF_HD int32_t rg_eligible(const rf_feat *F, const int32_t *tid_map, int64_t n_map)
{
    if ((F->flag & 4u) || F->tid < 0 || F->tid >= n_map || F->pos < 0 || F->n_cig == 0 || F->l_seq == 0) return -1;
    return tid_map ? tid_map[F->tid] : F->tid;
}

#if defined(__HIPCC__)
#define RG_M __host__ __device__
#else
#define RG_M
#endif
struct rg_md_count { uint64_t n; RG_M void put(uint8_t) { ++n; } };
struct rg_md_write { uint8_t *p; uint64_t n; RG_M void put(uint8_t c) { p[n++] = c; } };

template <class Sink> RF_HD void rg_put_u(Sink &S, uint32_t u)
{
    uint8_t d[10];
    uint32_t k = 0;
    do { d[k++] = (uint8_t)('0' + u % 10u); u /= 10u; } while (u);
    while (k) S.put(d[--k]);
}

// The walk of seqlib_amd_ref.h over the contig ref[0, rlen); returns NM.  It stops where the reference position passes the contig's end and -- where the rules
// are silent -- where an M, = or X would read a base at or behind l_seq.
template <class Sink> RF_HD int32_t rg_nm_md(const rf_feat *F, const uint8_t *ref, int64_t rlen, Sink &S)
{
    int64_t x = F->pos;
    uint64_t y = 0;
    const uint64_t ls = (uint64_t)F->l_seq;
    uint32_t u = 0, nm = 0;
    bool stop = false;
    for (uint32_t k = 0; k < F->n_cig && !stop; ++k) {
        const uint32_t wd = rf_u32(F->cig + 4ull * k), op = wd & 15u, len = wd >> 4;
        if (op == 0 || op == 7 || op == 8) {
            for (uint32_t i = 0; i < len; ++i) {
                if (x >= rlen || y >= ls) { stop = true; break; }
                const uint8_t rb = ref[x];
                if (rg_match(rg_read_code(F->seq, y), rg_nt16(rb))) ++u;
                else { rg_put_u(S, u); S.put(rg_upper(rb)); ++nm; u = 0; }
                ++x; ++y;
            }
        } else if (op == 2) {
            rg_put_u(S, u); S.put('^');
            for (uint32_t i = 0; i < len; ++i) {
                if (x >= rlen) { stop = true; break; }
                S.put(rg_upper(ref[x])); ++x; ++nm;
            }
            u = 0;
        } else if (op == 1) { nm += len; y += len; }
        else if (op == 4) y += len;
        else if (op == 3) x += len;
    }
    rg_put_u(S, u);
    return (int32_t)nm;
}
