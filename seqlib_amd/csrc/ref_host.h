// ref_host.h -- the host side of the reference genome unit (include/seqlib_amd_ref.h): the contig table, the sentences of the FASTA errors, the .fai text, and
// the rules of dev_ref.h run line by line over a text in host memory (slx_ref_fai_of_text).  Host code only; slx_ref.hip and tests/cpp/ref_host_test.cpp (under
// ASan + UBSan) go over it.
#pragma once
#include <stdint.h>
#include <stdio.h>
#include <string>
#include <unordered_map>
#include <vector>
#include "dev_ref.h"

// beside the RG_E_* of a sequence line
#define RG_E_NAME_EMPTY 4u
#define RG_E_NAME_TWICE 5u
#define RG_E_BEFORE     6u
#define RG_E_FASTQ      7u
#define RG_E_TOO_LONG   8u
#define RG_E_NONE       9u

struct rg_contig { std::string name; int64_t len = 0; uint64_t off = 0; uint32_t lb = 0, lw = 0; };

static inline const char *rg_what(uint32_t code)
{
    switch (code) {
    case RG_E_BYTE: return "a space, a tab or another byte outside 33..126 inside a sequence line";
    case RG_E_RAGGED: return "a ragged line in the middle of a contig";
    case RG_E_AFTER_BLANK: return "a sequence line behind a blank line";
    case RG_E_NAME_EMPTY: return "an empty contig name";
    case RG_E_NAME_TWICE: return "a contig name seen twice";
    case RG_E_BEFORE: return "bytes before the first '>'";
    case RG_E_FASTQ: return "a '@' record: this is FASTQ, not FASTA";
    case RG_E_TOO_LONG: return "a contig of more than 2^31 - 1 bases";
    default: return "no contig";
    }
}
static inline std::string rg_message(uint32_t code, const std::string &contig, uint64_t byte)
{
    return std::string(rg_what(code)) + " (contig '" + contig + "', byte " + std::to_string((unsigned long long)byte) + ")";
}

static inline std::string rg_fai_text(const std::vector<rg_contig> &C)
{
    std::string t;
    char buf[96];
    for (const rg_contig &c : C) {
        snprintf(buf, sizeof buf, "\t%lld\t%llu\t%u\t%u\n", (long long)c.len, (unsigned long long)c.off, c.lb, c.lw);
        t += c.name; t += buf;
    }
    return t;
}

// the names of the contigs so far; what a header line can do wrong
struct rg_names {
    std::unordered_map<std::string, int64_t> tid;
    uint32_t add(const std::string &name, int64_t id)
    {
        if (name.empty()) return RG_E_NAME_EMPTY;
        return tid.emplace(name, id).second ? 0u : RG_E_NAME_TWICE;
    }
};

// 0, or the code of the first thing wrong with the text's first byte
static inline uint32_t rg_first_byte(const uint8_t *text, uint64_t n)
{
    if (n == 0) return RG_E_NONE;
    return text[0] == '>' ? 0u : text[0] == '@' ? RG_E_FASTQ : RG_E_BEFORE;
}

// The contigs of text[0, n), the rules applied line by line in file order.  false: *msg is the sentence of the first error.
static inline bool rg_fai_of_text(const uint8_t *text, uint64_t n, std::vector<rg_contig> *out, std::string *msg)
{
    out->clear();
    uint32_t er = rg_first_byte(text, n);
    if (er) { *msg = rg_message(er, "", 0); return false; }
    rg_names names;
    bool prev_blank = false;
    uint64_t a = 0;
    rg_line cur = {}, nxt = {};
    uint64_t b = a;
    while (b < n && text[b] != '\n') ++b;
    b = b < n ? b + 1 : n + 1;
    rg_line_of(text, n, a, b, &cur);
    while (a < n) {
        // the next line, for is_last
        const uint64_t a2 = b;
        uint64_t b2 = a2;
        const bool has_next = a2 < n;
        if (has_next) {
            while (b2 < n && text[b2] != '\n') ++b2;
            b2 = b2 < n ? b2 + 1 : n + 1;
            rg_line_of(text, n, a2, b2, &nxt);
        }
        if (cur.cls == RG_HEADER) {
            rg_contig c;
            c.name.assign((const char *)text + a + 1, cur.name_len);
            c.off = a + cur.width;
            er = names.add(c.name, (int64_t)out->size());
            if (er) { *msg = rg_message(er, c.name, a); return false; }
            out->push_back(c);
        } else if (cur.cls == RG_SEQ) {
            rg_contig &c = out->back();
            if (c.lb == 0 && !prev_blank && c.len == 0) { c.lb = cur.nb; c.lw = cur.width; }
            er = rg_check_line(cur.nb, cur.width, cur.bad, c.lb, c.lw, !has_next || nxt.cls != RG_SEQ, prev_blank);
            if (er) { *msg = rg_message(er, c.name, a); return false; }
            c.len += cur.nb;
            if (c.len > RG_MAX_CONTIG) { *msg = rg_message(RG_E_TOO_LONG, c.name, c.off); return false; }
        }
        prev_blank = cur.cls == RG_BLANK;
        a = a2; b = b2; cur = nxt;
    }
    return true;
}

// One block_size-prefixed record of n bytes against contig[0, contig_len): what slx_ref_record_nm_md answers.  false: the record does not hold (SLX_EIO).  *nm = -1
// and *md_len = 0 for a record that is not eligible; at most cap bytes of MD are written, and only when all of them fit.
static inline bool rg_record_nm_md(const uint8_t *rec, uint64_t n, const uint8_t *contig, int64_t contig_len, int32_t *nm, uint8_t *md, uint64_t cap, uint64_t *md_len)
{
    *nm = -1; *md_len = 0;
    rf_feat F;
    if (!rf_fixed(rec, n, &F)) return false;
    if (rg_eligible(&F, nullptr, 0x80000000ll) < 0) return true;
    rg_md_count S = {0};
    *nm = rg_nm_md(&F, contig, contig_len, S);
    *md_len = S.n;
    if (S.n <= cap) { rg_md_write W = {md, 0}; (void)rg_nm_md(&F, contig, contig_len, W); }
    return true;
}
