// sam_host.h -- the host side of the SAM reader: the serial parser (dev_sam.h's per-line body with strtod plugged in: what a sam_read1 loop does, one line at a
// time), its messages, the header (@SQ lines -> references), the reference-name table, and the sniffing of a file's first bytes.  Host only, no GPU; compiled into
// slx_sam.hip (the slow path, slx_sam_parse_line, slx_sam_sniff) and into tests/cpp/sam_host_test.cpp.  htslib is not part of this image: the grammar is restated
// from SAMv1 (include/seqlib_amd_sam.h lists every rule and the deviations).
#pragma once
#include <stdint.h>
#include <stdlib.h>
#include <string.h>
#include <algorithm>
#include <string>
#include <vector>
#include "dev_sam.h"

// [-+]?(digits[.digits*] | .digits)([eE][-+]?digits)? : what both strtod in the C locale and the Python restatement read alike
static inline bool samh_float_text(const uint8_t *p, uint32_t n)
{
    uint32_t i = 0, d = 0;
    if (i < n && (p[i] == '-' || p[i] == '+')) ++i;
    while (i < n && p[i] >= '0' && p[i] <= '9') { ++i; ++d; }
    if (i < n && p[i] == '.') {
        ++i;
        uint32_t f = 0;
        while (i < n && p[i] >= '0' && p[i] <= '9') { ++i; ++f; }
        if (!d && !f) return false;
    } else if (!d) return false;
    if (i < n && (p[i] == 'e' || p[i] == 'E')) {
        ++i;
        if (i < n && (p[i] == '-' || p[i] == '+')) ++i;
        uint32_t x = 0;
        while (i < n && p[i] >= '0' && p[i] <= '9') { ++i; ++x; }
        if (!x) return false;
    }
    return i == n;
}

struct samh_float {
    static constexpr bool has = true;
    static bool text(const uint8_t *p, uint32_t n, double *v)
    {
        if (!samh_float_text(p, n)) return false;
        const std::string t((const char *)p, n);
        *v = strtod(t.c_str(), nullptr);
        return true;
    }
    bool f32(const uint8_t *p, uint32_t n, uint8_t *out) const { double v; if (!text(p, n, &v)) return false; const float f = (float)v; memcpy(out, &f, 4); return true; }
    bool f64(const uint8_t *p, uint32_t n, uint8_t *out) const { double v; if (!text(p, n, &v)) return false; memcpy(out, &v, 8); return true; }
};

static inline const char *samh_errtext(int e)
{
    switch (e) {
    case SAM_E_EMPTY: return "empty line";
    case SAM_E_AT: return "header line ('@') after the first record";
    case SAM_E_FIELDS: return "fewer than 11 tab-separated fields";
    case SAM_E_EMPTY_FIELD: return "an empty mandatory field";
    case SAM_E_QNAME: return "QNAME is longer than 254 bytes";
    case SAM_E_FLAG: return "FLAG is not a decimal number in [0, 65535]";
    case SAM_E_RNAME: return "RNAME is neither '*' nor a reference of the header";
    case SAM_E_POS: return "POS is not a decimal number in [0, 2^31 - 1]";
    case SAM_E_MAPQ: return "MAPQ is not a decimal number in [0, 255]";
    case SAM_E_CIGAR: return "CIGAR is neither '*' nor a list of <length><op> over MIDNSHP=X";
    case SAM_E_CIGAR_LEN: return "a CIGAR op is longer than 2^28 - 1";
    case SAM_E_CIGAR_OPS: return "more than 65535 CIGAR ops: the CG:B form is not written";
    case SAM_E_RNEXT: return "RNEXT is none of '=', '*' and a reference of the header";
    case SAM_E_PNEXT: return "PNEXT is not a decimal number in [0, 2^31 - 1]";
    case SAM_E_TLEN: return "TLEN is not a signed decimal number that fits int32";
    case SAM_E_CIGAR_SEQ: return "the CIGAR's query length is not the length of SEQ";
    case SAM_E_QUAL_LEN: return "QUAL is neither '*' nor as long as SEQ";
    case SAM_E_QUAL_BYTE: return "a QUAL byte lies outside [33, 126]";
    case SAM_E_AUX_FORM: return "an optional field is not TAG:TYPE:VALUE with TAG [A-Za-z][A-Za-z0-9]";
    case SAM_E_AUX_A: return "an A field is not one printable byte";
    case SAM_E_AUX_I: return "an i field is not [-+]?digits in [-2^31, 2^32 - 1]";
    case SAM_E_AUX_H: return "an H field is not an even number of hex digits";
    case SAM_E_AUX_F: return "an f, d or B:f value is not a decimal floating-point number";
    case SAM_E_AUX_B_SUB: return "a B field has no subtype from cCsSiIf";
    case SAM_E_AUX_B_ELEM: return "a B field's element is missing, not a number, or outside the subtype's range";
    case SAM_E_AUX_TYPE: return "an optional field's type is none of AiZHBfd";
    case SAM_E_CR: return "the input ends in a CR without a line feed";
    case SAM_E_LONG: return "the line is longer than 2^30 bytes";
    }
    return "unknown error";
}

// the sorted name table of sam_refs, on the host
struct SamRefTable {
    std::vector<uint8_t> names;
    std::vector<uint32_t> off;
    std::vector<int32_t> tid;
    void build(const std::vector<std::string> &ref)
    {
        std::vector<int32_t> ord(ref.size());
        for (size_t i = 0; i < ref.size(); ++i) ord[i] = (int32_t)i;
        auto less = [&](int32_t x, int32_t y) {          // bytes as unsigned, a shorter name before its extensions: sam_ref_find's order
            const std::string &p = ref[x], &q = ref[y];
            const size_t m = std::min(p.size(), q.size());
            const int c = m ? memcmp(p.data(), q.data(), m) : 0;
            return c ? c < 0 : p.size() < q.size();
        };
        std::stable_sort(ord.begin(), ord.end(), less);
        names.clear(); tid.clear(); off.assign(1, 0);
        for (size_t i = 0; i < ord.size(); ++i) {
            if (i && ref[ord[i]] == ref[ord[i - 1]]) continue;          // (the first line that carries a name keeps it)
            names.insert(names.end(), ref[ord[i]].begin(), ref[ord[i]].end());
            off.push_back((uint32_t)names.size()); tid.push_back(ord[i]);
        }
        names.push_back(0);          // (never an empty array)
    }
    sam_refs view() const { return sam_refs{names.data(), off.data(), tid.data(), (int32_t)tid.size()}; }
};

// one line (no line feed; one trailing CR is dropped) -> rec.  SAM_FAST, or SAM_ERROR with *err
static inline int samh_parse_line(const uint8_t *line, uint64_t n, const sam_refs &R, std::vector<uint8_t> &rec, int *err)
{
    rec.clear();
    if (n && line[n - 1] == '\r') --n;
    if (n > SAM_MAX_LINE) { *err = SAM_E_LONG; return SAM_ERROR; }
    sam_fld F;
    sam_fields(line, (uint32_t)n, &F);
    uint32_t size = 0;
    const samh_float fl;
    int v = sam_record(line, (uint32_t)n, F, R, (uint8_t *)nullptr, &size, err, 0u, 1u, fl);
    if (v != SAM_FAST) return v;
    rec.resize(size);
    return sam_record(line, (uint32_t)n, F, R, rec.data(), &size, err, 0u, 1u, fl);
}

// The leading '@' lines of data[0, n).  Returns 1 when the header is complete (a line that is not an '@' line begins at *body, or at_eof and the input is used up),
// 0 when more bytes are needed, -1 with msg for an @SQ line without SN or LN.  text = the lines with LF ends, a CR before the LF dropped.
static inline int samh_header(const uint8_t *data, uint64_t n, bool at_eof, std::string &text, std::vector<std::string> &names, std::vector<int64_t> &lens, uint64_t *body,
                              uint64_t *n_lines, std::string &msg)
{
    text.clear(); names.clear(); lens.clear();
    uint64_t p = 0, lines = 0;
    for (;;) {
        if (p >= n) { if (!at_eof) return 0; break; }
        if (data[p] != '@') break;
        const uint8_t *nl = (const uint8_t *)memchr(data + p, '\n', n - p);
        if (!nl && !at_eof) return 0;
        uint64_t e = nl ? (uint64_t)(nl - data) : n;
        const uint64_t next = nl ? e + 1 : n;
        if (nl && e > p && data[e - 1] == '\r') --e;
        const std::string ln((const char *)data + p, e - p);
        text += ln; text += '\n';
        ++lines;
        if (ln == "@SQ" || ln.compare(0, 4, "@SQ\t") == 0) {
            std::string sn, lnv;
            bool has_sn = false, has_ln = false;
            size_t a = 4;
            while (a <= ln.size()) {
                size_t b = ln.find('\t', a);
                if (b == std::string::npos) b = ln.size();
                if (b - a >= 3 && ln[a + 2] == ':') {
                    if (!has_sn && ln.compare(a, 3, "SN:") == 0) { sn = ln.substr(a + 3, b - a - 3); has_sn = true; }
                    if (!has_ln && ln.compare(a, 3, "LN:") == 0) { lnv = ln.substr(a + 3, b - a - 3); has_ln = true; }
                }
                a = b + 1;
            }
            uint64_t L = 0;
            if (!has_sn || !has_ln || sn.empty() || !sam_uint((const uint8_t *)lnv.data(), 0, (uint32_t)lnv.size(), 0x7fffffffull, &L)) {
                msg = "line " + std::to_string(lines) + ": an @SQ line without SN or without a decimal LN";
                return -1;
            }
            names.push_back(sn); lens.push_back((int64_t)L);
        }
        p = next;
    }
    *body = p; *n_lines = lines;
    return 1;
}
