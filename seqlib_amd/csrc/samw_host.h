// samw_host.h -- the host side of the SAM writer: dev_samw.h's per-record body with printf's %g plugged in (what a sam_write1 loop does, one record at a time), the
// refusals' messages and the reference-name table.  Host only, no GPU; compiled into slx_samw.hip (the slow path, slx_samw_format_record) and into
// tests/cpp/samw_host_test.cpp.  htslib is not part of this image: the text is BamWriter::format_sam's (include/seqlib_amd_samw.h lists every rule).
#pragma once
#include <stdint.h>
#include <stdio.h>
#include <string.h>
#include <string>
#include <vector>
#include "dev_samw.h"

// %g of the value's bytes, as BamWriter::format_num prints them (a float is promoted to double); returns the length
struct samwh_float {
    static constexpr bool has = true;
    int f32(const uint8_t *p, char *buf) const { float v; memcpy(&v, p, 4); return snprintf(buf, SAMW_FLOAT_MAX, "%g", v); }
    int f64(const uint8_t *p, char *buf) const { double v; memcpy(&v, p, 8); return snprintf(buf, SAMW_FLOAT_MAX, "%g", v); }
};

static inline const char *samwh_errtext(int e)
{
    switch (e) {
    case SAMW_E_SPAN: return "the record's extent is not its block_size + 4 inside the stream";
    case SAMW_E_FIELDS: return "the record's fields pass its block_size (32 + l_read_name + 4 n_cigar + (l_seq + 1) / 2 + l_seq > block_size)";
    case SAMW_E_TID: return "tid is not a reference of the header";
    case SAMW_E_MTID: return "mtid is not a reference of the header";
    case SAMW_E_QNAME: return "no NUL inside l_read_name";
    case SAMW_E_AUX_END: return "an optional field passes the record's end";
    case SAMW_E_AUX_NUL: return "a Z or H field has no NUL";
    case SAMW_E_AUX_TYPE: return "an optional field's type is none of AcCsSiIfdZHB";
    case SAMW_E_AUX_B_SUB: return "a B field's subtype is none of cCsSiIf";
    }
    return "unknown error";
}

// the name table of samw_refs, on the host
struct SamwRefTable {
    std::vector<uint8_t> names;
    std::vector<uint32_t> off;
    void build(const std::vector<std::string> &ref)
    {
        names.clear(); off.assign(1, 0);
        for (const std::string &s : ref) { names.insert(names.end(), s.begin(), s.end()); off.push_back((uint32_t)names.size()); }
        names.push_back(0);          // (never an empty array)
    }
    samw_refs view() const { return samw_refs{names.data(), off.data(), (int32_t)off.size() - 1}; }
};

// one record -> its line appended to text (line feed included).  SAMW_FAST, or SAMW_ERROR with *err and text as it was
static inline int samwh_format(const uint8_t *rec, uint64_t n, const samw_refs &R, std::vector<uint8_t> &text, int *err)
{
    samw_fld F;
    memset(&F, 0, sizeof F);
    uint64_t size = 0, size2 = 0;
    const samwh_float fl;
    const int v = samw_line(rec, n, R, &F, (uint8_t *)nullptr, &size, err, 0u, 1u, lanes_one(), fl, SAMW_NO_DEFER);
    if (v != SAMW_FAST) return v;
    const size_t at = text.size();
    text.resize(at + size);
    (void)samw_line(rec, n, R, &F, text.data() + at, &size2, err, 0u, 1u, lanes_one(), fl, SAMW_NO_DEFER);
    samw_bulk(rec, F, text.data() + at, 0, 1);
    return SAMW_FAST;
}
