// merge_host.h -- the host side of the k-way merge of coordinate-sorted BAM streams (include/seqlib_amd_merge.h): the planner of the rounds and the header
// rule, both plain host functions with no GPU in them.  slx_merge.hip runs them; tests/cpp/merge_host_test.cpp runs the same planner over the host-compiled
// bodies of dev_merge.h.  DESIGN.md section 9.17 has the proof.
//
// The planner.  Every input has a window: the records read from it and not yet emitted, in file order, so their keys rise.  L_i is the last key of a non-empty
// window.  An input is "at its end" once a read of it has returned nothing.
//   refill   before a round, every input not at its end whose window is empty, and every such input whose L_i equalled the previous round's bound
//   bound    B = min L_i over the inputs not at their end; infinite when all are at their end
//   emit     exactly the held records with key < B (strictly): every record not yet read of input i has key >= L_i >= B, so the stable merge of those
//            prefixes is the next stretch of the global order.  An input at the bound is refilled every round, so a round that emits nothing has read
//            something or has brought an input to its end.
//   budget   the windows together hold at most max_bytes; a block of equal keys longer than that cannot be merged
#pragma once
#include <cstdint>
#include <string>
#include <vector>
#include "recsort_host.h"

struct merge_in {
    bool at_end = false;
    uint64_t held = 0;            // records in the window
    uint64_t last_key = 0;        // L_i; meaningful while held > 0
};

// does input `in` read its next batch before the coming round?  had_bound / prev_bound: the finite bound of the previous round, if there was one
static inline bool merge_wants_refill(const merge_in &in, bool had_bound, uint64_t prev_bound)
{
    return !in.at_end && (in.held == 0 || (had_bound && in.last_key == prev_bound));
}

// the bound of the round over the k inputs as they stand after the refills: false = infinite (every input at its end, everything held is emitted)
static inline bool merge_bound(const merge_in *in, int k, uint64_t *bound)
{
    bool any = false;
    uint64_t b = 0;
    for (int i = 0; i < k; ++i) {
        if (in[i].at_end || in[i].held == 0) continue;          // (not at its end and empty does not occur after the refills: a read gives records or the end)
        if (!any || in[i].last_key < b) b = in[i].last_key;
        any = true;
    }
    *bound = b;
    return any;
}

// the windows may hold held_bytes together?
static inline bool merge_fits(uint64_t held_bytes, int64_t max_bytes) { return max_bytes >= 0 && held_bytes <= (uint64_t)max_bytes; }

static inline int32_t merge_key_tid(uint64_t key) { return (int32_t)(uint32_t)(key >> 32); }
static inline int32_t merge_key_pos(uint64_t key) { return (int32_t)((uint32_t)key ^ 0x80000000u); }

// ------------------------------------------------------------------ the header rule
// The text of the merged file from the texts of its inputs, in add order:
//   input 0's text through recsort_header_so (the sorter's rule: the file is coordinate-sorted);
//   then from inputs 1.., in order, every @RG, @PG or @CO line that is not byte-identical to a line already present;
//   an @RG or @PG whose ID: is that of a different line of its kind already present is refused (rc 2; *what = the ID) -- samtools would rename it and edit
//   the records, and records are never edited here;  @HD, @SQ and any other line of a later input is dropped.
// rc 0 = *out is the text.
static inline std::vector<std::string> merge_lines(const std::string &text)
{
    std::vector<std::string> v;
    for (size_t p = 0; p < text.size(); ) {
        size_t q = text.find('\n', p);
        if (q == std::string::npos) q = text.size();
        v.push_back(text.substr(p, q - p));
        p = q + 1;
    }
    return v;
}
static inline std::string merge_line_id(const std::string &line)
{
    for (size_t p = line.find('\t'); p != std::string::npos; p = line.find('\t', p + 1))
        if (line.compare(p + 1, 3, "ID:") == 0) { const size_t q = line.find('\t', p + 1); return line.substr(p + 4, q == std::string::npos ? q : q - p - 4); }
    return std::string();
}
static inline int merge_header_rule(const std::vector<std::string> &texts, std::string *out, std::string *what)
{
    if (texts.empty()) { out->clear(); return 0; }
    std::string text = recsort_header_so(texts[0]);
    std::vector<std::string> have = merge_lines(text);
    for (size_t t = 1; t < texts.size(); ++t) {
        for (const std::string &ln : merge_lines(texts[t])) {
            const std::string kind = ln.substr(0, 3);
            if (ln.size() > 3 && ln[3] != '\t') continue;
            if (kind != "@RG" && kind != "@PG" && kind != "@CO") continue;
            bool present = false;
            for (const std::string &h : have) if (h == ln) { present = true; break; }
            if (present) continue;
            if (kind != "@CO") {
                const std::string id = merge_line_id(ln);
                for (const std::string &h : have)
                    if (h.compare(0, 3, kind) == 0 && merge_line_id(h) == id) { *what = kind + " ID:" + id; return 2; }
            }
            if (!text.empty() && text.back() != '\n') text.push_back('\n');
            text += ln; text.push_back('\n');
            have.push_back(ln);
        }
    }
    out->swap(text);
    return 0;
}
