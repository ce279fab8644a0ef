// dup_host.h -- the per-record body of the duplicate marker (include/seqlib_amd_dup.h): validate, classify, the unclipped 5' end, the score, the library, the
// hash of (library, name).  Compiles for host and device like win_host.h and edit_host.h: k_dup_sig and k_dup_sig_long (dev_dup.h) run it a lane or a wave per
// record, slx_dup_signature_host and slx_dup_library_of run it on the CPU (`lane` of `nlanes`; the host build runs lane 0 of 1).  The rules are the header
// comment of include/seqlib_amd_dup.h; DESIGN.md 9.15.
//
// Memory safety.  Nothing of record i is read before ed_span (dev_edit.h) has placed [off[i], off[i + 1]) inside the stream with 36 bytes at least; ed_fixed
// checks name, CIGAR, sequence and qualities against the span before any of them is read; the name's last byte is read at 36 + l_read_name - 1 < span.  The
// quality sum reads qual[0, l_seq) only: the bytes before the first and behind the last aligned word one by one, never a word that hangs over either end.  The
// aux walk compares every header (3 bytes), value, B header (8 bytes) and B payload with the record's end before it is read, and stops where that fails.
#pragma once
#include <stdint.h>
#include <string.h>
#include "dev_edit.h"
#include "dev_lanes.h"

enum { DP_IGNORED = 0, DP_FRAGMENT = 1, DP_PAIRED = 2, DP_CLASS = 3, DP_FIRST = 4, DP_SECOND = 8 };          // dp_sig.cls: the class, and 0x40 / 0x80 of a paired record
#define DP_WAVE_LEN 512u          // the default of "wave_len"
#define DP_LANE_CIGAR 64u         // more operations than this: the wave form
#define DP_MAX_LIB 65535u
#define DP_MAX_SCORE 0x7fffffffull
#define DP_HI_IGNORED (1ull << 48)          // the first word of an ignored record: above every (library, refID)
#define DP_HI_BITS 49
#define DP_NO_MATE 0xffffffffu

// the read groups of a header: open addressing, slots[i] = entry + 1 or 0; entry e's id is pool[koff[e], koff[e + 1]) and its library lib[e].  Whole words only
// (a kernel argument; dev_edit.h says why).  n == 0: no header, or one without @RG.
struct dp_libtab {
    const uint32_t *slots, *koff, *lib;
    const uint8_t *pool;
    uint32_t mask, n;
};
// what the signature step leaves of a record.  hi, lo: E(r) as two words that order as the tuple does -- hi = library << 32 | refID, lo = (upos + 2^62) << 1 |
// reverse.  hash: of (library, name), paired records only.
struct dp_sig {
    uint64_t hi, lo, hash;
    uint32_t cls, score, library, name_len;          // name_len: without the NUL
};

#if defined(__HIP_DEVICE_COMPILE__)
#define DP_SAD(w, acc) __builtin_amdgcn_sad_u8((w), 0u, (acc))
#else
#define DP_SAD(w, acc) ((acc) + ((w) & 255u) + (((w) >> 8) & 255u) + (((w) >> 16) & 255u) + ((w) >> 24))
#endif

// the sum of v over the lanes (WAVE: all 64 lanes call it together; otherwise v itself)
template <bool WAVE> ED_FN uint64_t dp_wsum(uint64_t v)
{
#if defined(__HIP_DEVICE_COMPILE__)
    if (WAVE) v = wave_sum(v);
#endif
    return v;
}

// which lanes say yes (WAVE: all 64 lanes call it together; otherwise bit 0 is the caller's own answer -- a lane that walks a record alone asks nobody)
template <bool WAVE> ED_FN uint64_t dp_ballot(bool p) { return WAVE ? ED_BALLOT(p) : (p ? 1ull : 0ull); }

#define DP_FNV_INIT 14695981039346656037ull
ED_FN uint64_t dp_fnv(uint64_t h, uint8_t c) { return (h ^ c) * 1099511628211ull; }
ED_FN uint64_t dp_mix(uint64_t h) { h ^= h >> 33; h *= 0xff51afd7ed558ccdull; h ^= h >> 33; h *= 0xc4ceb9fe1a85ec53ull; return h ^ (h >> 33); }
ED_FN uint32_t dp_hash_id(const uint8_t *p, uint32_t n)
{
    uint64_t h = DP_FNV_INIT;
    for (uint32_t i = 0; i < n; ++i) h = dp_fnv(h, p[i]);
    return (uint32_t)dp_mix(h);
}

// the library of the read group id[0, n): the header's number, or 0 when the header does not name it.  Ids are compared byte for byte, in full.
ED_FN uint32_t dp_lookup(const dp_libtab &T, const uint8_t *id, uint32_t n)
{
    if (T.n == 0 || n == 0) return 0;
    uint32_t i = dp_hash_id(id, n) & T.mask;
    for (uint32_t v; (v = T.slots[i]) != 0; i = (i + 1) & T.mask) {
        const uint32_t e = v - 1, o = T.koff[e];
        if (T.koff[e + 1] - o != n) continue;
        uint32_t k = 0;
        while (k < n && T.pool[o + k] == id[k]) ++k;
        if (k == n) return T.lib[e];
    }
    return 0;
}

// the value of the first RG field of rec[aux_at, span) when it has type Z and is not empty; false otherwise, and where the area cannot be walked that far
ED_FN bool dp_aux_rg(const uint8_t *rec, uint32_t aux_at, uint32_t span, const uint8_t **rg, uint32_t *rg_len)
{
    uint32_t at = aux_at;
    while (at < span) {
        if (span - at < 3) return false;
        const uint8_t t = rec[at + 2];
        const bool is_rg = rec[at] == 'R' && rec[at + 1] == 'G';
        uint64_t e;
        if (t == 'A' || t == 'c' || t == 'C') e = (uint64_t)at + 4;
        else if (t == 's' || t == 'S') e = (uint64_t)at + 5;
        else if (t == 'i' || t == 'I' || t == 'f') e = (uint64_t)at + 7;
        else if (t == 'd') e = (uint64_t)at + 11;
        else if (t == 'Z' || t == 'H') {
            const uint32_t z = ed_find_nul<false>(rec, at + 3, span, 0, 1);
            if (z >= span) return false;
            if (is_rg && t == 'Z') { *rg = rec + at + 3; *rg_len = z - (at + 3); return *rg_len != 0; }
            e = (uint64_t)z + 1;
        } else if (t == 'B') {
            if (span - at < 8) return false;
            const uint8_t et = rec[at + 3];
            const uint32_t es = (et == 'c' || et == 'C') ? 1u : (et == 's' || et == 'S') ? 2u : (et == 'i' || et == 'I' || et == 'f') ? 4u : 0u;
            if (!es) return false;
            e = (uint64_t)at + 8 + (uint64_t)es * ed_ld32(rec + at + 4);
        } else return false;
        if (e > span || is_rg) return false;          // (the first RG decides, whatever its type)
        at = (uint32_t)e;
    }
    return false;
}

// the CIGAR's reference length and its leading and trailing clip runs.  WAVE: every lane of a wave with the same arguments, 64 operations per ballot from both
// ends; all lanes return the same.  A CIGAR of clips only has lead == trail == their sum.
template <bool WAVE> ED_FN void dp_cigar(const uint8_t *cig, uint32_t n, int lane, int nlanes, uint64_t *ref_len, uint64_t *lead, uint64_t *trail)
{
    uint64_t r = 0, a = 0, b = 0;
    for (uint32_t k = (uint32_t)lane; k < n; k += (uint32_t)nlanes) {
        const uint32_t w = ed_ld32(cig + 4 * (uint64_t)k), op = w & 15u;
        if (op == 0 || op == 2 || op == 3 || op == 7 || op == 8) r += w >> 4;
    }
    r = dp_wsum<WAVE>(r);
    for (int64_t base = 0; base < (int64_t)n; base += nlanes) {
        const int64_t p = base + lane;
        const bool valid = p < (int64_t)n;
        const uint32_t w = valid ? ed_ld32(cig + 4 * p) : 0u, op = w & 15u;
        const uint64_t m = dp_ballot<WAVE>(valid && op != 4 && op != 5);
        const int first = m ? (int)ed_ctz64(m) : nlanes;
        a += dp_wsum<WAVE>(valid && lane < first ? (uint64_t)(w >> 4) : 0ull);
        if (m) break;
    }
    for (int64_t hi = (int64_t)n; hi > 0; hi -= nlanes) {
        const int64_t p = hi - 1 - lane;
        const bool valid = p >= 0;
        const uint32_t w = valid ? ed_ld32(cig + 4 * p) : 0u, op = w & 15u;
        const uint64_t m = dp_ballot<WAVE>(valid && op != 4 && op != 5);
        const int first = m ? (int)ed_ctz64(m) : nlanes;
        b += dp_wsum<WAVE>(valid && lane < first ? (uint64_t)(w >> 4) : 0ull);
        if (m) break;
    }
    *ref_len = r; *lead = a; *trail = b;
}

// the bytes of w with 15 <= byte <= 0xfe, the others zeroed: four at a time, no carry crosses a byte
ED_FN uint32_t dp_qual_keep(uint32_t w)
{
    const uint32_t ge = ((((w & 0x7f7f7f7fu) | 0x80808080u) - 0x0f0f0f0fu) | w) & 0x80808080u;          // byte >= 15
    const uint32_t y = ~w, nz = (((y & 0x7f7f7f7fu) + 0x7f7f7f7fu) | y) & 0x80808080u;                    // byte != 0xff
    const uint32_t k = (ge & nz) >> 7;
    return w & (k * 0xffu);
}
ED_FN uint32_t dp_qual_byte(uint8_t q) { return q >= 15 && q <= 0xfe ? q : 0u; }
ED_FN uint32_t dp_ld32a(const uint8_t *p)
{
#if defined(__HIP_DEVICE_COMPILE__)
    return *reinterpret_cast<const uint32_t *>(p);          // (aligned)
#else
    uint32_t w; memcpy(&w, p, 4); return w;
#endif
}
// the sum of the counted bytes of q[0, n): the aligned words lane, lane + nlanes, ... four bytes an instruction; lane 0 also takes the up to 3 bytes before
// the first and behind the last word.  All lanes return the wave's sum.
template <bool WAVE> ED_FN uint64_t dp_qual(const uint8_t *q, uint64_t n, int lane, int nlanes)
{
    uint64_t head = (4u - (uint32_t)((uintptr_t)q & 3u)) & 3u;
    if (head > n) head = n;
    const uint64_t nw = (n - head) >> 2, tail0 = head + (nw << 2);
    uint64_t s = 0;
    if (lane == 0) {
        for (uint64_t i = 0; i < head; ++i) s += dp_qual_byte(q[i]);
        for (uint64_t i = tail0; i < n; ++i) s += dp_qual_byte(q[i]);
    }
    const uint8_t *w = q + head;
    for (uint64_t i = (uint64_t)lane; i < nw;) {
        uint32_t acc = 0;          // 65536 words of at most 1016 each
        for (uint32_t k = 0; k < 65536u && i < nw; ++k, i += (uint64_t)nlanes) acc = DP_SAD(dp_qual_keep(dp_ld32a(w + 4 * i)), acc);
        s += acc;
    }
    return dp_wsum<WAVE>(s);
}

// the fixed part of a record of `span` bytes whose block_size fills it: false when a field passes the span or the name does not end in NUL (l_read_name 0 included)
ED_FN bool dp_head(const uint8_t *rec, uint32_t span, uint32_t *seq_at, uint32_t *aux_at)
{
    if (!ed_fixed(rec, span, seq_at, aux_at)) return false;
    const uint32_t l_name = rec[12];
    return l_name >= 1 && rec[36 + l_name - 1] == 0;
}
// whether a record with a whole head goes to the wave form
ED_FN bool dp_is_long(const uint8_t *rec, uint32_t wave_len)
{
    const uint32_t n_cig = (uint32_t)rec[16] | (uint32_t)rec[17] << 8, l_seq = ed_ld32(rec + 20);
    return n_cig > DP_LANE_CIGAR || l_seq > wave_len;
}

// The signature of a record whose head dp_head has passed.  WAVE: every lane of a wave with the same arguments; all lanes compute the same S.
template <bool WAVE> ED_FN void dp_signature(const dp_libtab &T, const uint8_t *rec, uint32_t span, uint32_t seq_at, uint32_t aux_at, int lane, int nlanes, dp_sig *S)
{
    const uint32_t l_name = rec[12], n_cig = (uint32_t)rec[16] | (uint32_t)rec[17] << 8, flag = (uint32_t)rec[18] | (uint32_t)rec[19] << 8, l_seq = ed_ld32(rec + 20);
    const int32_t refid = (int32_t)ed_ld32(rec + 4), pos = (int32_t)ed_ld32(rec + 8);
    S->hi = DP_HI_IGNORED; S->lo = 0; S->hash = 0; S->cls = DP_IGNORED; S->score = 0; S->library = 0; S->name_len = l_name - 1;
    if ((flag & (0x4u | 0x100u | 0x800u)) || refid < 0) return;
    uint64_t ref_len, lead, trail;
    dp_cigar<WAVE>(rec + 36 + l_name, n_cig, lane, nlanes, &ref_len, &lead, &trail);
    const uint32_t rev = (flag & 0x10u) ? 1u : 0u;
    const int64_t upos = rev ? (int64_t)pos + (int64_t)ref_len - 1 + (int64_t)trail : (int64_t)pos - (int64_t)lead;          // (an empty CIGAR on the reverse strand: pos - 1)
    const uint64_t q = dp_qual<WAVE>(rec + seq_at + ((l_seq + 1) >> 1), l_seq, lane, nlanes);
    const uint8_t *rg = nullptr;
    uint32_t rg_len = 0;
    const uint32_t lib = dp_aux_rg(rec, aux_at, span, &rg, &rg_len) ? dp_lookup(T, rg, rg_len) : 0u;
    const bool paired = (flag & 0x1u) && !(flag & 0x8u);
    S->library = lib;
    S->hi = (uint64_t)lib << 32 | (uint32_t)refid;
    S->lo = ((uint64_t)(upos + (1ll << 62)) << 1) | rev;
    S->score = (uint32_t)(q > DP_MAX_SCORE ? DP_MAX_SCORE : q);
    S->cls = paired ? (uint32_t)DP_PAIRED | ((flag & 0x40u) ? DP_FIRST : 0u) | ((flag & 0x80u) ? DP_SECOND : 0u) : (uint32_t)DP_FRAGMENT;
    if (paired) {
        uint64_t h = dp_fnv(dp_fnv(DP_FNV_INIT, (uint8_t)lib), (uint8_t)(lib >> 8));
        for (uint32_t i = 0; i + 1 < l_name; ++i) h = dp_fnv(h, rec[36 + i]);
        S->hash = dp_mix(h);
    }
}

// ------------------------------------------------------------------ host only
#include <string>
#include <unordered_map>
#include <vector>
// The read groups of a header text, on the host.  The text ends at l_text or at its first NUL.  Lines are cut at '\n', fields at '\t'.  An @RG line takes part
// when it has an ID field that is not empty and that no earlier line has named; its library is the number of its first LB field's value -- distinct values are
// numbered from 1 by first appearance -- or, without LB, the next number for itself.  False: more than DP_MAX_LIB libraries.
struct dp_header {
    std::vector<std::string> ids;
    std::vector<uint32_t> lib, slots, koff;
    std::vector<uint8_t> pool;
    uint32_t n_lib = 0;
    dp_libtab view() const { return dp_libtab{slots.data(), koff.data(), lib.data(), pool.data(), slots.empty() ? 0u : (uint32_t)slots.size() - 1u, (uint32_t)ids.size()}; }
    void clear() { ids.clear(); lib.clear(); slots.clear(); koff.clear(); pool.clear(); n_lib = 0; }
    bool parse(const char *text, int64_t l_text)
    {
        clear();
        std::string t(text ? text : "", text && l_text > 0 ? (size_t)l_text : 0);
        t = t.substr(0, t.find('\0'));
        std::unordered_map<std::string, uint32_t> by_lb, by_id;
        for (size_t at = 0; at < t.size();) {
            size_t nl = t.find('\n', at);
            if (nl == std::string::npos) nl = t.size();
            const std::string line = t.substr(at, nl - at);
            at = nl + 1;
            if (line.compare(0, 4, "@RG\t") != 0) continue;
            std::string id, lb;
            bool has_id = false, has_lb = false;
            for (size_t f = 4; f <= line.size();) {
                size_t tab = line.find('\t', f);
                if (tab == std::string::npos) tab = line.size();
                const std::string field = line.substr(f, tab - f);
                f = tab + 1;
                if (!has_id && field.compare(0, 3, "ID:") == 0) { id = field.substr(3); has_id = true; }
                if (!has_lb && field.compare(0, 3, "LB:") == 0) { lb = field.substr(3); has_lb = true; }
            }
            if (!has_id || id.empty() || by_id.count(id)) continue;
            uint32_t l;
            if (has_lb && by_lb.count(lb)) l = by_lb[lb];
            else {
                l = ++n_lib;
                if (has_lb) by_lb[lb] = l;
            }
            by_id[id] = l;
            ids.push_back(id); lib.push_back(l);
        }
        if (n_lib > DP_MAX_LIB) return false;
        if (ids.empty()) return true;
        size_t cap = 4;
        while (cap < 2 * ids.size()) cap <<= 1;
        slots.assign(cap, 0u);
        koff.push_back(0);
        for (const std::string &s : ids) { pool.insert(pool.end(), s.begin(), s.end()); koff.push_back((uint32_t)pool.size()); }
        for (size_t e = 0; e < ids.size(); ++e) {
            uint32_t i = dp_hash_id((const uint8_t *)ids[e].data(), (uint32_t)ids[e].size()) & (uint32_t)(cap - 1);
            while (slots[i]) i = (i + 1) & (uint32_t)(cap - 1);
            slots[i] = (uint32_t)e + 1;
        }
        return true;
    }
};

// A batch in host memory through the signature step, lane 0 of 1: true with one dp_sig per record, or false and in *bad the lowest broken record
static inline bool dp_signatures_on_host(const dp_libtab &T, const uint8_t *stream, uint64_t n_bytes, const uint64_t *off, uint64_t n, std::vector<dp_sig> *out, uint64_t *bad)
{
    out->assign(n, dp_sig{DP_HI_IGNORED, 0, 0, DP_IGNORED, 0, 0, 0});
    *bad = ED_NONE;
    if (n == 0 && n_bytes) { *bad = 0; return false; }
    for (uint64_t i = 0; i < n; ++i) {
        uint32_t span = 0, seq_at = 0, aux_at = 0;
        bool own = false;
        if (!ed_span(stream, n_bytes, off, i, n, &span, &own)) { *bad = i; return false; }
        if (!own) continue;          // (record i + 1 is the one named)
        const uint8_t *rec = stream + (off[i] - off[0]);
        if (!dp_head(rec, span, &seq_at, &aux_at)) { *bad = i; return false; }
        dp_signature<false>(T, rec, span, seq_at, aux_at, 0, 1, &(*out)[i]);
    }
    return true;
}
