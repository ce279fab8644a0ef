// rfilter_host.h -- the host side of the read filter's tables (dev_rfilter.h evaluates them): the rule set as the C-ABI collects it, and its compilation into
// the flat rule table, the sorted regions with their running maximum, the string pool and the dense motif automata.  Host only, no GPU, no HIP: slx_filter.hip
// uploads the result, slx_filter_test_record and tests/cpp/filter_host_test.cpp evaluate it where it stands.
#pragma once
#include <algorithm>
#include <cmath>
#include <cstdint>
#include <string>
#include <vector>
#include "seqlib_amd_filter.h"
#include "dev_rfilter.h"

struct RfHostRule { slx_filter_rule r; std::string rg; std::vector<std::string> motifs; };
struct RfHostFilter { bool excluder = false, mate = false; std::vector<slx_bam_region> regs; std::vector<RfHostRule> rules; };

struct RfCompiled {
    std::vector<rf_filter> flt; std::vector<rf_rule> rules; std::vector<rf_reg> regs; std::vector<uint8_t> strs; std::vector<uint32_t> dfa;
    rf_tab tab;          // with host pointers into the vectors above
    uint32_t n_states = 0;
};

static inline int rf_base_code(char c)
{
    const char *codes = "=ACMGRSVTWYHKDBN";
    for (int i = 0; i < 16; ++i) if (codes[i] == c) return i;
    return -1;
}

// Aho-Corasick over the 16 nibble codes with the failure links resolved into a dense table: entry [state * 16 + code] = (base + next) << 1 | next ends a motif
// (itself or along its failure chain).  A motif with a character outside =ACMGRSVTWYHKDBN, or an empty one, is left out: it never matches.  Appends the states
// to `table`, whose states so far number `base`; returns the root's state number.  *lmax: the longest motif taken.
static inline uint32_t rf_build_dfa(const std::vector<std::string> &motifs, std::vector<uint32_t> &table, uint32_t *lmax)
{
    const uint32_t base = (uint32_t)(table.size() / 16);
    std::vector<std::vector<int32_t>> go(1, std::vector<int32_t>(16, -1));
    std::vector<uint8_t> acc(1, 0);
    *lmax = 0;
    for (const std::string &m : motifs) {
        bool ok = !m.empty();
        for (char c : m) ok = ok && rf_base_code(c) >= 0;
        if (!ok) continue;
        uint32_t s = 0;
        for (char c : m) {
            const int k = rf_base_code(c);
            if (go[s][k] < 0) { go[s][k] = (int32_t)go.size(); go.emplace_back(16, -1); acc.push_back(0); }
            s = (uint32_t)go[s][k];
        }
        acc[s] = 1;
        *lmax = std::max<uint32_t>(*lmax, (uint32_t)m.size());
    }
    const size_t n = go.size();
    std::vector<uint32_t> fail(n, 0), order;
    order.reserve(n);
    for (int k = 0; k < 16; ++k) {
        if (go[0][k] < 0) go[0][k] = 0;
        else { fail[go[0][k]] = 0; order.push_back((uint32_t)go[0][k]); }
    }
    for (size_t q = 0; q < order.size(); ++q) {          // breadth first: a state's failure state is complete before the state is
        const uint32_t s = order[q];
        acc[s] |= acc[fail[s]];
        for (int k = 0; k < 16; ++k) {
            const int32_t t = go[s][k];
            if (t < 0) go[s][k] = go[fail[s]][k];
            else { fail[t] = (uint32_t)go[fail[s]][k]; order.push_back((uint32_t)t); }
        }
    }
    table.resize((size_t)(base + n) * 16);
    for (size_t s = 0; s < n; ++s)
        for (int k = 0; k < 16; ++k) table[(base + s) * 16 + k] = (base + (uint32_t)go[s][k]) << 1 | acc[go[s][k]];
    return base;
}

// false: more than RF_MAX_DFA rules with motifs
static inline bool rf_compile(const std::vector<RfHostFilter> &filters, RfCompiled &C)
{
    C = RfCompiled();
    rf_tab &T = C.tab;
    memset(&T, 0, sizeof T);
    uint32_t need = 0;
    for (const RfHostFilter &hf : filters) {
        rf_filter f;
        f.rule0 = (uint32_t)C.rules.size(); f.n_rules = (uint32_t)hf.rules.size(); f.reg0 = (uint32_t)C.regs.size(); f.n_regs = (uint32_t)hf.regs.size();
        f.excluder = hf.excluder; f.mate = hf.mate;
        if (f.n_regs) need |= RF_NEED_CIGAR;
        std::vector<slx_bam_region> g = hf.regs;
        std::stable_sort(g.begin(), g.end(), [](const slx_bam_region &a, const slx_bam_region &b) { return a.tid != b.tid ? a.tid < b.tid : a.beg < b.beg; });
        auto clamp = [](int64_t v) { return (int32_t)std::max<int64_t>(INT32_MIN, std::min<int64_t>(INT32_MAX, v)); };
        for (size_t i = 0; i < g.size(); ++i) {
            rf_reg r;
            r.chr = g[i].tid; r.p1 = clamp(g[i].beg); r.run_p2 = clamp(g[i].end);
            if (i && C.regs.back().chr == r.chr) r.run_p2 = std::max(r.run_p2, C.regs.back().run_p2);
            C.regs.push_back(r);
        }
        for (const RfHostRule &hr : hf.rules) {
            rf_rule R;
            memset(&R, 0, sizeof R);
            for (int i = 0; i < RF_R_N; ++i) { R.mn[i] = hr.r.r[i].min; R.mx[i] = hr.r.r[i].max; R.inv[i] = hr.r.r[i].inverted != 0; R.every[i] = hr.r.r[i].every != 0; }
            R.all_on = hr.r.all_on; R.all_off = hr.r.all_off; R.any_on = hr.r.any_on; R.any_off = hr.r.any_off; R.tri = hr.r.tri;
            R.seed = hr.r.subsample_seed;
            if (hr.r.subsample_frac < 1) {          // x / 2^24 >= f  <=>  x >= f * 2^24 (exact in doubles)  <=>  x >= ceil(f * 2^24) for an integer x
                const double t = hr.r.subsample_frac * 16777216.0;
                R.sub_on = 1; R.sub_thresh = t <= 0 ? 0u : (uint32_t)std::ceil(t);
                need |= RF_NEED_HASH;
            }
            if (!hr.rg.empty()) { R.rg_off = (uint32_t)C.strs.size(); R.rg_len = (uint32_t)hr.rg.size(); C.strs.insert(C.strs.end(), hr.rg.begin(), hr.rg.end()); need |= RF_NEED_AUX; }
            R.motif_bit = -1;
            if (!hr.motifs.empty()) {
                if (T.n_dfa >= RF_MAX_DFA) return false;
                T.root[T.n_dfa] = rf_build_dfa(hr.motifs, C.dfa, &T.lmax[T.n_dfa]);
                R.motif_bit = (int32_t)T.n_dfa++;
                need |= RF_NEED_MOTIF;
            }
            if (!R.every[RF_R_ISIZE] || !R.every[RF_R_CLIP] || !R.every[RF_R_INS] || !R.every[RF_R_DEL] || ((R.tri >> (2 * RF_T_HARDCLIP)) & 3u)) need |= RF_NEED_CIGAR;
            if (!R.every[RF_R_NM]) need |= RF_NEED_AUX;
            if (!R.every[RF_R_NBASES]) need |= RF_NEED_NCOUNT;
            C.rules.push_back(R);
        }
        C.flt.push_back(f);
    }
    C.n_states = (uint32_t)(C.dfa.size() / 16);
    if (C.strs.empty()) C.strs.push_back(0);
    T.flt = C.flt.data(); T.rules = C.rules.data(); T.regs = C.regs.data(); T.strs = C.strs.data(); T.dfa = C.dfa.data();
    T.n_flt = (uint32_t)C.flt.size(); T.need = need;
    return true;
}
