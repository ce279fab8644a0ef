// filter_host_test.cpp -- dev_rfilter.h and rfilter_host.h on the host with one lane, a program of its own for ASan + UBSan (tests/test_filter_host.py builds and
// runs it; nothing is loaded into Python).  Every buffer a body reads is allocated at exactly its size, so a read past a record, a stream, a stage or a table is a
// sanitizer report.
//   1. the DFA builder against naive substring search on random motif sets, whole texts and the chunked search of the long path (lanes 1, 3, 64; chunks 0, 1, 7, 64)
//   2. the features of random records against what the generator knows of them (CIGAR sums and maxima, N count) and against naive search
//   3. the window evaluator (rf_window) for several window / overhang sizes and the long-record evaluator for several lane and chunk counts, against the one-lane
//      evaluation of every record from an allocation of its own
//   4. damaged records: the error bits are set and nothing outside the record is read
// Prints "filter_host OK <records> <long records seen> <dfa states>".
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <random>
#include <string>
#include <vector>
#include "../../seqlib_amd/csrc/rfilter_host.h"

static int fails = 0;
#define CHECK(c) do { if (!(c)) { if (++fails < 20) printf("FAIL %s:%d %s\n", __FILE__, __LINE__, #c); } } while (0)

static std::mt19937 rng(12345);
static uint32_t rnd(uint32_t n) { return n ? (uint32_t)(rng() % n) : 0; }
static const char *CODES = "=ACMGRSVTWYHKDBN";

struct Known { uint64_t reflen = 0, qlen = 0; uint32_t clip = 0, hclip = 0, max_ins = 0, max_del = 0, n_n = 0; std::string seq; };

static void put32(std::vector<uint8_t> &o, uint32_t v) { for (int i = 0; i < 4; ++i) o.push_back((uint8_t)(v >> (8 * i))); }

static std::vector<uint8_t> make_record(uint32_t l_seq, uint32_t n_cig, Known &K, const std::string &plant)
{
    std::vector<uint8_t> b(36, 0);
    const std::string name = rnd(2) ? "r" + std::to_string(rnd(100000)) : "grp1:" + std::to_string(rnd(1000));
    const int32_t tid = (int32_t)rnd(4) - 1, pos = (int32_t)rnd(5000), mtid = rnd(3) ? tid : (int32_t)rnd(3), mpos = (int32_t)rnd(5000);
    const uint32_t flag = rng() & 0xfff;
    memcpy(&b[4], &tid, 4); memcpy(&b[8], &pos, 4);
    b[12] = (uint8_t)(name.size() + 1); b[13] = (uint8_t)rnd(61);
    b[16] = (uint8_t)n_cig; b[17] = (uint8_t)(n_cig >> 8); b[18] = (uint8_t)flag; b[19] = (uint8_t)(flag >> 8);
    memcpy(&b[20], &l_seq, 4); memcpy(&b[24], &mtid, 4); memcpy(&b[28], &mpos, 4);
    b.insert(b.end(), name.begin(), name.end()); b.push_back(0);
    for (uint32_t i = 0; i < n_cig; ++i) {
        const uint32_t op = rnd(9), len = 1 + rnd(op == 3 ? 2000 : 40);
        put32(b, len << 4 | op);
        if (op == 0 || op == 2 || op == 3 || op == 7 || op == 8) K.reflen += len;
        if (op == 0 || op == 1 || op == 4 || op == 7 || op == 8) K.qlen += len;
        if (op == 4 || op == 5) K.clip += len;
        if (op == 5) K.hclip += len;
        if (op == 1 && len > K.max_ins) K.max_ins = len;
        if (op == 2 && len > K.max_del) K.max_del = len;
    }
    K.seq.resize(l_seq);
    for (uint32_t i = 0; i < l_seq; ++i) K.seq[i] = rnd(12) ? "ACGT"[rnd(4)] : CODES[rnd(16)];
    if (!plant.empty() && l_seq >= plant.size() && rnd(3) == 0) K.seq.replace(rnd(l_seq - (uint32_t)plant.size() + 1), plant.size(), plant);
    for (char c : K.seq) K.n_n += c == 'N';
    std::vector<uint8_t> packed((l_seq + 1) / 2, 0);
    for (uint32_t i = 0; i < l_seq; ++i) packed[i >> 1] |= (uint8_t)((strchr(CODES, K.seq[i]) - CODES) << ((~i & 1) * 4));
    b.insert(b.end(), packed.begin(), packed.end());
    for (uint32_t i = 0; i < l_seq; ++i) b.push_back((uint8_t)rnd(41));
    if (rnd(2)) { const char z[] = "XZZsome text"; b.insert(b.end(), z, z + sizeof z); }
    if (rnd(2)) { b.push_back('X'); b.push_back('B'); b.push_back('B'); b.push_back('S'); put32(b, 3); for (int i = 0; i < 6; ++i) b.push_back((uint8_t)i); }
    if (rnd(3)) { b.push_back('N'); b.push_back('M'); b.push_back('C'); b.push_back((uint8_t)rnd(9)); }
    if (rnd(2)) { const char z[] = "RGZgrp1"; b.insert(b.end(), z, z + sizeof z); }
    const uint32_t bs = (uint32_t)b.size() - 4;
    memcpy(&b[0], &bs, 4);
    return b;
}

static slx_filter_rule every_rule()
{
    slx_filter_rule r;
    memset(&r, 0, sizeof r);
    for (auto &g : r.r) g.every = 1;
    r.subsample_frac = 1; r.subsample_seed = 999;
    return r;
}
static void set_range(slx_filter_rule &r, int i, int mn, int mx, bool inv) { r.r[i].min = mn; r.r[i].max = mx; r.r[i].inverted = inv; r.r[i].every = 0; }

static std::vector<std::vector<RfHostFilter>> rule_sets()
{
    std::vector<std::vector<RfHostFilter>> out;
    { RfHostFilter f; RfHostRule a; a.r = every_rule(); set_range(a.r, SLX_FR_MAPQ, 20, 60, false); f.rules.push_back(a); out.push_back({f}); }
    { RfHostFilter f; RfHostRule a; a.r = every_rule(); set_range(a.r, SLX_FR_CLIP, 0, 60, false); set_range(a.r, SLX_FR_NM, 0, 4, false); set_range(a.r, SLX_FR_INS, 0, 30, false);
      set_range(a.r, SLX_FR_ISIZE, 0, 3000, false); a.rg = "grp1"; f.rules.push_back(a); out.push_back({f}); }
    { RfHostFilter f; RfHostRule a; a.r = every_rule(); a.motifs = {"ACACG", "CACT", "GATTACAGATTACA", "acgt", ""}; f.rules.push_back(a);
      RfHostRule b; b.r = every_rule(); b.motifs = {"NN", "TTTTTT"}; set_range(b.r, SLX_FR_NBASES, 0, 3, true); f.rules.push_back(b); out.push_back({f}); }
    { RfHostFilter f; f.mate = true; f.regs = {{0, 1000, 2000}, {0, 100, 150}, {1, 0, 4000}, {0, 1100, 1200}}; RfHostRule a; a.r = every_rule(); a.r.subsample_frac = 0.5; a.r.tri = 2u << (2 * SLX_FT_DUP);
      f.rules.push_back(a); RfHostFilter x; x.excluder = true; RfHostRule c; c.r = every_rule(); c.r.tri = 1u << (2 * SLX_FT_FR); x.rules.push_back(c); out.push_back({f, x}); }
    out.push_back({});
    return out;
}

static bool naive_find(const std::string &text, const std::vector<std::string> &motifs)
{
    for (const std::string &m : motifs) {
        bool ok = !m.empty();
        for (char c : m) ok = ok && strchr(CODES, c) && c;
        if (ok && text.find(m) != std::string::npos) return true;
    }
    return false;
}

// one lane, the record in an allocation of exactly its size
static bool eval_alone(const rf_tab *T, const std::vector<uint8_t> &rec, uint32_t *er, rf_feat *Fout = nullptr)
{
    uint8_t *p = (uint8_t *)malloc(rec.size());
    memcpy(p, rec.data(), rec.size());
    rf_feat F;
    *er = rf_features(p, rec.size(), T, &F);
    const bool k = !*er && rf_eval(T, &F);
    if (Fout) *Fout = F;
    free(p);
    return k;
}

// the long path as k_flt_eval_long runs it, the lanes one after the other
static bool eval_long(const rf_tab *T, const uint8_t *h, uint64_t span, uint32_t nlanes, uint32_t chunk, uint32_t *er)
{
    rf_feat F;
    if (!rf_fixed(h, span, &F)) { *er = RF_E_FIELDS; return false; }
    rf_part P;
    memset(&P, 0, sizeof P);
    for (uint32_t l = 0; l < nlanes; ++l) { rf_part Q; rf_long_part(T, &F, chunk, l, nlanes, &Q); rf_part_join(&P, &Q); }
    return rf_long_finish(T, &F, &P, er);
}

int main()
{
    uint32_t dfa_states = 0;
    // 1. DFA against naive search
    for (int round = 0; round < 300; ++round) {
        std::vector<std::string> motifs;
        const uint32_t nm = 1 + rnd(6);
        for (uint32_t i = 0; i < nm; ++i) { std::string m; const uint32_t l = rnd(20) ? 1 + rnd(6) : 0; for (uint32_t j = 0; j < l; ++j) m += rnd(30) ? "ACGN"[rnd(4)] : 'x'; motifs.push_back(m); }
        std::vector<uint32_t> table;
        if (round & 1) table.assign(32, 0xffffffffu);          // a second set behind another one: states are numbered from the table's start
        uint32_t lmax = 0;
        const uint32_t root = rf_build_dfa(motifs, table, &lmax);
        dfa_states += (uint32_t)(table.size() / 16) - root;
        rf_tab T;
        memset(&T, 0, sizeof T);
        uint32_t *dfa = (uint32_t *)malloc(4 * table.size());
        memcpy(dfa, table.data(), 4 * table.size());
        T.dfa = dfa; T.n_dfa = 1; T.root[0] = root; T.lmax[0] = lmax; T.need = RF_NEED_MOTIF;
        for (int t = 0; t < 20; ++t) {
            const uint32_t L = rnd(60);
            std::string text;
            for (uint32_t i = 0; i < L; ++i) text += "ACGN"[rnd(4)];
            uint8_t *seq = (uint8_t *)malloc((L + 1) / 2 + 1);          // (+ 1: malloc(0) is not a buffer)
            memset(seq, 0, (L + 1) / 2 + 1);
            for (uint32_t i = 0; i < L; ++i) seq[i >> 1] |= (uint8_t)((strchr(CODES, text[i]) - CODES) << ((~i & 1) * 4));
            const bool want = naive_find(text, motifs);
            CHECK(rf_dfa_scan(dfa, root, seq, 0, 0, L) == want);
            rf_feat F;
            memset(&F, 0, sizeof F);
            F.seq = seq; F.l_seq = (int32_t)L;
            for (uint32_t nl : {1u, 3u, 64u})
                for (uint32_t cb : {0u, 1u, 7u, 64u}) {
                    uint64_t hits = 0;
                    for (uint32_t l = 0; l < nl; ++l) { rf_part P; rf_long_part(&T, &F, cb, l, nl, &P); hits |= P.hits; }
                    CHECK((hits != 0) == want);
                }
            free(seq);
        }
        free(dfa);
    }
    // 2. + 3. records
    std::vector<std::vector<uint8_t>> recs;
    std::vector<Known> known;
    for (int i = 0; i < 400; ++i) {
        Known K;
        const uint32_t kind = rnd(40);
        const uint32_t l_seq = kind == 0 ? 5000 + rnd(9000) : kind < 4 ? 0 : rnd(260), n_cig = kind == 1 ? 900 : rnd(4) ? rnd(8) : 0;
        recs.push_back(make_record(l_seq, n_cig, K, i % 2 ? "ACACT" : "GATTACAGATTACA"));
        known.push_back(K);
    }
    std::vector<uint64_t> off(1, 0);
    for (auto &r : recs) off.push_back(off.back() + r.size());
    const uint64_t n_bytes = off.back(), n_rec = recs.size();
    uint8_t *stream = (uint8_t *)malloc(n_bytes);
    for (size_t i = 0; i < recs.size(); ++i) memcpy(stream + off[i], recs[i].data(), recs[i].size());
    uint64_t *d_off = (uint64_t *)malloc(8 * (n_rec + 1));
    memcpy(d_off, off.data(), 8 * (n_rec + 1));
    uint32_t long_seen = 0;
    const auto sets = rule_sets();
    for (size_t si = 0; si < sets.size(); ++si) {
        RfCompiled C;
        CHECK(rf_compile(sets[si], C));
        const rf_tab *T = &C.tab;
        std::vector<uint8_t> want(n_rec);
        for (size_t i = 0; i < n_rec; ++i) {
            uint32_t er;
            rf_feat F;
            want[i] = eval_alone(T, recs[i], &er, &F);
            CHECK(er == 0);
            if (T->need & RF_NEED_CIGAR) CHECK(F.reflen == known[i].reflen && F.qlen == known[i].qlen && F.clip == known[i].clip && F.hclip == known[i].hclip && F.max_ins == known[i].max_ins && F.max_del == known[i].max_del);
            if (T->need & RF_NEED_NCOUNT) CHECK(F.n_n == known[i].n_n);
            for (size_t ri = 0, bit = 0; si < sets.size() && !sets[si].empty() && ri < sets[si][0].rules.size(); ++ri)
                if (!sets[si][0].rules[ri].motifs.empty()) { CHECK((((F.hits >> bit) & 1) != 0) == naive_find(known[i].seq, sets[si][0].rules[ri].motifs)); ++bit; }
        }
        if (si + 1 < sets.size()) { size_t k = 0; for (uint8_t w : want) k += w; CHECK(k > 0 && k < n_rec); }
        const uint32_t WV[][2] = {{64, 48}, {256, 64}, {4096, 512}, {16384, 2048}};
        for (auto &wv : WV) {
            const uint32_t W = wv[0], V = wv[1];
            uint8_t *lds = (uint8_t *)aligned_alloc(16, W + V + 16);
            uint8_t *keep = (uint8_t *)malloc(n_rec);
            memset(keep, 7, n_rec);
            uint32_t *long_list = (uint32_t *)malloc(4 * n_rec), st[2] = {0, 0}, kept = 0;
            for (uint64_t w = 0; w * W < n_bytes; ++w) kept += rf_window(stream, n_bytes, d_off, n_rec, w, W, V, lds, T, keep, long_list, &st[0], &st[1], 0, 1);
            CHECK(st[1] == 0);
            long_seen += st[0];
            const uint32_t lanes[] = {1, 5, 64}, chunks[] = {0, 3, 100};
            for (uint32_t i = 0; i < st[0]; ++i) {
                const uint64_t r = long_list[i];
                uint32_t er;
                const bool k = eval_long(T, stream + d_off[r], d_off[r + 1] - d_off[r], lanes[i % 3], chunks[(i / 3) % 3], &er);
                CHECK(er == 0);
                keep[r] = k; kept += k;
            }
            size_t sum = 0;
            for (size_t i = 0; i < n_rec; ++i) { CHECK(keep[i] == want[i]); sum += want[i]; }
            CHECK(kept == sum);
            free(lds); free(keep); free(long_list);
        }
    }
    CHECK(long_seen > 0);
    // 4. damaged records, alone and inside a stream of exactly their size
    {
        RfCompiled C;
        CHECK(rf_compile(sets[1], C));
        Known K;
        std::vector<uint8_t> good = make_record(9, 2, K, "");
        auto retail = [&](std::vector<uint8_t> r, std::initializer_list<uint8_t> aux) {          // the aux fields replaced
            rf_feat F;
            rf_fixed(r.data(), r.size(), &F);
            r.resize((size_t)(F.aux - r.data()));
            r.insert(r.end(), aux);
            const uint32_t bs = (uint32_t)r.size() - 4;
            memcpy(&r[0], &bs, 4);
            return r;
        };
        std::vector<std::vector<uint8_t>> bad;
        bad.push_back(retail(good, {'N', 'M', 'i', 1, 0}));
        bad.push_back(retail(good, {'N', 'M', 'C', 1, 'X'}));
        bad.push_back(retail(good, {'X', 'Z', 'Z', 'a', 'b'}));
        bad.push_back(retail(good, {'X', 'B', 'B', 'S', 0xe8, 3, 0, 0, 1, 0}));
        bad.push_back(retail(good, {'X', 'B', 'B', 'I', 0xff, 0xff, 0xff, 0xff, 1, 0}));
        bad.push_back(retail(good, {'X', 'Q', 'q', 1}));
        { std::vector<uint8_t> r = good; r[16] = 0x60; r[17] = 0xea; bad.push_back(r); }                 // n_cigar 60000
        { std::vector<uint8_t> r = good; r[20] = 0xff; r[21] = 0xff; r[22] = 0xff; r[23] = 0x7f; bad.push_back(r); }      // l_seq 2^31 - 1
        { std::vector<uint8_t> r = good; r[23] = 0x80; bad.push_back(r); }                                 // l_seq negative
        { std::vector<uint8_t> r = good; r[0] ^= 1; bad.push_back(r); }                                    // block_size is not the span
        for (auto &r : bad) {
            uint32_t er;
            CHECK(!eval_alone(&C.tab, r, &er) && er != 0);
            uint8_t *s = (uint8_t *)malloc(r.size());
            memcpy(s, r.data(), r.size());
            uint32_t e2;
            CHECK(!eval_long(&C.tab, s, r.size(), 64, 0, &e2) && e2 != 0);
            const uint64_t o2[2] = {0, r.size()};
            uint8_t *lds = (uint8_t *)aligned_alloc(16, 256 + 64 + 16), keep = 9;
            uint32_t ll[1], st[2] = {0, 0};
            rf_window(s, r.size(), o2, 1, 0, 256, 64, lds, &C.tab, &keep, ll, &st[0], &st[1], 0, 1);
            CHECK(st[1] != 0 && keep == 0);
            free(lds); free(s);
        }
    }
    free(stream); free(d_off);
    if (fails) { printf("filter_host FAILED %d\n", fails); return 1; }
    printf("filter_host OK %zu %u %u\n", (size_t)n_rec, long_seen, dfa_states);
    return 0;
}
