// The lane-made chain header of the extension walk (seqlib_amd/csrc/dev_chain_hdr.h) compiled for the host: chains are built here and the
// header's window, top seed and one-seed seedcov are compared with a literal restatement of the checker's mem_chain2aln
// (oracle/orc_mem.c: the rmax loop, its clamps, the l_pac rule, bns_fetch_seq's clip to the contig; the (score, index) sort's last element;
// the seedcov loop).  Stand-alone: g++ -fsanitize=address,undefined chain_hdr_test.cpp && ./a.out
#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <random>
#include <vector>
#include "../../seqlib_amd/csrc/dev_chain_hdr.h"

struct Opt { int a = 1, o_del = 6, e_del = 1, o_ins = 6, e_ins = 1, w = 100; };
struct Seed { int64_t rbeg; int qbeg, len, score; };
struct Contig { int64_t offset; int32_t len; };

// ---- the checker, restated
static int ref_cal_max_gap(const Opt *opt, int qlen)
{
    int l_del = (int)((double)(qlen * opt->a - opt->o_del) / opt->e_del + 1.);
    int l_ins = (int)((double)(qlen * opt->a - opt->o_ins) / opt->e_ins + 1.);
    int l = l_del > l_ins ? l_del : l_ins;
    l = l > 1 ? l : 1;
    return l < opt->w << 1 ? l : opt->w << 1;
}
static int ref_pos2rid(int64_t l_pac, const std::vector<Contig> &anns, int64_t pos_f)
{
    int left, mid, right, n_seqs = (int)anns.size();
    if (pos_f >= l_pac) return -1;
    left = 0; mid = 0; right = n_seqs;
    while (left < right) {
        mid = (left + right) >> 1;
        if (pos_f >= anns[mid].offset) {
            if (mid == n_seqs - 1) break;
            if (pos_f < anns[mid + 1].offset) break;
            left = mid + 1;
        } else right = mid;
    }
    return mid;
}
struct RefHdr { int64_t rmax[2]; int rid; int top; };
static RefHdr ref_header(const Opt *opt, int64_t l_pac, const std::vector<Contig> &anns, int l_query, const std::vector<Seed> &seeds)
{
    RefHdr h;
    int64_t *rmax = h.rmax;
    const int n = (int)seeds.size();
    rmax[0] = l_pac << 1; rmax[1] = 0;
    for (int i = 0; i < n; ++i) {
        int64_t b, e;
        const Seed *t = &seeds[i];
        b = t->rbeg - (t->qbeg + ref_cal_max_gap(opt, t->qbeg));
        e = t->rbeg + t->len + ((l_query - t->qbeg - t->len) + ref_cal_max_gap(opt, l_query - t->qbeg - t->len));
        rmax[0] = rmax[0] < b ? rmax[0] : b;
        rmax[1] = rmax[1] > e ? rmax[1] : e;
    }
    rmax[0] = rmax[0] > 0 ? rmax[0] : 0;
    rmax[1] = rmax[1] < l_pac << 1 ? rmax[1] : l_pac << 1;
    if (rmax[0] < l_pac && l_pac < rmax[1]) {
        if (seeds[0].rbeg < l_pac) rmax[1] = l_pac;
        else rmax[0] = l_pac;
    }
    {   // bns_fetch_seq(idx, &rmax[0], seeds[0].rbeg, &rmax[1], &rid)
        int64_t far_beg, far_end, mid = seeds[0].rbeg;
        int is_rev = mid >= l_pac;
        h.rid = ref_pos2rid(l_pac, anns, is_rev ? (l_pac << 1) - 1 - mid : mid);
        far_beg = anns[h.rid].offset;
        far_end = far_beg + anns[h.rid].len;
        if (is_rev) {
            int64_t t = far_beg;
            far_beg = (l_pac << 1) - far_end;
            far_end = (l_pac << 1) - t;
        }
        rmax[0] = rmax[0] > far_beg ? rmax[0] : far_beg;
        rmax[1] = rmax[1] < far_end ? rmax[1] : far_end;
    }
    std::vector<uint64_t> srt(n);
    for (int i = 0; i < n; ++i) srt[i] = (uint64_t)seeds[i].score << 32 | (uint64_t)i;
    std::sort(srt.begin(), srt.end());
    h.top = (int)(uint32_t)srt[n - 1];          // k = n - 1, the seed the walk takes first
    return h;
}
static int ref_seedcov(const std::vector<Seed> &seeds, int a_qb, int a_qe, int64_t a_rb, int64_t a_re)
{
    int cov = 0;
    for (size_t i = 0; i < seeds.size(); ++i) {
        const Seed *t = &seeds[i];
        if (t->qbeg >= a_qb && t->qbeg + t->len <= a_qe && t->rbeg >= a_rb && t->rbeg + t->len <= a_re) cov += t->len;
    }
    return cov;
}

// ---- the header's policies over the same seeds: slots are a permutation of the list, as after the chaining kernel's flattening
struct SeedView {
    const std::vector<Seed> *slots;
    int qbeg(int s) const { return (*slots)[(size_t)s].qbeg; }
    int len(int s) const { return (*slots)[(size_t)s].len; }
    int64_t rbeg(int s) const { return (*slots)[(size_t)s].rbeg; }
    int score(int s) const { return (*slots)[(size_t)s].score; }
};

static int n_fail = 0, n_checked = 0, n_made = 0, n_unmade = 0, n_straddle = 0, n_clipped = 0, n_rev = 0, n_cov0 = 0;
#define CHECK(cond, ...) do { if (!(cond)) { ++n_fail; fprintf(stderr, "FAIL %s:%d: ", __FILE__, __LINE__); fprintf(stderr, __VA_ARGS__); fprintf(stderr, "\n"); } } while (0)

static void run_chain(const Opt &opt, int64_t l_pac, const std::vector<Contig> &anns, int l_query, const std::vector<Seed> &seeds, std::mt19937 &rng, const char *what)
{
    const int n = (int)seeds.size();
    // the read's slots hold the chain's seeds in shuffled order among seeds of other chains; cs[] lists the chain's slots in list order
    const int pad = 5;
    std::vector<int> perm((size_t)n + pad);
    for (size_t i = 0; i < perm.size(); ++i) perm[i] = (int)i;
    std::shuffle(perm.begin(), perm.end(), rng);
    std::vector<Seed> slots((size_t)n + pad, Seed{7, 3, 19, 19});
    std::vector<int> cs((size_t)n);
    for (int i = 0; i < n; ++i) { cs[(size_t)i] = perm[(size_t)i]; slots[(size_t)perm[(size_t)i]] = seeds[(size_t)i]; }
    std::vector<int64_t> ann_off; std::vector<int32_t> ann_len;
    for (const Contig &c : anns) { ann_off.push_back(c.offset); ann_len.push_back(c.len); }
    std::vector<int> lut((size_t)l_query + 2);
    for (int q = 0; q < l_query + 2; ++q) lut[(size_t)q] = ref_cal_max_gap(&opt, q);
    auto gap = [&](int q) { return lut[(size_t)(q < 0 ? 0 : (q > l_query + 1 ? l_query + 1 : q))]; };      // the kernel's LDS table and its clamp
    SeedView sv{&slots};
    ChainHdr h;
    const bool made = chain_hdr_make(h, cs.data(), n, sv, gap, l_query, l_pac, (int)anns.size(), ann_off.data(), ann_len.data());
    ++n_checked;
    CHECK(made == (n >= 1 && n <= CHDR_MAX_SEEDS), "%s: n = %d made = %d", what, n, (int)made);
    if (!made) { ++n_unmade; return; }
    ++n_made;
    const RefHdr r = ref_header(&opt, l_pac, anns, l_query, seeds);
    CHECK(h.rmax0 == r.rmax[0] && h.rmax1 == r.rmax[1], "%s: n = %d window [%lld, %lld), the checker [%lld, %lld)", what, n, (long long)h.rmax0, (long long)h.rmax1,
          (long long)r.rmax[0], (long long)r.rmax[1]);
    CHECK(h.rid == r.rid, "%s: rid %d, the checker %d", what, h.rid, r.rid);
    const Seed &t = seeds[(size_t)r.top];
    CHECK(h.top_s == cs[(size_t)r.top] && h.top_qbeg == t.qbeg && h.top_len == t.len && h.top_rbeg == t.rbeg, "%s: n = %d top seed slot %d, the checker's list index %d (slot %d)", what,
          n, h.top_s, r.top, cs[(size_t)r.top]);
    // what the cases are there for
    {
        int64_t lo = l_pac << 1, hi = 0;
        for (const Seed &s : seeds) {
            lo = std::min(lo, s.rbeg - (s.qbeg + ref_cal_max_gap(&opt, s.qbeg)));
            hi = std::max(hi, s.rbeg + s.len + ((l_query - s.qbeg - s.len) + ref_cal_max_gap(&opt, l_query - s.qbeg - s.len)));
        }
        if (lo < l_pac && l_pac < hi) ++n_straddle;
        if (h.rmax0 > std::max<int64_t>(lo, 0) || h.rmax1 < std::min(hi, l_pac << 1)) ++n_clipped;
        if (seeds[0].rbeg >= l_pac) ++n_rev;
    }
    if (n == 1) {
        // the one-seed shortcut against the general loop, on regions that do and do not contain the seed (a region of mem_chain2aln always does; not assumed)
        const Seed &s = seeds[0];
        for (int dq0 = -2; dq0 <= 2; ++dq0) for (int dq1 = -2; dq1 <= 2; ++dq1) for (int dr0 = -2; dr0 <= 2; ++dr0) for (int dr1 = -2; dr1 <= 2; ++dr1) {
            const int a_qb = s.qbeg + dq0, a_qe = s.qbeg + s.len + dq1;
            const int64_t a_rb = s.rbeg + dr0, a_re = s.rbeg + s.len + dr1;
            const int got = chain_hdr_seedcov1(h.top_qbeg, h.top_len, h.top_rbeg, a_qb, a_qe, a_rb, a_re), exp = ref_seedcov(seeds, a_qb, a_qe, a_rb, a_re);
            CHECK(got == exp, "%s: seedcov %d, the general loop %d", what, got, exp);
            n_cov0 += exp == 0;
        }
        const int full = chain_hdr_seedcov1(h.top_qbeg, h.top_len, h.top_rbeg, 0, l_query, h.rmax0, h.rmax1);
        CHECK(full == s.len && full == ref_seedcov(seeds, 0, l_query, h.rmax0, h.rmax1), "%s: seedcov of the whole window %d, seed length %d", what, full, s.len);
    }
}

int main()
{
    Opt opt;
    std::mt19937 rng(7);
    // three contigs; l_pac is their sum, coordinates >= l_pac are the reverse strand
    const std::vector<Contig> anns = {{0, 5000}, {5000, 301}, {5301, 9000}};
    const int64_t l_pac = 14301;
    auto U = [&](int lo, int hi) { return lo + (int)(rng() % (unsigned)(hi - lo + 1)); };
    for (int l_query : {40, 150}) {
        for (int n : {1, 2, 8, 9, 65}) {
            // seeds of one chain: on one contig and one strand, on two diagonals, scores (lengths) with ties so that the list index decides the top seed
            auto make = [&](int64_t first_rbeg, int first_qbeg, int first_len) {
                std::vector<Seed> v;
                for (int i = 0; i < n; ++i) {
                    Seed s;
                    if (i == 0) { s.qbeg = first_qbeg; s.len = first_len; s.rbeg = first_rbeg; }
                    else {
                        s.len = std::min(19 + U(0, 3), l_query);
                        s.qbeg = U(0, l_query - s.len);
                        s.rbeg = first_rbeg - first_qbeg + s.qbeg + (i & 1 ? 0 : U(-4, 4));
                    }
                    s.score = s.len;
                    v.push_back(s);
                }
                return v;
            };
            const int sl = std::min(25, l_query);
            struct Pos { const char *what; int64_t rbeg; int qbeg; } pos[] = {
                {"contig 0, first base", 0, 0},
                {"contig 0, first bases, seed inside the read", 3, 10},
                {"contig 0, last bases", 5000 - sl, l_query - sl},
                {"contig 1 (301 bases), both ends clipped", 5000 + 120, 7},
                {"contig 2, first base", 5301, 0},
                {"contig 2, last bases: the window would cross l_pac", l_pac - sl - 2, 2},
                {"contig 2, middle", 9000, 5},
                {"reverse strand, contig 2's last bases (first after l_pac): the window would cross l_pac", l_pac + 1, l_query - sl - 1},
                {"reverse strand, contig 2, ends at its first base", 2 * l_pac - 5301 - sl, l_query - sl},
                {"reverse strand, contig 1", 2 * l_pac - 5301 + 100, 4},
                {"reverse strand, contig 0, last position", 2 * l_pac - sl, l_query - sl},
                {"reverse strand, contig 0, middle", 2 * l_pac - 2500, 9},
            };
            for (const Pos &p : pos)
                for (int rep = 0; rep < 4; ++rep) {
                    std::vector<Seed> v = make(p.rbeg, p.qbeg, sl);
                    // keep every seed on the first seed's strand and inside the coordinate space (a chain never mixes strands)
                    const bool rev = p.rbeg >= l_pac;
                    for (Seed &s : v) {
                        const int64_t lo = rev ? l_pac : 0, hi = (rev ? 2 * l_pac : l_pac) - s.len;
                        s.rbeg = std::max(lo, std::min(hi, s.rbeg));
                    }
                    if (rep == 1 && n > 1) for (Seed &s : v) s.score = 19;                     // all scores equal: the LAST list index is the top seed
                    if (rep == 2 && n > 1) v[(size_t)U(0, n - 1)].score = 1000;                // mem_flt_chained_seeds' scores differ from the lengths
                    if (rep == 3 && n > 1) v[0].score = v[(size_t)n - 1].score = 24;
                    run_chain(opt, l_pac, anns, l_query, v, rng, p.what);
                }
        }
    }
    printf("chains %d (headers made %d, left to the wave %d), windows crossing l_pac %d, clipped to the contig %d, reverse strand %d, one-seed regions without the seed %d, failures %d\n",
           n_checked, n_made, n_unmade, n_straddle, n_clipped, n_rev, n_cov0, n_fail);
    if (n_made == 0 || n_unmade == 0 || n_straddle == 0 || n_clipped == 0 || n_rev == 0 || n_cov0 == 0) { fprintf(stderr, "a case class is missing\n"); return 2; }
    return n_fail ? 1 : 0;
}
