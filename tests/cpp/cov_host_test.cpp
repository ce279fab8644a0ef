// cov_host_test.cpp -- the host-compilable bodies of the coverage unit (seqlib_amd/csrc/cov_host.h) against what the Python statement of the rules wrote
// (tests/cov_util.py through tests/test_cov_host.py).  Stand-alone: no library, no GPU; tests/test_cov_host.py builds it with -fsanitize=address,undefined and runs it.
//   cov_host_test layout LEN...     prints the offset of every contig and the total, in entries
//   cov_host_test dec VALUE...      prints every value through cov_dec_put / cov_depth_put, one per line
//   cov_host_test cases FILE        lines of FILE:
//     R n_ref (name len)...                              the contigs
//     C name hex eligible mode buff count_del beg end n (lo hi)...   cov_head's verdict with the default parameters, and cov_record's intervals for the clip [beg, end),
//                                                        by one lane and by the 64 lanes of tests/cpp/lanes_sim.h (the same intervals as a multiset);
//                                                        the record lies in a heap block of exactly its size, so a byte read past it is a sanitizer report
//     B mode buff count_del include_zero hex             all C records so far through cov_head + cov_record into the difference array of the layout, a prefix sum,
//                                                        and cov_bg_piece over every entry: the text
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <fstream>
#include <iostream>
#include <sstream>
#include <string>
#include <vector>
#include <algorithm>
#include "cov_host.h"
#include "lanes_sim.h"

static int g_fail = 0;
#define CHECK(c, ...) do { if (!(c)) { std::fprintf(stderr, "FAIL %s:%d: ", __FILE__, __LINE__); std::fprintf(stderr, __VA_ARGS__); std::fprintf(stderr, "\n"); ++g_fail; } } while (0)

static std::string unhex(const std::string &h)
{
    std::string s;
    if (h == "-") return s;
    for (size_t i = 0; i + 1 < h.size(); i += 2) s.push_back((char)std::stoi(h.substr(i, 2), nullptr, 16));
    return s;
}

struct ListSink {
    std::vector<std::pair<int64_t, int64_t>> v;
    void operator()(int32_t, int64_t lo, int64_t hi) { v.push_back({lo, hi}); }
};
struct ArraySink {
    std::vector<int32_t> *a; const cov_geo *G;
    void operator()(int32_t tid, int64_t lo, int64_t hi) { (*a)[(size_t)(G->off[tid] + lo - G->beg[tid])] += 1; (*a)[(size_t)(G->off[tid] + hi - G->beg[tid])] -= 1; }
};

static int run_cases(const char *path)
{
    std::ifstream f(path);
    if (!f) { std::fprintf(stderr, "cannot read %s\n", path); return 2; }
    std::vector<std::string> names;
    std::vector<int64_t> len, beg, off;
    std::vector<std::string> recs;
    std::string line;
    long n_cases = 0, n_texts = 0;
    while (std::getline(f, line)) {
        std::istringstream in(line);
        std::string kind;
        in >> kind;
        if (kind == "R") {
            int n; in >> n;
            for (int i = 0; i < n; ++i) { std::string nm; int64_t l; in >> nm >> l; names.push_back(nm); len.push_back(l); }
            beg.assign(len.size(), 0); off.assign(len.size(), 0);
        } else if (kind == "C") {
            std::string name, hex; int elig, mode, buff, cd; int64_t cb, ce; size_t n;
            in >> name >> hex >> elig >> mode >> buff >> cd >> cb >> ce >> n;
            std::vector<std::pair<int64_t, int64_t>> want(n);
            for (auto &w : want) in >> w.first >> w.second;
            const std::string r = unhex(hex);
            uint8_t *h = (uint8_t *)malloc(r.size());
            memcpy(h, r.data(), r.size());
            const cov_par dflt = {COV_ALIGNED, 0, 0, 0, 0x704u, 64u};
            rf_feat F;
            const int v = cov_head(h, r.size(), dflt, (int32_t)len.size(), &F);
            CHECK((v > COV_R_SKIP) == (elig != 0) && v != COV_R_BAD, "%s: verdict %d, eligible %d", name.c_str(), v, elig);
            CHECK(v != COV_R_LONG || F.n_cig > 64, "%s: LONG with %u ops", name.c_str(), F.n_cig);
            const cov_par P = {mode, buff, cd, 0, 0u, 1u << 20};
            ListSink S;
            const int64_t o = 0;
            const cov_geo G = {&cb, &ce, &o, 1, 0, 0};
            const bool elig_walk = cov_head(h, r.size(), P, 0x7fffffff, &F) > COV_R_SKIP;
            if (elig_walk) {
                F.tid = 0;
                cov_record(F, P, G, 0u, 1u, lanes_one(), S);
            }
            CHECK(S.v == want, "%s mode %d buff %d count_del %d: %zu intervals, expected %zu", name.c_str(), mode, buff, cd, S.v.size(), want.size());
            // the same record by 64 lanes that call together (the long-record kernel's path): the same intervals in some other order
            if (elig_walk) {
                std::vector<ListSink> sinks(64);
                lanes_run(64u, [&](uint32_t l, const GroupLane &W) { cov_record(F, P, G, l, 64u, W, sinks[l]); });
                std::vector<std::pair<int64_t, int64_t>> got, one = S.v;
                for (const ListSink &s : sinks) got.insert(got.end(), s.v.begin(), s.v.end());
                std::sort(got.begin(), got.end()); std::sort(one.begin(), one.end());
                CHECK(got == one, "%s mode %d buff %d count_del %d with 64 lanes: %zu intervals, one lane gives %zu", name.c_str(), mode, buff, cd, got.size(), one.size());
            }
            // cut short, the record is refused, never read past
            for (size_t cut : {(size_t)0, (size_t)35, r.size() - 1}) {
                uint8_t *q = (uint8_t *)malloc(cut ? cut : 1);
                memcpy(q, r.data(), cut);
                CHECK(cov_head(q, cut, P, 0x7fffffff, &F) == COV_R_BAD, "%s cut at %zu is not refused", name.c_str(), cut);
                free(q);
            }
            free(h);
            if (recs.empty() || recs.back() != r) recs.push_back(r);
            ++n_cases;
        } else if (kind == "B") {
            int mode, buff, cd, iz; std::string hex;
            in >> mode >> buff >> cd >> iz >> hex;
            const std::string want = unhex(hex);
            const uint64_t total = cov_layout(len.data(), (int32_t)len.size(), off.data());
            const cov_geo G = {beg.data(), len.data(), off.data(), (int32_t)len.size(), 0, (int64_t)total};
            std::vector<int32_t> a(total, 0);          // exactly the layout's size: an entry past it is a sanitizer report
            const cov_par P = {mode, buff, cd, 0, 0x704u, 1u << 20};
            ArraySink S = {&a, &G};
            for (const std::string &r : recs) {
                rf_feat F;
                if (cov_head((const uint8_t *)r.data(), r.size(), P, G.n_ref, &F) > COV_R_SKIP) cov_record(F, P, G, 0u, 1u, lanes_one(), S);
            }
            for (uint64_t g = 1; g < total; ++g) a[g] += a[g - 1];
            std::string nm; std::vector<uint32_t> noff(1, 0);
            for (const std::string &s : names) { nm += s; noff.push_back((uint32_t)nm.size()); }
            const cov_names N = {(const uint8_t *)nm.data(), noff.data()};
            std::string text;
            for (uint64_t g = 0; g < total; ++g) {
                uint32_t head = 0;
                const uint32_t n = cov_bg_piece(a.data(), G, N, g, iz, nullptr, &head);
                if (!n) continue;
                uint8_t *o = (uint8_t *)malloc(n);
                CHECK(cov_bg_piece(a.data(), G, N, g, iz, o, &head) == n, "entry %llu: the piece's two lengths differ", (unsigned long long)g);
                text.append((const char *)o, n);
                free(o);
            }
            CHECK(text == want, "bedGraph mode %d buff %d count_del %d include_zero %d: %zu bytes, expected %zu", mode, buff, cd, iz, text.size(), want.size());
            ++n_texts;
        }
    }
    if (g_fail) return 1;
    std::printf("cov_host_test OK: %ld cases, %ld texts\n", n_cases, n_texts);
    return 0;
}

int main(int argc, char **argv)
{
    if (argc >= 2 && !strcmp(argv[1], "layout")) {
        std::vector<int64_t> len, off((size_t)argc, 0);
        for (int i = 2; i < argc; ++i) len.push_back(std::atoll(argv[i]));
        const uint64_t total = cov_layout(len.data(), (int32_t)len.size(), off.data());
        for (size_t i = 0; i < len.size(); ++i) std::printf("%lld\n", (long long)off[i]);
        std::printf("%llu\n", (unsigned long long)total);
        return 0;
    }
    if (argc >= 2 && !strcmp(argv[1], "dec")) {
        for (int i = 2; i < argc; ++i) {
            const long long v = std::atoll(argv[i]);
            uint8_t *o = (uint8_t *)malloc(v < 0 ? cov_depth_len((int32_t)v) : cov_dec_len((uint64_t)v));
            const uint32_t n = v < 0 ? cov_depth_put(o, (int32_t)v) : cov_dec_put(o, (uint64_t)v);
            std::printf("%.*s\n", (int)n, (const char *)o);
            free(o);
        }
        return 0;
    }
    if (argc == 3 && !strcmp(argv[1], "cases")) return run_cases(argv[2]);
    std::fprintf(stderr, "usage: cov_host_test layout LEN... | dec VALUE... | cases FILE\n");
    return 2;
}
