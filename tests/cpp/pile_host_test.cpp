// pile_host_test.cpp -- the host-compilable bodies of the pileup unit (seqlib_amd/csrc/pile_host.h) against what the Python statement of the rules wrote
// (tests/pile_util.py through tests/test_pile_host.py).  Stand-alone: no library, no GPU; tests/test_pile_host.py builds it with -fsanitize=address,undefined and
// runs it.
//   pile_host_test cases FILE        lines of FILE:
//     C name hex eligible min_baseq many beg end n (plane pos)...   pile_head's verdict for the window [beg, end) of contig 2 with the default parameters, and
//                                    pile_record's events for that window.  The record lies in a heap block of exactly its size, so a byte read past it is a
//                                    sanitizer report.  The body runs with 1 lane and, when many is 1, with 16 and 64 lanes: a lane is a thread of lanes_sim.h's
//                                    simulated group.  One lane gives the events in the walk's order; 16 and 64
//                                    lanes give the same events in some other order.
//     S min_depth min_alt num den ref_byte c0..c14 is_site ref depth alt ins     pile_site on one position
#include <algorithm>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <fstream>
#include <sstream>
#include <string>
#include <utility>
#include <vector>
#include "lanes_sim.h"
#include "pile_host.h"

static int g_fail = 0;
#define CHECK(c, ...) do { if (!(c)) { std::fprintf(stderr, "FAIL %s:%d: ", __FILE__, __LINE__); std::fprintf(stderr, __VA_ARGS__); std::fprintf(stderr, "\n"); ++g_fail; } } while (0)

typedef std::vector<std::pair<int32_t, int64_t>> Events;

static std::string unhex(const std::string &h)
{
    std::string s;
    if (h == "-") return s;
    for (size_t i = 0; i + 1 < h.size(); i += 2) s.push_back((char)std::stoi(h.substr(i, 2), nullptr, 16));
    return s;
}

struct ListSink {
    Events v;
    void operator()(uint32_t plane, int64_t x) { v.push_back({(int32_t)plane, x}); }
};

static Events run_lanes(const rf_feat &F, const pile_par &P, uint32_t nlanes)
{
    if (nlanes == 1) { ListSink S; pile_record(F, P, 0u, 1u, lanes_one(), S); return S.v; }
    std::vector<ListSink> sinks(nlanes);
    lanes_run(nlanes, [&](uint32_t l, const GroupLane &W) { pile_record(F, P, l, nlanes, W, sinks[l]); });
    Events all;
    for (const ListSink &s : sinks) all.insert(all.end(), s.v.begin(), s.v.end());
    return all;
}

static int run_cases(const char *path)
{
    std::ifstream f(path);
    if (!f) { std::fprintf(stderr, "cannot read %s\n", path); return 2; }
    std::string line;
    long n_cases = 0, n_sites = 0;
    while (std::getline(f, line)) {
        std::istringstream in(line);
        std::string kind;
        in >> kind;
        if (kind == "C") {
            std::string name, hex; int elig, min_baseq, many; int64_t cb, ce; size_t n;
            in >> name >> hex >> elig >> min_baseq >> many >> cb >> ce >> n;
            Events want(n);
            for (auto &w : want) in >> w.first >> w.second;
            const std::string r = unhex(hex);
            uint8_t *h = (uint8_t *)malloc(r.size());
            memcpy(h, r.data(), r.size());
            const pile_par dflt = {cb, ce, 2, 0, min_baseq, 0x704u, 64u, 1024u};
            rf_feat F;
            const int v = pile_head(h, r.size(), dflt, &F);
            CHECK((v > PILE_R_SKIP) == (elig != 0) && v != PILE_R_BAD, "%s: verdict %d, eligible %d", name.c_str(), v, elig);
            CHECK(v != PILE_R_LONG || F.n_cig > 64 || F.l_seq > 1024, "%s: LONG with %u ops and %d bases", name.c_str(), F.n_cig, F.l_seq);
            // the events, whatever the flags, the mapq and the contig say
            pile_par P = {cb, ce, 0, 0, min_baseq, 0u, 1u << 20, 0x7fffffffu};
            CHECK(rf_fixed(h, r.size(), &F), "%s: not a record", name.c_str());
            P.tid = F.tid;
            const bool walk = pile_head(h, r.size(), P, &F) > PILE_R_SKIP;
            CHECK(walk || want.empty(), "%s: skipped with %zu events expected", name.c_str(), want.size());
            if (walk) {
                Events sorted_want = want;
                std::sort(sorted_want.begin(), sorted_want.end());
                for (const uint32_t nlanes : {1u, 16u, 64u}) {
                    if (nlanes > 1 && !many) break;
                    Events got = run_lanes(F, P, nlanes);
                    if (nlanes == 1) CHECK(got == want, "%s min_baseq %d clip [%lld, %lld): one lane gives %zu events out of order or wrong, expected %zu", name.c_str(), min_baseq, (long long)cb, (long long)ce, got.size(), want.size());
                    std::sort(got.begin(), got.end());
                    CHECK(got == sorted_want, "%s min_baseq %d clip [%lld, %lld) with %u lanes: %zu events, expected %zu", name.c_str(), min_baseq, (long long)cb, (long long)ce, nlanes, got.size(), want.size());
                }
            }
            // cut short, the record is refused, never read past
            for (size_t cut : {(size_t)0, (size_t)35, r.size() - 1}) {
                uint8_t *q = (uint8_t *)malloc(cut ? cut : 1);
                memcpy(q, r.data(), cut);
                CHECK(pile_head(q, cut, P, &F) == PILE_R_BAD, "%s cut at %zu is not refused", name.c_str(), cut);
                free(q);
            }
            free(h);
            ++n_cases;
        } else if (kind == "S") {
            pile_site_par Q; int ref_byte, is_site; int32_t c[PILE_PLANES]; pile_site_val E, V;
            in >> Q.min_depth >> Q.min_alt >> Q.frac_num >> Q.frac_den >> ref_byte;
            for (int32_t &x : c) in >> x;
            in >> is_site >> E.ref >> E.depth >> E.alt >> E.ins;
            const bool got = pile_site(c, (uint32_t)ref_byte, Q, &V);
            CHECK(got == (is_site != 0) && V.ref == E.ref && V.depth == E.depth && V.alt == E.alt && V.ins == E.ins, "site line %ld: %d ref %d depth %d alt %d ins %d", n_sites, (int)got, V.ref, V.depth, V.alt, V.ins);
            ++n_sites;
        }
    }
    if (g_fail) return 1;
    std::printf("pile_host_test OK: %ld cases, %ld positions\n", n_cases, n_sites);
    return 0;
}

int main(int argc, char **argv)
{
    if (argc == 3 && !strcmp(argv[1], "cases")) return run_cases(argv[2]);
    std::fprintf(stderr, "usage: pile_host_test cases FILE\n");
    return 2;
}
