// grc_host_test.cpp -- csrc/grc_host.h on the host, under ASan + UBSan (tests/test_grc_host.py builds and runs it): the host build of the index, the searches, the
// exact count, the fill, the width sweep and the merge flags over the case list of tests/grc_util.py, every array in a heap block of exactly its size.
//   grc_host_test cases FILE
// FILE:  S n (chr p1 p2 strand)*                      a subject set: builds the index
//        X (chr p1 p2 strand perm run_p2 ends)*       ... whose arrays must be these
//        M m (chr p1 p2 strand)*                      ... and whose merge must be this
//        Q chr p1 p2 strand flags width k (sid c1 c2)*   a query against it
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <fstream>
#include <sstream>
#include <string>
#include <vector>
#include "grc_host.h"

static int fail(const std::string &what, const std::string &line)
{
    std::fprintf(stderr, "grc_host_test: %s\n  %s\n", what.c_str(), line.substr(0, 300).c_str());
    return 1;
}

static bool read_iv(std::istringstream &in, grc_iv &v)
{
    long long c, a, b;
    std::string s;
    if (!(in >> c >> a >> b >> s)) return false;
    std::memset(&v, 0, sizeof v);
    v.chr = (int32_t)c; v.pos1 = (int32_t)a; v.pos2 = (int32_t)b; v.strand = s[0];
    return true;
}

int main(int argc, char **argv)
{
    if (argc != 3 || std::strcmp(argv[1], "cases")) { std::fprintf(stderr, "usage: grc_host_test cases FILE\n"); return 2; }
    std::ifstream f(argv[2]);
    if (!f) return fail("cannot open", argv[2]);
    grc_host_arrays H;
    std::string line;
    long n_sets = 0, n_queries = 0, n_merges = 0;
    while (std::getline(f, line)) {
        std::istringstream in(line);
        std::string tag;
        in >> tag;
        if (tag == "S") {
            size_t n;
            in >> n;
            grc_iv *v = (grc_iv *)std::malloc(n ? n * sizeof(grc_iv) : 1);          // exactly n: a read past it is a report
            for (size_t i = 0; i < n; ++i) if (!read_iv(in, v[i])) return fail("short S line", line);
            H = grc_host_arrays();
            grc_build_host(v, (uint32_t)n, H);
            H.chr.shrink_to_fit(); H.p1.shrink_to_fit(); H.p2.shrink_to_fit(); H.run_p2.shrink_to_fit(); H.ends.shrink_to_fit(); H.seg_chr.shrink_to_fit(); H.seg_beg.shrink_to_fit();
            std::free(v);
            ++n_sets;
        } else if (tag == "X") {
            for (size_t i = 0; i < H.chr.size(); ++i) {
                grc_iv v;
                long long perm, run, end;
                if (!read_iv(in, v) || !(in >> perm >> run >> end)) return fail("short X line", line);
                if (v.chr != H.chr[i] || v.pos1 != H.p1[i] || v.pos2 != H.p2[i] || (uint8_t)v.strand != H.strand[i] || perm != H.perm[i] || run != H.run_p2[i] || end != H.ends[i])
                    return fail("sorted entry " + std::to_string(i) + " differs", line);
            }
        } else if (tag == "M") {
            size_t m;
            in >> m;
            const grc_idx X = H.idx();
            std::vector<grc_iv> got;
            for (uint32_t i = 0; i < X.n; ++i) {
                if (grc_run_starts(X, i)) { grc_iv v; std::memset(&v, 0, sizeof v); v.chr = X.chr[i]; v.pos1 = X.p1[i]; v.strand = (char)X.strand[i]; got.push_back(v); }
                got.back().pos2 = X.run_p2[i];
            }
            if (got.size() != m) return fail("merge gives " + std::to_string(got.size()) + " intervals", line);
            for (size_t i = 0; i < m; ++i) {
                grc_iv v;
                if (!read_iv(in, v)) return fail("short M line", line);
                if (v.chr != got[i].chr || v.pos1 != got[i].pos1 || v.pos2 != got[i].pos2 || v.strand != got[i].strand) return fail("merged interval " + std::to_string(i) + " differs", line);
            }
            ++n_merges;
        } else if (tag == "Q") {
            grc_iv q;
            unsigned flags;
            long long width;
            size_t k;
            if (!read_iv(in, q) || !(in >> flags >> width >> k)) return fail("short Q line", line);
            const grc_idx X = H.idx();
            const grc_cand C = grc_range(X, q);
            if (C.lo > C.hi || C.hi > X.n) return fail("candidate range outside the index", line);
            if (grc_count(X, q, flags, C) != k) return fail("count " + std::to_string(grc_count(X, q, flags, C)) + " differs", line);
            std::vector<int32_t> sid(k), c1(k), c2(k);          // exactly k
            if (grc_fill(X, q, flags, C.lo, C.hi, sid.data(), c1.data(), c2.data(), k) != k) return fail("fill's number differs", line);
            for (size_t j = 0; j < k; ++j) {
                long long s, a, b;
                if (!(in >> s >> a >> b)) return fail("short Q line", line);
                if (s != sid[j] || a != c1[j] || b != c2[j]) return fail("hit " + std::to_string(j) + " differs", line);
            }
            if (!(flags & GRC_CONTAINED) && (long long)grc_width(c1.data(), c2.data(), k) != width) return fail("width " + std::to_string(grc_width(c1.data(), c2.data(), k)) + " differs", line);
            ++n_queries;
        }
    }
    std::printf("grc_host_test OK: %ld sets, %ld merges, %ld queries\n", n_sets, n_merges, n_queries);
    return 0;
}
