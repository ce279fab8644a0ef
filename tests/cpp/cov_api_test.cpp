// SeqLib::STCoverage as a SeqLib user drives it, through the headers only (tests/test_cpp_cov.py).
//   cov_api_test errors                       what throws, with or without a GPU; without one also that adding is refused (no CPU fallback)
//   cov_api_test run <bam> <expect> <dir>     <expect>: lines "name n v0 v1 ..." written by Python from tests/cov_util.py.  For SPAN (buff 0 and 3) and FULL: an addRead
//                                             loop over Next() == addReads(BamReader&) == the expected depth of contig 2; maxCov; getCoverageAtPosition inside and
//                                             outside; ToBedgraph in both forms (<dir>/*.bg, compared by Python); the window constructor; SetMode(ALIGNED) with
//                                             samtools' flags; RegionSums
#include <cstdio>
#include <cstring>
#include <fstream>
#include <map>
#include <sstream>
#include <string>
#include <vector>
#include "SeqLib/BamReader.h"
#include "SeqLib/STCoverage.h"

using namespace SeqLib;
#define CHECK(x) do { if (!(x)) { std::printf("FAILED line %d: %s\n", __LINE__, #x); return 1; } } while (0)

template <class F> static bool throws_runtime(F f, const char *what)
{
    try { f(); } catch (const std::runtime_error &e) { return std::strstr(e.what(), what) != nullptr; } catch (...) { return false; }
    return false;
}

static int errors()
{
    bool threw = false;
    try { STCoverage bad{GenomicRegion()}; } catch (const std::invalid_argument &) { threw = true; }
    CHECK(threw);
    STCoverage none;
    BamReader closed;
    CHECK(throws_runtime([&] { none.maxCov(); }, "SetHeader() before the first read"));
    CHECK(throws_runtime([&] { none.addReads(closed, 0, false); }, "the reader is not open"));
    CHECK(none.Counter("records_seen") == -1);
    HeaderSequenceVector hsv;
    hsv.push_back(HeaderSequence("a", 100)); hsv.push_back(HeaderSequence("b", 50));
    STCoverage c;
    c.SetHeader(BamHeader(hsv));          // (without a GPU: a host-only object)
    CHECK(throws_runtime([&] { c.SetKnob("mode", 7); }, "outside") && throws_runtime([&] { c.SetKnob("no such knob", 1); }, "unknown key"));
    CHECK(c.Counter("records_seen") == 0 && c.Counter("no such counter") == -1);
    if (slx_device_count() <= 0) {
        CHECK(throws_runtime([&] { c.maxCov(); }, "no HIP device") && throws_runtime([&] { c.getCoverageAtPosition(0, 5); }, "no HIP device"));
        CHECK(throws_runtime([&] { c.clear(); }, "no HIP device") && throws_runtime([&] { c.ToBedgraph("/dev/null"); }, "no HIP device"));
        std::printf("cov api errors OK (no GPU)\n");
    } else {
        CHECK(c.maxCov() == 0 && c.getCoverageAtPosition(0, 5) == 0 && c.getCoverageAtPosition(7, 5) == 0 && c.getCoverageAtPosition(0, -1) == 0 && c.getCoverageAtPosition(0, 100) == 0);
        std::printf("cov api errors OK (GPU)\n");
    }
    return 0;
}

static int run(const char *bam, const char *expect, const std::string &dir)
{
    std::map<std::string, std::vector<int64_t>> E;
    {
        std::ifstream f(expect);
        std::string line;
        while (std::getline(f, line)) {
            std::istringstream in(line);
            std::string name; size_t n;
            in >> name >> n;
            std::vector<int64_t> v(n);
            for (auto &x : v) in >> x;
            E[name] = v;
        }
    }
    auto same = [](const std::vector<int32_t> &a, const std::vector<int64_t> &b) { if (a.size() != b.size()) return false; for (size_t i = 0; i < a.size(); ++i) if (a[i] != b[i]) return false; return true; };
    BamReader rd;
    CHECK(rd.Open(bam));
    rd.SetBatchBytes(1);          // one BGZF member a batch: several batches
    const struct { const char *name; int buff; bool full; } cfg[3] = {{"span0", 0, false}, {"span3", 3, false}, {"full", 0, true}};
    for (const auto &c : cfg) {
        const std::vector<int64_t> &want = E[std::string(c.name) + "_depth2"];
        CHECK(want.size() == 5000);
        STCoverage a, b;
        a.SetHeader(rd.Header());
        rd.Reset();
        size_t n = 0;
        while (std::optional<BamRecord> r = rd.Next()) { a.addRead(*r, c.buff, c.full); ++n; }
        rd.Reset();
        CHECK(b.addReads(rd, c.buff, c.full) == n && n == (size_t)E["n_records"][0]);
        CHECK(same(a.Depth(2, 0, 5000), want) && same(b.Depth(2, 0, 5000), want));
        CHECK(a.Counter("records_seen") == (int64_t)n && b.Counter("records_seen") == (int64_t)n);
        const int mx = (int)E[std::string(c.name) + "_max"][0];
        CHECK(a.maxCov() == mx && b.maxCov() == mx);
        CHECK(b.getCoverageAtPosition(2, 4999) == want[4999] && b.getCoverageAtPosition(2, 105) == want[105] && b.getCoverageAtPosition(2, 5000) == 0 && b.getCoverageAtPosition(2, -1) == 0 &&
              b.getCoverageAtPosition(99, 5) == 0 && b.getCoverageAtPosition(-1, 5) == 0);
        // a read taken by Next() is not handed over again by addReads: the two halves make the whole
        rd.Reset();
        STCoverage h2;
        h2.SetHeader(rd.Header());
        for (size_t i = 0; i < n / 2; ++i) { std::optional<BamRecord> r = rd.Next(); CHECK(r); h2.addRead(*r, c.buff, c.full); }
        CHECK(h2.addReads(rd, c.buff, c.full) == n - n / 2 && same(h2.Depth(2, 0, 5000), want));
        std::ofstream o(dir + "/" + c.name + "_stream.bg", std::ios::binary);
        a.ToBedgraph(&o, rd.Header());
        o.close();
        b.ToBedgraph(dir + "/" + c.name + "_path.bg");
        b.ToBedgraph(dir + "/" + c.name + "_zero.bg", true);
        b.settleCoverage();
        b.clear();
        CHECK(b.maxCov() == 0);
        // the window constructor: [100, 300) of contig 2
        STCoverage w{GenomicRegion(2, 100, 300)};
        rd.Reset();
        CHECK(w.addReads(rd, c.buff, c.full) == n);
        CHECK(same(w.Depth(2, 100, 300), std::vector<int64_t>(want.begin() + 100, want.begin() + 300)) && same(w.Depth(2, 0, 100), std::vector<int64_t>(100, 0)));
        CHECK(same(w.Depth(2, 290, 310), E[std::string(c.name) + "_win_290_310"]) && w.getCoverageAtPosition(2, 99) == 0 && w.getCoverageAtPosition(2, 100) == want[100]);
    }
    // what samtools depth counts
    STCoverage s;
    s.SetMode(SLX_COV_ALIGNED);
    s.SetExcludeFlags(0x704);
    s.SetMinMapq(4);
    rd.Reset();
    s.addReads(rd, 0, false);
    CHECK(same(s.Depth(2, 0, 5000), E["aligned_depth2"]));
    s.clear();
    s.SetCountDeletions(true);
    rd.Reset();
    s.addReads(rd, 0, false);
    CHECK(same(s.Depth(2, 0, 5000), E["aligned_del_depth2"]));
    GRC grc;
    grc.add(GenomicRegion(2, 0, 5000)); grc.add(GenomicRegion(2, 700, 730)); grc.add(GenomicRegion(1, 10, 10)); grc.add(GenomicRegion(3, 9999000, 10000001));
    std::vector<int64_t> sum, cnt;
    s.RegionSums(grc, 2, sum, cnt);
    CHECK(sum == E["region_sum"] && cnt == E["region_cnt"]);
    std::printf("cov api OK\n");
    return 0;
}

int main(int argc, char **argv)
{
    try {
        if (argc == 2 && !std::strcmp(argv[1], "errors")) return errors();
        if (argc == 5 && !std::strcmp(argv[1], "run")) return run(argv[2], argv[3], argv[4]);
    } catch (const std::exception &e) {
        std::printf("exception: %s\n", e.what());
        return 1;
    }
    return 2;
}
