// SeqLib::Pileup as a SeqLib user drives it, through the headers only (tests/test_cpp_pile.py).
//   pile_api_test errors                             what throws, with or without a GPU; without one also that adding is refused (no CPU fallback)
//   pile_api_test run <bam> <fa> <expect> <dir>      <expect>: lines "name n v0 v1 ..." written by Python from tests/pile_util.py: the window (tid beg end), its
//                                                    15 planes one behind the other with the default knobs and with a quality and a mapq floor, a narrower
//                                                    window, and the candidate sites (pos ref depth alt ins per site).  addReads(BamReader&) == an addRead loop
//                                                    over Next() == half of each; At; Sites against RefGenome; WriteSites to <dir>/sites.tsv (compared by Python);
//                                                    Clear
#include <cstdio>
#include <cstring>
#include <fstream>
#include <map>
#include <sstream>
#include <string>
#include <vector>
#include "SeqLib/BamReader.h"
#include "SeqLib/Pileup.h"
#include "SeqLib/RefGenome.h"

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
    try { Pileup bad{GenomicRegion()}; } catch (const std::invalid_argument &) { threw = true; }
    CHECK(threw);
    Pileup p{GenomicRegion(0, 10, 90)};
    BamReader closed;
    CHECK(throws_runtime([&] { p.addReads(closed); }, "the reader is not open"));
    CHECK(p.Counter("records_seen") == -1);
    HeaderSequenceVector hsv;
    hsv.push_back(HeaderSequence("a", 100)); hsv.push_back(HeaderSequence("b", 50));
    p.SetHeader(BamHeader(hsv));          // (without a GPU: a host-only object)
    CHECK(throws_runtime([&] { p.SetKnob("lds_window", 5000); }, "outside") && throws_runtime([&] { p.SetKnob("no such knob", 1); }, "unknown key"));
    CHECK(p.Counter("records_seen") == 0 && p.Counter("no such counter") == -1);
    RefGenome none;
    if (slx_device_count() <= 0) {
        CHECK(throws_runtime([&] { p.Counts(0); }, "no HIP device") && throws_runtime([&] { p.At(20); }, "no HIP device"));
        CHECK(throws_runtime([&] { p.Clear(); }, "no HIP device") && throws_runtime([&] { p.WriteSites("/dev/null"); }, "no HIP device"));
        std::printf("pile api errors OK (no GPU)\n");
    } else {
        CHECK(p.Counts(0) == std::vector<int32_t>(80, 0) && p.At(20)[0] == 0 && p.At(5)[3] == 0 && p.At(100)[14] == 0);
        CHECK(throws_runtime([&] { p.Counts(15); }, "plane") && throws_runtime([&] { p.WriteSites("/dev/null"); }, "no result"));
        threw = false;
        try { p.Sites(none, 1, 1, 0, 1); } catch (const std::invalid_argument &) { threw = true; }
        CHECK(threw);
        std::printf("pile api errors OK (GPU)\n");
    }
    return 0;
}

static int run(const char *bam, const char *fa, const char *expect, const std::string &dir)
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
    auto planes = [](Pileup &p) { std::vector<int64_t> all; for (int k = 0; k < SLX_PILE_PLANES; ++k) { const std::vector<int32_t> v = p.Counts(k); all.insert(all.end(), v.begin(), v.end()); } return all; };
    const GenomicRegion win((int32_t)E["window"][0], (int32_t)E["window"][1], (int32_t)E["window"][2]);
    BamReader rd;
    CHECK(rd.Open(bam));
    rd.SetBatchBytes(1);          // one BGZF member a batch: several batches
    Pileup a(win), b(win), h2(win);
    a.SetHeader(rd.Header()); h2.SetHeader(rd.Header());
    size_t n = 0;
    while (std::optional<BamRecord> r = rd.Next()) { a.addRead(*r); ++n; }
    rd.Reset();
    CHECK(b.addReads(rd) == n && n == (size_t)E["n_records"][0]);          // (b takes the reader's header)
    CHECK(planes(a) == E["planes"] && planes(b) == E["planes"]);
    CHECK(a.Counter("records_seen") == (int64_t)n && b.Counter("records_seen") == (int64_t)n);
    // a read taken by Next() is not handed over again by addReads: the two halves make the whole
    rd.Reset();
    for (size_t i = 0; i < n / 2; ++i) { std::optional<BamRecord> r = rd.Next(); CHECK(r); h2.addRead(*r); }
    CHECK(h2.addReads(rd) == n - n / 2 && planes(h2) == E["planes"]);
    const int64_t L = win.pos2 - win.pos1, at = E["at"][0];
    for (int k = 0; k < SLX_PILE_PLANES; ++k) CHECK(b.At(at)[(size_t)k] == E["planes"][(size_t)(k * L + at - win.pos1)]);
    CHECK(b.At(win.pos1 - 1)[0] == 0 && b.At(win.pos2)[0] == 0);
    // the floors
    Pileup f(win);
    f.SetMinBaseQuality(20); f.SetMinMapq(30);
    rd.Reset();
    CHECK(f.addReads(rd) == n && planes(f) == E["planes_floors"] && E["planes_floors"] != E["planes"]);
    f.SetExcludeFlags(0x704);
    // a narrower window
    Pileup w(GenomicRegion(win.chr, (int32_t)E["narrow"][0], (int32_t)E["narrow"][1]));
    rd.Reset();
    CHECK(w.addReads(rd) == n && planes(w) == E["planes_narrow"]);
    // the sites
    RefGenome ref;
    CHECK(ref.LoadIndex(fa));
    const std::vector<int64_t> &S = E["sites"], &Q = E["site_params"];
    const std::vector<PileupSite> got = b.Sites(ref, (int)Q[0], (int)Q[1], (int)Q[2], (int)Q[3]);
    CHECK(got.size() * 5 == S.size() && !got.empty());
    for (size_t i = 0; i < got.size(); ++i) {
        CHECK(got[i].pos == S[5 * i] && got[i].ref == (char)S[5 * i + 1] && got[i].depth == S[5 * i + 2] && got[i].alt == S[5 * i + 3] && got[i].ins == S[5 * i + 4]);
        for (int k = 0; k < SLX_PILE_PLANES; ++k) CHECK(got[i].plane[(size_t)k] == E["planes"][(size_t)(k * L + got[i].pos - win.pos1)]);
    }
    b.WriteSites(dir + "/sites.tsv");
    CHECK(b.Counter("sites") == (int64_t)got.size() && b.Sites(ref, 100000, 1, 0, 1).empty());
    b.Clear();
    CHECK(planes(b) == std::vector<int64_t>((size_t)(SLX_PILE_PLANES * L), 0) && b.Sites(ref, 1, 1, 0, 1).empty());
    std::printf("pile api OK\n");
    return 0;
}

int main(int argc, char **argv)
{
    try {
        if (argc == 2 && !std::strcmp(argv[1], "errors")) return errors();
        if (argc == 6 && !std::strcmp(argv[1], "run")) return run(argv[2], argv[3], argv[4], argv[5]);
    } catch (const std::exception &e) {
        std::printf("exception: %s\n", e.what());
        return 1;
    }
    return 2;
}
