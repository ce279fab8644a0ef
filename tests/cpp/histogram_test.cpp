// SeqLib::Histogram and SeqLib::Bin through the header only; links nothing (tests/test_stats_host.py).
//   histogram_test self                          the constructor's argument check, the last bin, values outside, removeElem, Bin's operators, toFileString
//   histogram_test bins <start> <end> <width> [values...]   prints "first second count" per bin, then "below above", then toFileString, after adding the values
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <sstream>
#include <string>
#include "SeqLib/Histogram.h"

using namespace SeqLib;
#define CHECK(x) do { if (!(x)) { std::printf("FAILED line %d: %s\n", __LINE__, #x); return 1; } } while (0)

static bool throws(int32_t s, int32_t e, uint32_t w)
{
    try { Histogram h(s, e, w); } catch (const std::invalid_argument &) { return true; }
    return false;
}

static int self()
{
    CHECK(throws(5, 5, 1) && throws(5, 4, 1) && throws(0, 10, 0) && !throws(0, 100, 1) && !throws(-2, 2000, 10));          // the reference throws for the valid ones
    Histogram h(-2, 2000, 10);
    CHECK(h.numBins() == 201 && h.m_bins.front().First() == -2 && h.m_bins.front().Second() == 7 && h.m_bins.back().First() == 1998 && h.m_bins.back().Second() == 2000);
    CHECK(h.retrieveBinID(-2) == 0 && h.retrieveBinID(7) == 0 && h.retrieveBinID(8) == 1 && h.retrieveBinID(1997) == 199 && h.retrieveBinID(1998) == 200 && h.retrieveBinID(2000) == 200);
    CHECK(h.retrieveBinID(-3) == Histogram::npos && h.retrieveBinID(2001) == Histogram::npos);
    CHECK(h.toFileString().empty() && h.totalCount() == 0);
    h.addElem(2000); h.addElem(1998); h.addElem(-2); h.addElem(2001); h.addElem(-3); h.addElem(300);          // a 300 bp read exits the reference's len histogram
    CHECK(h.binCount(200) == 2 && h.binCount(0) == 1 && h.NumBelow() == 1 && h.NumAbove() == 1 && h.totalCount() == 4);
    CHECK(h.toFileString() == "-2_7_1,298_307_1,1998_2000_2");
    h.removeElem(2000); h.removeElem(2001); h.removeElem(-3); h.removeElem(-3);
    CHECK(h.binCount(200) == 1 && h.NumAbove() == 0 && h.NumBelow() == 0);
    h.addCount((int64_t)1 << 31, 5); h.addToBin(3, 2); h.addOutside(1, 0);
    CHECK(h.NumAbove() == 5 && h.binCount(3) == 2 && h.NumBelow() == 1);
    Histogram c(0, 100, 5);
    CHECK(c.numBins() == 21 && c.m_bins.back().First() == 100 && c.m_bins.back().Second() == 100 && c.retrieveBinID(99) == 19 && c.retrieveBinID(100) == 20);
    Bin a, b;
    CHECK(a.getCount() == 0 && a.contains(0) && a.contains(1) && !a.contains(2) && !a.contains(-1) && !(a < b) && !(b < a));
    ++a; ++a; --a;
    CHECK(a.getCount() == 1);
    --a; --a;
    CHECK(a.getCount() == 0);
    CHECK(c.m_bins[0] < c.m_bins[1] && !(c.m_bins[1] < c.m_bins[0]));
    std::ostringstream o;
    o << c.m_bins[1];
    CHECK(o.str() == "5,9,0");
    Histogram none;
    CHECK(none.numBins() == 0 && none.retrieveBinID(0) == Histogram::npos && none.toFileString().empty());
    std::printf("histogram self OK\n");
    return 0;
}

int main(int argc, char **argv)
{
    if (argc == 2 && !std::strcmp(argv[1], "self")) return self();
    if (argc >= 5 && !std::strcmp(argv[1], "bins")) {
        Histogram h(std::atoi(argv[2]), std::atoi(argv[3]), (uint32_t)std::atoi(argv[4]));
        for (int i = 5; i < argc; ++i) h.addElem(std::atoi(argv[i]));
        for (const Bin &b : h.m_bins) std::printf("%d %d %llu\n", b.First(), b.Second(), (unsigned long long)b.getCount());
        std::printf("%llu %llu\n%s\n", (unsigned long long)h.NumBelow(), (unsigned long long)h.NumAbove(), h.toFileString().c_str());
        return 0;
    }
    return 2;
}
