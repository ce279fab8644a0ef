// SeqLib::GenomicRegion and GRC (include/SeqLib/GenomicRegion.h, GenomicRegionCollection.h) compiled with g++ through the headers only
// (tests/test_cpp_region.py): constructors and their exceptions, the samtools-style strings, GetOverlap's four answers, Pad, the ordering, the text
// forms, the container.  No GPU and no library call.
#include <cstdio>
#include <sstream>
#include <stdexcept>
#include <string>
#include "SeqLib/GenomicRegionCollection.h"

using namespace SeqLib;

static int fails = 0;
#define CHECK(x) do { if (!(x)) { std::printf("FAILED line %d: %s\n", __LINE__, #x); ++fails; } } while (0)
template <class E, class F> static bool throws(F f)
{
    try { f(); } catch (const E &) { return true; } catch (...) { return false; }
    return false;
}

int main()
{
    const BamHeader hdr(HeaderSequenceVector{HeaderSequence("chrA", 200000), HeaderSequence("chrB", 150000), HeaderSequence("HLA-A*01:01", 3000), HeaderSequence("7", 5000)});
    const BamHeader none;

    GenomicRegion e;
    CHECK(e.IsEmpty() && e.chr == -1 && e.pos1 == 0 && e.pos2 == 0 && e.strand == '*' && e.Width() == 1);
    GenomicRegion a(0, 100, 200);
    CHECK(!a.IsEmpty() && a.Width() == 101 && a.strand == '*' && GenomicRegion(1, 5, 5, '-').strand == '-');
    CHECK(throws<std::invalid_argument>([] { GenomicRegion(0, 200, 100); }));
    CHECK(throws<std::invalid_argument>([] { GenomicRegion(0, 100, 200, 'x'); }));

    // (chr, pos1, pos2) as strings
    GenomicRegion s1("chrB", "10", "20", hdr);
    CHECK(s1.chr == 1 && s1.pos1 == 10 && s1.pos2 == 20);
    CHECK(GenomicRegion("chr7", "1", "2", hdr).chr == -1 && GenomicRegion("7", "1", "2", hdr).chr == 3 && GenomicRegion("A", "1", "2", hdr).chr == -1);
    CHECK(GenomicRegion("chr2", "1", "2", none).chr == 1 && GenomicRegion("X", "1", "2", none).chr == 22 && GenomicRegion("chrY", "1", "2", none).chr == 23);
    CHECK(throws<std::invalid_argument>([&] { GenomicRegion("chrA", "ten", "20", hdr); }));
    CHECK(throws<std::out_of_range>([&] { GenomicRegion("chrA", "99999999999", "20", hdr); }));

    // samtools-style strings
    GenomicRegion w("chrA", hdr);
    CHECK(w.chr == 0 && w.pos1 == 1 && w.pos2 == 200000);
    GenomicRegion r("chrA:1,000-2,000", hdr);
    CHECK(r.chr == 0 && r.pos1 == 1000 && r.pos2 == 2000 && r.strand == '*');
    GenomicRegion r2("chrB:500", hdr);
    CHECK(r2.chr == 1 && r2.pos1 == 500 && r2.pos2 == 150000);
    GenomicRegion h1("HLA-A*01:01", hdr), h2("HLA-A*01:01:10-20", hdr);
    CHECK(h1.chr == 2 && h1.pos1 == 1 && h1.pos2 == 3000 && h2.chr == 2 && h2.pos1 == 10 && h2.pos2 == 20);
    CHECK(throws<std::invalid_argument>([&] { GenomicRegion("chrZ", hdr); }));
    CHECK(throws<std::invalid_argument>([&] { GenomicRegion("chrZ:1-100", hdr); }));
    CHECK(throws<std::invalid_argument>([&] { GenomicRegion("chrA:200-100", hdr); }));
    CHECK(throws<std::invalid_argument>([&] { GenomicRegion("", hdr); }));
    CHECK(throws<std::invalid_argument>([&] { GenomicRegion("chrA:1-100", none); }));

    // GetOverlap: 0 none, 1 partial, 2 the argument inside, 3 the argument around
    CHECK(a.GetOverlap(GenomicRegion(0, 201, 300)) == 0 && a.GetOverlap(GenomicRegion(1, 100, 200)) == 0 && a.GetOverlap(GenomicRegion(0, 0, 99)) == 0);
    CHECK(a.GetOverlap(GenomicRegion(0, 150, 300)) == 1 && a.GetOverlap(GenomicRegion(0, 0, 100)) == 1 && a.GetOverlap(GenomicRegion(0, 200, 201)) == 1);
    CHECK(a.GetOverlap(GenomicRegion(0, 120, 180)) == 2 && a.GetOverlap(GenomicRegion(0, 100, 199)) == 2);
    CHECK(a.GetOverlap(GenomicRegion(0, 50, 300)) == 3 && a.GetOverlap(a) == 3);

    // Pad
    GenomicRegion p(0, 100, 200);
    p.Pad(10);
    CHECK(p.pos1 == 90 && p.pos2 == 210);
    p.Pad(-60);
    CHECK(p.pos1 == 150 && p.pos2 == 150);
    CHECK(throws<std::out_of_range>([&] { p.Pad(-1); }));
    CHECK(p.pos1 == 150 && p.pos2 == 150);

    // the ordering: chr, pos1, pos2; the strand takes no part
    const GenomicRegion x(0, 100, 200), y(0, 100, 300), z(0, 101, 102), u(1, 0, 1);
    CHECK(x < y && y < z && z < u && !(y < x) && u > x && y > x && x <= y && x <= x && y >= x && x >= x && !(x > x) && !(x < x));
    CHECK(x == GenomicRegion(0, 100, 200, '-') && x != y && !(x != x));
    CHECK(x.DistanceBetweenStarts(z) == 1 && z.DistanceBetweenStarts(x) == 1 && x.DistanceBetweenEnds(y) == 100 && x.DistanceBetweenStarts(u) == -1 && x.DistanceBetweenEnds(u) == -1);

    // text
    const GenomicRegion t(1, 1234567, 2345678, '+');
    CHECK(t.ToString(hdr) == "chrB:1,234,567-2,345,678(+)" && t.PointString(hdr) == "chrB:1,234,567(+)" && t.ChrName(hdr) == "chrB" && t.ChrName(none) == "2");
    CHECK(GenomicRegion(22, 1, 999).ChrName(none) == "X" && GenomicRegion(0, 1000, 1000).ToString(hdr) == "chrA:1,000-1,000(*)");
    std::ostringstream os;
    os << t << " " << GenomicRegion(23, 5, 6);
    CHECK(os.str() == "2:1,234,567-2,345,678(+) Y:5-6(*)");
    CHECK(throws<std::invalid_argument>([&] { GenomicRegion(9, 1, 2).ChrName(hdr); }));

    // the container
    GRC g;
    CHECK(g.size() == 0 && g.IsEmpty() && g.begin() == g.end());
    g.add(u); g.add(x); g.add(r);
    CHECK(g.size() == 3 && g[0] == u && g.at(2) == r && !g.IsEmpty());
    int n = 0;
    for (const GenomicRegion &q : g) n += q.Width();
    CHECK(n == 2 + 101 + 1001);
    CHECK(throws<std::out_of_range>([&] { g.at(3); }));
    g.clear();
    CHECK(g.size() == 0);

    if (fails) std::printf("genomic_region FAILED (%d)\n", fails);
    else std::printf("genomic_region OK\n");
    return fails ? 1 : 0;
}
