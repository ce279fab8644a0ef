// SeqLib::GenomicRegionCollection (include/SeqLib/GenomicRegionCollection.h) through the headers and the C-ABI, compiled with g++ -Wall -Werror -DSEQLIB_GRC_QUERIES
// (tests/test_cpp_grc.py, tests/test_gpu_grc.py).
//   grc_api_test host DIR                     everything that needs no GPU: the reference's `merge` and `interval_queries` (part 1) shapes of seq_test.cpp, the
//                                             host-only members, ReadBED / ReadVCF on files written into DIR, the single queries, the exceptions
//   grc_api_test nogpu                        the collection join without a GPU: std::runtime_error
//   grc_api_test gpu BAM N SUBJECTS TOTAL     the collection join and Intersection against the single-query path, `interval_queries` part 2, and OverlapReads /
//                                             CountReads over BAM (N records; SUBJECTS: lines of chr pos1 pos2; TOTAL: the sum of the per-subject counts)
#include <cstdio>
#include <cstdlib>
#include <fstream>
#include <iostream>
#include <sstream>
#include <string>
#include <vector>
#include <zlib.h>
#include "SeqLib/BamReader.h"
#include "SeqLib/GenomicRegionCollection.h"

using namespace SeqLib;

#define CHECK(x) do { if (!(x)) { std::fprintf(stderr, "grc_api_test: %s:%d: CHECK(%s) failed\n", __FILE__, __LINE__, #x); std::exit(1); } } while (0)
template <class E, class F> static bool throws(F f) { try { f(); } catch (const E &) { return true; } catch (...) { return false; } return false; }

static GRC random_collection(unsigned seed, int n)
{
    GRC g;
    std::srand(seed);
    for (int i = 0; i < n; ++i) {
        const int p = std::rand() % 100000;
        g.add(GenomicRegion(std::rand() % 3, p, p + std::rand() % 400, "+-*"[std::rand() % 3]));
    }
    return g;
}

static void write_file(const std::string &path, const std::string &text, bool gz)
{
    if (gz) {
        gzFile f = gzopen(path.c_str(), "w");
        CHECK(f && gzwrite(f, text.data(), (unsigned)text.size()) == (int)text.size());
        gzclose(f);
    } else {
        std::ofstream(path) << text;
    }
}

static int host(const std::string &dir)
{
    // ---- seq_test.cpp `merge`
    {
        GRC grc;
        grc.add(GenomicRegion(23, 10, 100)); grc.add(GenomicRegion(23, 20, 110)); grc.add(GenomicRegion(2, 10, 100)); grc.add(GenomicRegion(2, 20, 110)); grc.add(GenomicRegion(2, 200, 310));
        grc.MergeOverlappingIntervals();
        CHECK(grc.size() == 3 && grc[0].chr == 2 && grc[1].chr == 2 && grc[2].chr == 23 && grc[2].pos2 == 110 && grc[2].pos1 == 10);
        CHECK(grc[0].pos1 == 10 && grc[0].pos2 == 110 && grc[1].pos1 == 200 && grc[1].pos2 == 310);
        grc.MergeOverlappingIntervals();          // again: nothing changes
        CHECK(grc.size() == 3 && grc[2].pos2 == 110);
    }
    // touching merges, adjacent does not; the first member's strand
    {
        GRC g;
        g.add(GenomicRegion(0, 6, 8, '+')); g.add(GenomicRegion(0, 4, 6, '-')); g.add(GenomicRegion(1, 4, 5)); g.add(GenomicRegion(1, 6, 7));
        g.MergeOverlappingIntervals();
        CHECK(g.size() == 3 && g[0].pos1 == 4 && g[0].pos2 == 8 && g[0].strand == '-' && g[1].pos2 == 5 && g[2].pos1 == 6);
        GRC e;
        e.MergeOverlappingIntervals();
        CHECK(e.size() == 0);
    }
    // ---- seq_test.cpp `interval_queries`, part 1
    {
        GRC grc = random_collection(42, 500);
        grc.MergeOverlappingIntervals();
        grc.add(GenomicRegion(23, 10, 100));
        grc.add(GenomicRegion(23, 20, 110));
        CHECK(throws<std::logic_error>([&] { grc.FindOverlaps(GenomicRegion(23, 10, 100), true); }));          // no tree yet
        CHECK(throws<std::logic_error>([&] { grc.FindOverlappedIntervals(GenomicRegion(23, 10, 100), true); }));
        CHECK(throws<std::logic_error>([&] { grc.FindOverlapWidth(GenomicRegion(23, 10, 100), true); }));
        CHECK(grc.CountOverlaps(GenomicRegion(23, 10, 100)) == 0 && grc.NumTree() == 0);          // (a warning on stderr)
        grc.CreateTreeMap();
        CHECK(grc.NumTree() == 4);
        GRC results = grc.FindOverlaps(GenomicRegion(23, 10, 100), true);
        CHECK(results.size() == 2 && results[1].pos2 == 100 && results[0].pos1 == 10 && results[1].pos1 == 20 && results[0].chr == 23);
        const std::vector<int> ids = grc.FindOverlappedIntervals(GenomicRegion(23, 10, 100), true);
        CHECK(ids.size() == 2 && ids[0] == (int)grc.size() - 2 && ids[1] == (int)grc.size() - 1);
        CHECK(grc.CountOverlaps(GenomicRegion(23, 10, 100)) == 2 && grc.CountOverlaps(GenomicRegion(24, 10, 100)) == 0);
        CHECK(throws<std::invalid_argument>([&] { GenomicRegion bad; bad.chr = 1; bad.pos1 = 9; bad.pos2 = 3; grc.FindOverlaps(bad, true); }));
        grc.clear();
        CHECK(grc.size() == 0 && grc.NumTree() == 0 && grc.FindOverlaps(GenomicRegion(23, 10, 100), true).size() == 0);
    }
    // nested intervals: CountContained, OverlapSameInterval, FindOverlapWidth, strands
    {
        GRC g;
        g.add(GenomicRegion(1, 100, 200, '+')); g.add(GenomicRegion(1, 120, 130, '-')); g.add(GenomicRegion(1, 125, 128, '+')); g.add(GenomicRegion(1, 300, 400)); g.add(GenomicRegion(2, 1, 5));
        g.CreateTreeMap();
        CHECK(g.CountContained(GenomicRegion(1, 110, 140)) == 2 && g.CountContained(GenomicRegion(1, 100, 400)) == 4 && g.CountContained(GenomicRegion(1, 126, 127)) == 0);
        CHECK(g.CountOverlaps(GenomicRegion(1, 126, 127)) == 3);
        CHECK(g.OverlapSameInterval(GenomicRegion(1, 101, 102), GenomicRegion(1, 190, 195)) && !g.OverlapSameInterval(GenomicRegion(1, 101, 102), GenomicRegion(1, 301, 302)));
        CHECK(!g.OverlapSameInterval(GenomicRegion(1, 101, 102), GenomicRegion(2, 1, 2)) && !g.OverlapSameInterval(GenomicRegion(1, 250, 260), GenomicRegion(1, 101, 102)));
        CHECK(g.OverlapSameInterval(GenomicRegion(1, 126, 126), GenomicRegion(1, 150, 350)));
        CHECK(g.FindOverlapWidth(GenomicRegion(1, 150, 350), true) == 51 + 51 && g.FindOverlapWidth(GenomicRegion(1, 90, 135), true) == 36 && g.FindOverlapWidth(GenomicRegion(3, 1, 2), true) == 0);
        CHECK(g.FindOverlapWidth(GenomicRegion(1, 90, 135, '-'), false) == 11 && g.FindOverlaps(GenomicRegion(1, 90, 135, '+'), false).size() == 2);
        const GRC clipped = g.FindOverlaps(GenomicRegion(1, 126, 350), true);
        CHECK(clipped.size() == 4 && clipped[0].pos1 == 126 && clipped[0].pos2 == 200 && clipped[2].pos2 == 128 && clipped[3].pos1 == 300 && clipped[3].pos2 == 350 && clipped[3].strand == '*');
        GRC copy = g;          // the copy shares the index
        CHECK(copy.CountOverlaps(GenomicRegion(2, 5, 9)) == 1 && copy.NumTree() == 2);
    }
    // add does not clear the sorted mark: CreateTreeMap then indexes the vector as it stands, ids are positions in it
    {
        GRC g(GenomicRegion(1, 50, 60));
        g.add(GenomicRegion(1, 10, 20));
        g.CreateTreeMap();
        CHECK(g[0].pos1 == 50 && g.FindOverlappedIntervals(GenomicRegion(1, 15, 15), true) == std::vector<int>({1}));
        GRC h;
        h.add(GenomicRegion(1, 50, 60)); h.add(GenomicRegion(1, 10, 20));
        h.CreateTreeMap();
        CHECK(h[0].pos1 == 10 && h.FindOverlappedIntervals(GenomicRegion(1, 15, 15), true) == std::vector<int>({0}));
    }
    // ---- the tiling constructors
    {
        CHECK(throws<std::invalid_argument>([] { GRC(10, 10, GenomicRegion(0, 0, 100)); }));
        GRC whole(200, 10, GenomicRegion(0, 0, 100));
        CHECK(whole.size() == 1 && whole[0].pos2 == 100);
        GRC t(40, 10, GenomicRegion(3, 0, 100));          // 0-40 30-70 60-100
        CHECK(t.size() == 3 && t[1].pos1 == 30 && t[1].pos2 == 70 && t[2].pos2 == 100 && t[2].chr == 3);
        GRC u(40, 10, GenomicRegion(3, 0, 95));          // ... and the final piece 60-95
        CHECK(u.size() == 3 && u[1].pos2 == 70 && u[2].pos1 == 60 && u[2].pos2 == 95);
        HeaderSequenceVector hs;
        hs.push_back(HeaderSequence("a", 100)); hs.push_back(HeaderSequence("b", 30));
        CHECK(throws<std::invalid_argument>([&] { GRC(5, 7, hs); }));
        GRC v(40, 10, hs);
        CHECK(v.size() == 4 && v[2].pos2 == 100 && v[3].chr == 1 && v[3].pos1 == 0 && v[3].pos2 == 30);
    }
    // ---- SortAndStretch*, Pad, Concat, TotalWidth, AsBEDString, operator<<, Shuffle, empty
    {
        GRC g;
        g.add(GenomicRegion(0, 50, 60)); g.add(GenomicRegion(0, 10, 20)); g.add(GenomicRegion(0, 30, 35));
        GRC r = g;
        r.SortAndStretchRight(100);
        CHECK(r[0].pos1 == 10 && r[0].pos2 == 29 && r[1].pos2 == 49 && r[2].pos2 == 100);
        r = g; r.SortAndStretchRight(0);
        CHECK(r[2].pos2 == 60);
        CHECK(throws<std::out_of_range>([&] { GRC x = g; x.SortAndStretchRight(55); }));
        GRC l = g;
        l.SortAndStretchLeft(15);          // the reference's check as it is written: a min past the first start is taken, one before it throws
        CHECK(l[0].pos1 == 15 && l[1].pos1 == 21 && l[2].pos1 == 36);
        l = g; l.SortAndStretchLeft(-1);
        CHECK(l[0].pos1 == 10 && l[1].pos1 == 21);
        CHECK(throws<std::out_of_range>([&] { GRC x = g; x.SortAndStretchLeft(5); }));
        CHECK(g.TotalWidth() == 11 + 11 + 6);
        GRC p = g;
        p.Pad(2);
        CHECK(p[0].pos1 == 48 && p[0].pos2 == 62 && p.TotalWidth() == 28 + 12);
        CHECK(throws<std::out_of_range>([&] { GRC x = g; x.Pad(-4); }));
        GRC c = g, none;
        c.Concat(none); c.Concat(g);
        CHECK(c.size() == 6 && c[3].pos1 == 50 && !c.empty() && none.empty());
        const BamHeader hdr(HeaderSequenceVector({HeaderSequence("chrA", 1000), HeaderSequence("chrB", 500)}));
        CHECK(g.AsBEDString(hdr) == "chrA\t50\t60\t*\nchrA\t10\t20\t*\nchrA\t30\t35\t*\n" && none.AsBEDString(hdr).empty());
        std::ostringstream os;
        os << c << "|" << none;
        CHECK(os.str().find("GenomicRegionCollection(size=6) [1:50-60(*), 1:10-20(*), 1:30-35(*), 1:50-60(*), 1:10-20(*), 1:30-35(*)]|GenomicRegionCollection(size=0)") == 0);
        GRC big = random_collection(1, 50);
        std::ostringstream ob;
        ob << big;
        CHECK(ob.str().find(", ... ") != std::string::npos);
        big.Shuffle(); big.Rewind();
        CHECK(big.size() == 50);
    }
    // ---- ReadBED / ReadVCF, plain and gzip'd
    {
        const BamHeader hdr(HeaderSequenceVector({HeaderSequence("chrA", 1000), HeaderSequence("chrB", 500)}));
        const std::string bed = "# a comment\nchrA\t10\t20\tname\nchrB\t5\t9\ntrack name=x # inline\nchrZ\t1\t2\n\nchrA\t30\t40\n";
        const std::string vcf = "##fileformat=VCFv4.2\n#CHROM\tPOS\nchrA\t15\t.\tA\tT\nchrZ\t3\t.\tA\tT\nchrB\t7\t.\tG\tC # kept\n";
        for (int gz = 0; gz < 2; ++gz) {
            const std::string pb = dir + (gz ? "/t.bed.gz" : "/t.bed"), pv = dir + (gz ? "/t.vcf.gz" : "/t.vcf");
            write_file(pb, bed, gz != 0); write_file(pv, vcf, gz != 0);
            GRC b;
            CHECK(b.ReadBED(pb, hdr) && b.size() == 3 && b[0].chr == 0 && b[0].pos1 == 10 && b[0].pos2 == 20 && b[1].chr == 1 && b[2].pos2 == 40);
            GRC v;
            CHECK(v.ReadVCF(pv, hdr) && v.size() == 2 && v[0].pos1 == 15 && v[0].pos2 == 15 && v[1].chr == 1 && v[1].pos1 == 7);
            GRC fb(pb, hdr), fv(pv, hdr);          // the constructor's dispatch on the name
            CHECK(fb.size() == 3 && fv.size() == 2);
        }
        GRC one("chrB:100-200", hdr);
        CHECK(one.size() == 1 && one[0].chr == 1 && one[0].pos1 == 100 && one[0].pos2 == 200);
        GRC none;
        CHECK(!none.ReadBED(dir + "/missing.bed", hdr) && !none.ReadVCF("", hdr) && none.size() == 0);
    }
    // the BamRecordVector constructor
    {
        BamRecordVector brv;
        GRC g(brv);
        CHECK(g.size() == 0);
    }
    std::printf("grc_api_test host OK\n");
    return 0;
}

static int nogpu()
{
    GRC a = random_collection(3, 40), b = random_collection(4, 30);
    a.CreateTreeMap(); b.CreateTreeMap();
    std::vector<int32_t> q, s;
    CHECK(throws<std::runtime_error>([&] { a.FindOverlaps(b, q, s, true); }));
    CHECK(throws<std::runtime_error>([&] { a.Intersection(b, true); }));
    CHECK(throws<std::runtime_error>([&] { a.SubjectCounts(); }));
    GRC c = random_collection(5, 10);          // no tree: a warning and nothing
    CHECK(a.FindOverlaps(c, q, s, true).size() == 0 && q.empty());
    std::printf("grc_api_test nogpu OK\n");
    return 0;
}

// the join a.FindOverlaps(b, ...) against the single-query path looped over a's intervals
static void same_as_single_queries(const GRC &a, const GRC &b, bool ignore_strand)
{
    std::vector<int32_t> q, s;
    const GRC out = a.FindOverlaps(b, q, s, ignore_strand);
    size_t k = 0;
    for (size_t i = 0; i < a.size(); ++i) {
        const std::vector<int> ids = b.FindOverlappedIntervals(a[i], ignore_strand);
        const GRC one = b.FindOverlaps(a[i], ignore_strand);
        CHECK(ids.size() == one.size());
        for (size_t j = 0; j < ids.size(); ++j, ++k) {
            CHECK(k < q.size() && q[k] == (int32_t)i && s[k] == ids[j]);
            CHECK(out[k].chr == one[j].chr && out[k].pos1 == one[j].pos1 && out[k].pos2 == one[j].pos2);
        }
    }
    CHECK(k == q.size() && k == s.size() && k == out.size() && k > 0);
}

static int gpu(const std::string &bam, size_t n_records, const std::string &subjects, long long total)
{
    GRC a = random_collection(7, 700), b = random_collection(8, 300);
    a.CreateTreeMap(); b.CreateTreeMap();
    for (int ig = 0; ig < 2; ++ig) { same_as_single_queries(a, b, ig != 0); same_as_single_queries(b, a, ig != 0); }
    std::vector<int32_t> q, s;
    CHECK(a.Intersection(b, true).size() == b.FindOverlaps(a, q, s, true).size() && q.size() == s.size() && !q.empty());
    q.clear(); s.clear();
    CHECK(b.Intersection(a, true).size() == a.Intersection(b, true).size());
    // ---- seq_test.cpp `interval_queries`, part 2: a merged collection against itself
    GRC grc = random_collection(42, 500);
    grc.MergeOverlappingIntervals();
    grc.add(GenomicRegion(23, 10, 100)); grc.add(GenomicRegion(23, 20, 110));
    grc.MergeOverlappingIntervals();
    grc.CreateTreeMap();
    const GRC self = grc.FindOverlaps(grc, q, s, true);
    CHECK(self.size() == grc.size() && self.TotalWidth() == grc.TotalWidth() && q == s);
    // ---- records of a reader against a collection
    GRC subj;
    std::ifstream f(subjects);
    int c, p1, p2;
    while (f >> c >> p1 >> p2) subj.add(GenomicRegion(c, p1, p2));
    CHECK(subj.size() > 5);
    subj.CreateTreeMap();
    BamReader rd;
    CHECK(rd.Open(bam));
    std::vector<int64_t> read_id;
    std::vector<int32_t> subject_id;
    GRC clipped;
    CHECK(subj.OverlapReads(rd, read_id, subject_id, &clipped) == n_records);
    CHECK((long long)read_id.size() == total && clipped.size() == read_id.size() && subject_id.size() == read_id.size());
    std::vector<int64_t> counts = subj.SubjectCounts(), by_pair(subj.size(), 0);
    for (int32_t x : subject_id) by_pair[(size_t)x]++;
    CHECK(counts == by_pair);
    for (size_t k = 1; k < read_id.size(); ++k) CHECK(read_id[k - 1] <= read_id[k]);
    for (size_t k = 0; k < clipped.size(); ++k) CHECK(clipped[k].chr == subj[(size_t)subject_id[k]].chr && clipped[k].pos1 >= subj[(size_t)subject_id[k]].pos1 && clipped[k].pos2 <= subj[(size_t)subject_id[k]].pos2);
    rd.Reset();
    CHECK(subj.CountReads(rd) == n_records);
    counts = subj.SubjectCounts();
    for (size_t i = 0; i < counts.size(); ++i) CHECK(counts[i] == 2 * by_pair[i]);
    subj.ClearCounts();
    CHECK(subj.SubjectCounts() == std::vector<int64_t>(subj.size(), 0) && subj.Counter("records") == (int64_t)(2 * n_records));
    // a batch of the C-ABI handed over directly
    slx_bam *raw = nullptr;
    CHECK(slx_bam_open(bam.c_str(), -1, &raw) == SLX_OK);
    slx_bam_batch batch;
    std::vector<int64_t> rid2;
    std::vector<int32_t> sid2;
    int64_t seen = 0;
    while (slx_bam_next(raw, 4000, &batch) == SLX_OK && batch.n_records) seen += (int64_t)subj.OverlapBatch(batch, &rid2, &sid2, nullptr, seen);
    slx_bam_close(raw);
    CHECK(seen == (int64_t)n_records && rid2 == read_id && sid2 == subject_id && subj.SubjectCounts() == by_pair);
    std::printf("grc_api_test gpu OK\n");
    return 0;
}

int main(int argc, char **argv)
{
    const std::string mode = argc > 1 ? argv[1] : "";
    try {
        if (mode == "host" && argc == 3) return host(argv[2]);
        if (mode == "nogpu") return nogpu();
        if (mode == "gpu" && argc == 6) return gpu(argv[2], (size_t)std::atoll(argv[3]), argv[4], std::atoll(argv[5]));
    } catch (const std::exception &e) {
        std::fprintf(stderr, "grc_api_test: exception: %s\n", e.what());
        return 1;
    }
    std::fprintf(stderr, "usage: grc_api_test host DIR | nogpu | gpu BAM N SUBJECTS TOTAL\n");
    return 2;
}
