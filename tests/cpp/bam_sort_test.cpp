// BamWriter::SortByCoordinate, the WriteDevice overload with offsets, alignToBam into a sorting writer and the BamRecordSort functors, compiled with g++
// through the headers only and driven as a SeqLib user drives them (tests/test_cpp_sort.py).
//   bam_sort_test <index prefix> <reads.fq> <n reads> <directory to write into>
// The reads go through alignToBam twice from srand48(4242): into a plain UseGpu() writer and into one with SortByCoordinate().  Read back, the sorted file's
// records are the plain file's under std::stable_sort by ((uint32)tid, pos), byte for byte.  stdout: "sort OK <records> <records of the region>".
#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>
#include "SeqLib/BWAAligner.h"
#include "SeqLib/BamReader.h"
#include "SeqLib/BamWriter.h"
#include "SeqLib/FastqReader.h"

using namespace SeqLib;

static int fails = 0;
#define CHECK(x) do { if (!(x)) { std::printf("FAILED line %d: %s\n", __LINE__, #x); ++fails; } } while (0)

// everything of a record that reaches the file, but the bin (computed by the writer from the fields below)
static std::string image(const BamRecord &r)
{
    const bam1_t *b = r.raw();
    const bam1_core_t &c = b->core;
    const int64_t f[10] = {c.tid, (int64_t)c.pos, c.qual, c.flag, (int64_t)c.n_cigar, c.l_qseq, c.mtid, (int64_t)c.mpos, (int64_t)c.isize, c.l_qname};
    std::string s((const char *)f, sizeof f);
    s.append((const char *)b->data, (size_t)b->l_data);
    return s;
}

static bool read_all(const std::string &path, BamRecordPtrVector &out, std::string *text = nullptr)
{
    BamReader r;
    if (!r.Open(path)) return false;
    if (text) *text = r.Header().AsString();
    for (;;) {
        BamRecordPtrVector v;
        if (!r.NextBatch(v, 100000)) break;
        out.insert(out.end(), v.begin(), v.end());
    }
    return true;
}

static bool by_coordinate(const BamRecordPtr &a, const BamRecordPtr &b)
{
    if ((uint32_t)a->ChrID() != (uint32_t)b->ChrID()) return (uint32_t)a->ChrID() < (uint32_t)b->ChrID();
    return a->Position() < b->Position();
}

static bool same(const BamRecordPtrVector &a, const BamRecordPtrVector &b)
{
    if (a.size() != b.size()) return false;
    for (size_t i = 0; i < a.size(); ++i) if (image(*a[i]) != image(*b[i])) { std::printf("record %zu differs\n", i); return false; }
    return true;
}

static BamRecord placed(int32_t tid, int32_t pos, int32_t mtid = -1, int32_t mpos = -1)
{
    BamRecord r;
    bam1_t *b = r.raw();
    b->core.tid = tid; b->core.pos = pos; b->core.mtid = mtid; b->core.mpos = mpos;
    return r;
}

int main(int argc, char **argv)
{
    if (argc < 5) return 2;
    const std::string fq = argv[2], dir = argv[4];
    const size_t n_reads = (size_t)std::atoll(argv[3]);
    try {
        BWAIndexPtr idx = std::make_shared<BWAIndex>();
        idx->LoadIndex(argv[1]);
        BWAAligner al(idx);
        UnalignedSequenceVector reads;
        {
            FastqReader f(fq);
            UnalignedSequence s;
            while (reads.size() < n_reads && f.GetNextSequence(s)) reads.push_back(s);
        }
        CHECK(reads.size() == n_reads);
        const std::string f_plain = dir + "/plain.bam", f_sorted = dir + "/sorted.bam", f_host = dir + "/host_sorted.bam";

        // ---- the refusals of SortByCoordinate mirror UseGpu's
        {
            BamWriter sam(SAM), host, open_one;
            CHECK(!sam.SortByCoordinate());                                  // not BAM
            CHECK(!host.SortByCoordinate());                                 // UseGpu() was not called: no host fallback
            open_one.SetHeader(idx->HeaderFromIndex());
            CHECK(open_one.UseGpu() && open_one.Open(dir + "/open.bam") && !open_one.SortByCoordinate());          // after Open()
            CHECK(!open_one.IsSorting() && open_one.WriteHeader() && open_one.Close());
        }

        // ---- alignToBam twice from the same lrand48 state
        size_t n_plain = 0, n_sorted = 0;
        {
            BamWriter w;
            w.SetHeader(idx->HeaderFromIndex());
            CHECK(w.UseGpu() && w.Open(f_plain) && w.WriteHeader());
            srand48(4242);
            n_plain = al.alignToBam(reads, w, false, 0.9, 10);
            CHECK(w.Close());
            CHECK(!w.BuildIndex());                                          // read order: the index build refuses it
        }
        {
            BamWriter w;
            w.SetHeader(idx->HeaderFromIndex());
            CHECK(w.UseGpu() && w.SortByCoordinate() && w.Open(f_sorted) && w.IsSorting() && w.WriteHeader());
            const char dummy[4] = {0, 0, 0, 0};
            CHECK(!w.WriteDevice(dummy, 4));                                 // a sorting writer needs the offsets
            srand48(4242);
            n_sorted = al.alignToBam(reads, w, false, 0.9, 10);
            CHECK(w.SortCounter("held_records") == (int64_t)n_sorted);
            CHECK(w.Close());
            CHECK(w.BuildIndex());
        }
        CHECK(n_plain == n_sorted && n_plain >= n_reads / 2);
        BamRecordPtrVector plain, sorted;
        std::string text_plain, text_sorted;
        CHECK(read_all(f_plain, plain, &text_plain) && read_all(f_sorted, sorted, &text_sorted));
        CHECK(plain.size() == n_plain);
        CHECK(text_plain.find("@HD") == std::string::npos && text_sorted == "@HD\tVN:1.6\tSO:coordinate\n" + text_plain);          // the index's header has no @HD line
        BamRecordPtrVector want = plain;
        std::stable_sort(want.begin(), want.end(), by_coordinate);
        CHECK(!std::is_sorted(plain.begin(), plain.end(), by_coordinate));   // there was something to sort
        CHECK(same(sorted, want));

        // ---- SetRegion on one reference interval: what a brute-force filter of the record list gives
        size_t n_region = 0;
        {
            const int tid = want[want.size() / 2]->ChrID();
            const int32_t mid = want[want.size() / 2]->Position();
            const GenomicRegion g(tid, std::max(mid - 2000, 0), mid + 2000);
            BamRecordPtrVector brute, got;
            for (const BamRecordPtr &r : want) if (r->ChrID() == g.chr && r->Position() < g.pos2 && r->PositionEnd() > g.pos1) brute.push_back(r);
            BamReader r;
            CHECK(r.Open(f_sorted) && r.HasIndex() && r.SetRegion(g));
            for (;;) {
                BamRecordPtrVector v;
                if (!r.NextBatch(v, 100000)) break;
                got.insert(got.end(), v.begin(), v.end());
            }
            CHECK(same(got, brute) && !brute.empty());
            n_region = brute.size();
        }

        // ---- host records through WriteRecords and WriteRecord into a sorting writer
        {
            BamWriter w;
            w.SetHeader(idx->HeaderFromIndex());
            CHECK(w.UseGpu() && w.SortByCoordinate() && w.Open(f_host) && w.WriteHeader());
            const size_t cut = plain.size() / 3;
            BamRecordPtrVector a(plain.begin(), plain.begin() + (ptrdiff_t)cut), b(plain.begin() + (ptrdiff_t)cut + 1, plain.end());
            CHECK(w.WriteRecords(a) && w.WriteRecord(*plain[cut]) && w.WriteRecords(b));
            CHECK(w.Close() && w.BuildIndex());
            BamRecordPtrVector back;
            CHECK(read_all(f_host, back) && same(back, want));
        }

        // ---- the functors: the reference's comparison, ChrID as signed
        {
            BamRecordVector v;
            v.push_back(placed(1, 50, 0, 9)); v.push_back(placed(0, 70, 1, 3)); v.push_back(placed(-1, -1, 0, 2)); v.push_back(placed(0, 7, 0, 1)); v.push_back(placed(1, 5));
            std::sort(v.begin(), v.end(), BamRecordSort::ByReadPosition());
            const int want_tid[5] = {-1, 0, 0, 1, 1}, want_pos[5] = {-1, 7, 70, 5, 50};
            for (int i = 0; i < 5; ++i) CHECK(v[(size_t)i].ChrID() == want_tid[i] && v[(size_t)i].Position() == want_pos[i]);
            std::vector<const BamRecord *> p;
            for (const BamRecord &r : v) p.push_back(&r);
            std::reverse(p.begin(), p.end());
            std::sort(p.begin(), p.end(), BamRecordSort::ByReadPositionPtr());
            for (int i = 0; i < 5; ++i) CHECK(p[(size_t)i] == &v[(size_t)i]);
            std::sort(v.begin(), v.end(), BamRecordSort::ByMatePosition());
            const int want_mtid[5] = {-1, 0, 0, 0, 1}, want_mpos[5] = {-1, 1, 2, 9, 3};
            for (int i = 0; i < 5; ++i) CHECK(v[(size_t)i].MateChrID() == want_mtid[i] && v[(size_t)i].MatePosition() == want_mpos[i]);
        }
        if (fails) std::printf("sort FAILED (%d)\n", fails);
        else std::printf("sort OK %zu %zu\n", n_plain, n_region);
    } catch (const std::exception &e) {
        std::fprintf(stderr, "bam_sort_test: %s\n", e.what());
        return 1;
    }
    return fails ? 1 : 0;
}
