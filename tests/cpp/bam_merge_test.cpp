// SeqLib::BamMerger and BamWriter::SortByCoordinate(spill_prefix), compiled with g++ through the headers only and driven as a SeqLib user drives them
// (tests/test_cpp_merge.py, which writes the inputs and holds the outputs against Python's answer).
//   bam_merge_test <directory> <k>
// The directory holds in_00.bam .. in_<k-1>.bam, coordinate-sorted, and unsorted.bam.  Written into it:
//   next.txt          "<qname> <input>" per record of the merged iteration by Next()
//   merged.bam        MergeTo
//   spilled.bam       unsorted.bam's records through a writer with SortByCoordinate(<directory>/tmp) and a budget of 40 000 bytes, then BuildIndex()
//   in_hbm.bam        the same through the plain SortByCoordinate()
// stdout: "merge OK <records> <runs>".
#include <cstdio>
#include <cstdlib>
#include <fstream>
#include <string>
#include <vector>
#include "SeqLib/BamMerger.h"
#include "SeqLib/BamReader.h"
#include "SeqLib/BamWriter.h"

using namespace SeqLib;

static int fails = 0;
#define CHECK(x) do { if (!(x)) { std::printf("FAILED line %d: %s\n", __LINE__, #x); ++fails; } } while (0)

static uint64_t key(const BamRecord &r) { return (uint64_t)(uint32_t)r.ChrID() << 32 | (uint64_t)((uint32_t)r.Position() ^ 0x80000000u); }

int main(int argc, char **argv)
{
    if (argc < 3) return 2;
    const std::string dir = argv[1];
    const int k = std::atoi(argv[2]);
    std::vector<std::string> in;
    for (int i = 0; i < k; ++i) { char nm[32]; std::snprintf(nm, sizeof nm, "/in_%02d.bam", i); in.push_back(dir + nm); }
    try {
        // ---- the merged iteration on the host
        size_t n = 0;
        {
            BamMerger m;
            CHECK(m.Header().isEmpty() && !m.Next() && !m.MergeTo(dir + "/nothing.bam"));          // no input yet
            CHECK(m.SetKnob("batch_bytes", 0x2000));
            for (const std::string &p : in) CHECK(m.AddFile(p));
            CHECK(!m.AddFile(dir + "/no_such_file.bam") && !m.AddFile("-") && m.NumFiles() == (size_t)k);
            CHECK(!m.SetKnob("by_sort", 7));
            BamReader first;
            CHECK(first.Open(in[0]));
            const BamHeader h = m.Header();
            CHECK(h.NumSequences() == first.Header().NumSequences() && h.NumSequences() > 0 && h.IDtoName(1) == first.Header().IDtoName(1));
            CHECK(h.AsString().find("SO:coordinate") != std::string::npos);
            std::ofstream names(dir + "/next.txt");
            BamRecord r;
            uint64_t prev = 0; int prev_in = -1;
            while (m.GetNextRecord(r)) {
                const uint64_t kk = key(r);
                CHECK(n == 0 || kk > prev || (kk == prev && m.LastInput() >= prev_in));          // coordinate order, ties by input
                prev = kk; prev_in = m.LastInput();
                names << r.Qname() << ' ' << m.LastInput() << '\n';
                ++n;
            }
            CHECK(!m.Next() && m.Counter("records") == (int64_t)n && m.Counter("rounds") > 10 && m.Counter("inputs") == k && m.Counter("nonsense") == -1);
            CHECK(!m.AddFile(in[0]));                                                              // the merge has begun
        }
        // ---- the batches left in HBM
        {
            BamMerger m;
            for (const std::string &p : in) CHECK(m.AddFile(p));
            slx_merge_batch b;
            int64_t recs = 0;
            while (m.NextBatch(b)) { CHECK(b.d_stream && b.d_rec_off && b.d_input && b.n_bytes >= 36 * b.n_records); recs += b.n_records; }
            CHECK(recs == (int64_t)n && b.n_records == 0);
        }
        // ---- file to file
        {
            BamMerger m;
            for (const std::string &p : in) CHECK(m.AddFile(p));
            CHECK(!m.MergeTo(in[1]) && !m.MergeTo("-"));
            CHECK(m.MergeTo(dir + "/merged.bam"));
            BamReader back;
            CHECK(back.Open(dir + "/merged.bam"));
            size_t n2 = 0;
            BamRecord r;
            while (back.GetNextRecord(r)) ++n2;
            CHECK(n2 == n);
        }
        // ---- a sorting writer that spills, and the one that holds everything
        int64_t runs = 0;
        for (int spill = 1; spill >= 0; --spill) {
            BamReader rd;
            CHECK(rd.Open(dir + "/unsorted.bam"));
            BamWriter w;
            w.SetHeader(rd.Header());
            CHECK(w.UseGpu());
            CHECK(spill ? w.SortByCoordinate(dir + "/tmp") : w.SortByCoordinate());
            CHECK(w.Open(dir + (spill ? "/spilled.bam" : "/in_hbm.bam")) && w.IsSorting() && w.WriteHeader());
            if (spill) CHECK(w.SortKnob("max_bytes", 40000));
            BamRecord r;
            size_t nw = 0;
            while (rd.GetNextRecord(r)) { CHECK(w.WriteRecord(r)); ++nw; }
            if (spill) { runs = w.SortCounter("runs"); CHECK(runs >= 2 && w.SortCounter("held_records") < (int64_t)nw); }
            else CHECK(w.SortCounter("runs") == 0);
            CHECK(w.Close());
            CHECK(w.BuildIndex());
        }
        // ---- the refused combinations
        {
            BamWriter w, host;
            CHECK(!host.SortByCoordinate(dir + "/tmp"));                                           // UseGpu() was not called: no host fallback
            CHECK(w.UseGpu() && !w.SortByCoordinate("") && w.SortByCoordinate(dir + "/tmp") && w.MarkDuplicates());
            CHECK(!w.Open(dir + "/refused.bam") && !w.IsOpen());
            CHECK(!w.SortKnob("max_bytes", 1));
        }
        if (fails) std::printf("merge FAILED (%d)\n", fails);
        else std::printf("merge OK %zu %lld\n", n, (long long)runs);
    } catch (const std::exception &e) {
        std::fprintf(stderr, "bam_merge_test: %s\n", e.what());
        return 1;
    }
    return fails ? 1 : 0;
}
