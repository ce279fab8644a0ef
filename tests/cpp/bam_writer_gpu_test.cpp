// SeqLib::BamWriter with UseGpu() as a SeqLib user drives it (tests/test_cpp_bamwriter_gpu.py): fixture reads are aligned, and the records are written three
// ways -- the host writer, UseGpu() + WriteRecord one by one, UseGpu() + WriteRecords -- to <dir>/host.bam, <dir>/gpu_one.bam, <dir>/gpu_many.bam; Python compares
// the inflated streams and the ISIZE lists.  BamReader reads the GPU-written file back record by record; the same records sorted by (tid, pos) go to
// <dir>/gpu_sorted.bam, and BuildIndex() succeeds on it.
//   bam_writer_gpu_test <index prefix> <reads.fq> <n> <dir>
#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <string>
#include <vector>
#include "SeqLib/BWAAligner.h"
#include "SeqLib/BamReader.h"
#include "SeqLib/BamWriter.h"
#include "SeqLib/FastqReader.h"

using namespace SeqLib;
#define CHECK(x) do { if (!(x)) { std::printf("FAILED line %d: %s\n", __LINE__, #x); return 1; } } while (0)

int main(int argc, char **argv)
{
    if (argc < 5) return 2;
    const std::string dir = argv[4];
    try {
        BWAIndexPtr idx = std::make_shared<BWAIndex>();
        idx->LoadIndex(argv[1]);
        BWAAligner al(idx);
        const long n = std::atol(argv[3]);
        FastqReader fr(argv[2]);
        UnalignedSequenceVector reads;
        UnalignedSequence s;
        while ((long)reads.size() < n && fr.GetNextSequence(s)) reads.push_back(s);
        std::vector<BamRecordPtrVector> res;
        al.alignSequences(reads, res, false, 0.9, 10);
        BamRecordPtrVector recs;
        for (auto &v : res) for (auto &p : v) recs.push_back(p);
        const BamHeader hdr = idx->HeaderFromIndex();

        BamWriter host, one, many;
        host.SetHeader(hdr); one.SetHeader(hdr); many.SetHeader(hdr);
        CHECK(host.Open(dir + "/host.bam") && host.WriteHeader());
        for (auto &p : recs) CHECK(host.WriteRecord(*p));
        CHECK(host.Close());
        CHECK(one.UseGpu() && one.Open(dir + "/gpu_one.bam") && one.IsOpen() && !one.UseGpu() && !one.Open(dir + "/again.bam") && one.WriteHeader());
        CHECK(!one.BuildIndex());                    // still open
        for (auto &p : recs) CHECK(one.WriteRecord(*p));
        CHECK(one.Close() && !one.IsOpen() && !one.Close());
        CHECK(many.UseGpu(0) && many.Open(dir + "/gpu_many.bam") && many.WriteHeader());
        const size_t cut = recs.size() / 3;
        CHECK(many.WriteRecords(BamRecordPtrVector(recs.begin(), recs.begin() + (ptrdiff_t)cut)) && many.WriteRecords(BamRecordPtrVector()) &&
              many.WriteRecords(BamRecordPtrVector(recs.begin() + (ptrdiff_t)cut, recs.end())));
        CHECK(many.Close());

        BamReader r;
        CHECK(r.Open(dir + "/gpu_many.bam"));
        CHECK(r.Header().AsString() == hdr.AsString());
        size_t k = 0;
        for (auto &p : recs) {
            auto x = r.Next();
            CHECK(x);
            const bam1_t *g = x->raw(), *e = p->raw();
            CHECK(g->l_data == e->l_data && std::string((const char *)g->data, (size_t)g->l_data) == std::string((const char *)e->data, (size_t)e->l_data) && g->core.tid == e->core.tid &&
                  g->core.pos == e->core.pos && g->core.flag == e->core.flag && g->core.qual == e->core.qual && g->core.n_cigar == e->core.n_cigar && g->core.l_qseq == e->core.l_qseq);
            ++k;
        }
        CHECK(!r.Next());

        BamRecordPtrVector sorted = recs;
        std::stable_sort(sorted.begin(), sorted.end(), [](const BamRecordPtr &a, const BamRecordPtr &b) {
            const uint32_t ta = (uint32_t)a->raw()->core.tid, tb = (uint32_t)b->raw()->core.tid;
            return ta != tb ? ta < tb : a->raw()->core.pos < b->raw()->core.pos;
        });
        BamWriter ws;
        ws.SetHeader(hdr);
        CHECK(ws.UseGpu() && ws.Open(dir + "/gpu_sorted.bam") && ws.WriteHeader() && ws.WriteRecords(sorted) && ws.Close());
        CHECK(ws.BuildIndex());
        std::printf("writer OK %zu\n", k);
    } catch (const std::exception &e) {
        std::printf("exception: %s\n", e.what());
        return 1;
    }
    return 0;
}
