// SeqLib::BamWriter with UseGpuSam() as a SeqLib user drives it (tests/test_cpp_samw.py): the reads of <reads.fq> are aligned from srand48(4242) and written as SAM
//   <dir>/host.sam       alignSequences + WriteRecords through a host BamWriter(SAM)                the definition
//   <dir>/gpu_one.sam    the same records, UseGpuSam() + WriteRecord one by one
//   <dir>/gpu_many.sam   the same records, UseGpuSam() + WriteRecords in three calls and an empty one
//   <dir>/gpu_a2b.sam    UseGpuSam() + alignToBam(reads)            <dir>/gpu_a2b.sam.gz   the same with bgzip
//   <dir>/gpu_rd.sam     UseGpuSam() + alignToBam(BamReader&) over <reads.bam>, the same reads as unaligned records
//   <dir>/gpu_fq.sam     UseGpuSam() + alignToBam(FastqReader&) over <reads.fq>
// Python compares the files.  Then the refusals: UseGpuSam() on BAM / CRAM writers and after Open(), UseGpu() / SortByCoordinate() on a SAM writer, WriteDevice
// without offsets, BuildIndex() on SAM output.
//   sam_writer_gpu_test <index prefix> <reads.fq> <reads.bam> <dir>
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
        UnalignedSequenceVector reads;
        {
            FastqReader fr(argv[2]);
            UnalignedSequence s;
            while (fr.GetNextSequence(s)) reads.push_back(s);
        }
        const BamHeader hdr = idx->HeaderFromIndex();
        std::vector<BamRecordPtrVector> res;
        srand48(4242);
        al.alignSequences(reads, res, false, 0.9, 10);
        BamRecordPtrVector recs;
        for (auto &v : res) for (auto &p : v) recs.push_back(p);

        BamWriter host(SAM), one(SAM), many(SAM), a2b(SAM), a2z(SAM), rd(SAM), fq(SAM);
        for (BamWriter *w : {&host, &one, &many, &a2b, &a2z, &rd, &fq}) w->SetHeader(hdr);
        CHECK(host.Open(dir + "/host.sam") && host.WriteHeader() && !host.IsGpuSam() && host.GpuSamCounter("records") == -1);
        for (auto &v : res) CHECK(host.WriteRecords(v));
        CHECK(host.Close());

        CHECK(one.UseGpuSam() && one.Open(dir + "/gpu_one.sam") && one.IsOpen() && one.IsGpuSam() && !one.IsGpuBam() && !one.UseGpuSam() && !one.Open(dir + "/again.sam") && one.WriteHeader());
        for (auto &p : recs) CHECK(one.WriteRecord(*p));
        CHECK(one.GpuSamCounter("records") == (int64_t)recs.size() && one.GpuSamCounter("no such counter") == -1);
        CHECK(one.Close() && !one.IsOpen() && !one.IsGpuSam() && !one.Close());

        CHECK(many.UseGpuSam(0) && many.Open(dir + "/gpu_many.sam") && many.WriteHeader());
        const size_t cut = recs.size() / 3;
        CHECK(many.WriteRecords(BamRecordPtrVector(recs.begin(), recs.begin() + (ptrdiff_t)cut)) && many.WriteRecords(BamRecordPtrVector()) &&
              many.WriteRecords(BamRecordPtrVector(recs.begin() + (ptrdiff_t)cut, recs.end())));
        CHECK(many.Close());

        CHECK(a2b.UseGpuSam() && a2b.Open(dir + "/gpu_a2b.sam") && a2b.WriteHeader());
        srand48(4242);
        const size_t n_a2b = al.alignToBam(reads, a2b, false, 0.9, 10);
        const long long fast = a2b.GpuSamCounter("fast_records"), slow = a2b.GpuSamCounter("slow_records");
        CHECK(a2b.Close());
        CHECK(a2z.UseGpuSam(-1, true) && a2z.Open(dir + "/gpu_a2b.sam.gz") && a2z.WriteHeader());
        srand48(4242);
        CHECK(al.alignToBam(reads, a2z, false, 0.9, 10) == n_a2b && a2z.Close());

        BamReader r;
        CHECK(r.Open(argv[3]) && rd.UseGpuSam() && rd.Open(dir + "/gpu_rd.sam") && rd.WriteHeader());
        srand48(4242);
        const size_t n_rd = al.alignToBam(r, rd, false, 0.9, 10);
        CHECK(rd.Close());
        FastqReader f2;
        CHECK(f2.Open(argv[2]) && fq.UseGpuSam() && fq.Open(dir + "/gpu_fq.sam") && fq.WriteHeader());
        srand48(4242);
        const size_t n_fq = al.alignToBam(f2, fq, false, 0.9, 10);
        CHECK(fq.Close());

        // what stays refused
        BamWriter bam, cram(CRAM), sam(SAM), gsam(SAM);
        bam.SetHeader(hdr); sam.SetHeader(hdr); gsam.SetHeader(hdr);
        CHECK(!bam.UseGpuSam() && !cram.UseGpuSam() && !sam.UseGpu() && !sam.SortByCoordinate() && !gsam.UseGpu());
        CHECK(gsam.UseGpuSam() && !gsam.SortByCoordinate() && gsam.Open(dir + "/edges.sam") && !gsam.UseGpuSam() && gsam.WriteHeader());
        const char dummy[4] = {0, 0, 0, 0};
        CHECK(!gsam.WriteDevice(dummy, 4) && !gsam.IsSorting());
        CHECK(gsam.WriteRecords(BamRecordPtrVector(recs.begin(), recs.begin() + 5)) && gsam.Close() && !gsam.BuildIndex());
        CHECK(sam.Open(dir + "/plain.sam") && sam.WriteHeader() && !sam.WriteDevice(dummy, 4) && !sam.WriteDevice(dummy, 4, dummy, 0) && !sam.IsGpuSam());
        bool threw = false;
        try { al.alignToBam(reads, sam, false, 0.9, 10); } catch (const std::invalid_argument &) { threw = true; }
        CHECK(threw && sam.Close());
        std::printf("sam writer OK %zu %zu %zu %zu %lld %lld\n", recs.size(), n_a2b, n_rd, n_fq, fast, slow);
    } catch (const std::exception &e) {
        std::printf("exception: %s\n", e.what());
        return 1;
    }
    return 0;
}
