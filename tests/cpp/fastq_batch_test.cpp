// FastqReader::NextBatch and the FastqReader overloads of BWAAligner (include/SeqLib/FastqReader.h, BWAAligner.h) compiled with g++ through the headers only
// and driven as a SeqLib user drives them (tests/test_cpp_fastq.py).  Every aligning route starts from srand48(4242).  Modes:
//   batch <reads.fq> <max_bytes>
//       NextBatch(UnalignedSequenceVector&) over the file against a GetNextSequence loop, field by field; then a second pass after Open.  stdout: BATCH OK <reads> <batches>
//   mix <reads.fq>
//       std::logic_error for GetNextSequence inside a NextBatch pass and for NextBatch inside a GetNextSequence pass; Open starts a new pass.  stdout: MIX OK
//   records <index prefix> <reads.fq> <max_bytes> <hardclip>
//       alignSequences(FastqReader&) against alignSequences(vector of a GetNextSequence loop): every record's fields.  stdout: RECORDS OK <reads> <records>
//   tobam <index prefix> <reads.fq> <out prefix> <max_bytes> <hardclip>
//       <out>.v.bam: alignToBam(vector of a GetNextSequence loop); <out>.f.bam: alignToBam(FastqReader&).  stdout: TOBAM <records v> <records f> <slow reads>
#include <cstdio>
#include <cstdlib>
#include <string>
#include <vector>
#include "SeqLib/BWAAligner.h"
#include "SeqLib/BamWriter.h"
#include "SeqLib/FastqReader.h"

using namespace SeqLib;

static UnalignedSequenceVector per_read(const std::string &file)
{
    FastqReader r;
    if (!r.Open(file)) throw std::runtime_error("cannot open " + file);
    UnalignedSequenceVector v;
    UnalignedSequence s;
    while (r.GetNextSequence(s)) v.push_back(s);
    return v;
}

static bool same(const UnalignedSequence &a, const UnalignedSequence &b) { return a.Name == b.Name && a.Com == b.Com && a.Seq == b.Seq && a.Qual == b.Qual && a.Strand == b.Strand; }

static bool open_gpu(BamWriter &w, const BWAIndexPtr &idx, const std::string &path)
{
    w.SetHeader(idx->HeaderFromIndex());
    return w.UseGpu() && w.Open(path) && w.WriteHeader();
}

template <typename F> static bool throws_logic(F f)
{
    try { f(); } catch (const std::logic_error &) { return true; } catch (...) { return false; }
    return false;
}

int main(int argc, char **argv)
{
    if (argc < 3) return 2;
    const std::string mode = argv[1];
    try {
        if (mode == "batch" && argc >= 4) {
            const UnalignedSequenceVector exp = per_read(argv[2]);
            FastqReader r;
            if (!r.Open(argv[2])) return 1;
            size_t batches = 0;
            for (int pass = 0; pass < 2; ++pass) {
                UnalignedSequenceVector got, part;
                while (r.NextBatch(part, (size_t)std::atoll(argv[3]))) { got.insert(got.end(), part.begin(), part.end()); ++batches; }
                if (got.size() != exp.size()) { std::printf("pass %d: %zu reads, expected %zu\n", pass, got.size(), exp.size()); return 1; }
                for (size_t i = 0; i < got.size(); ++i) if (!same(got[i], exp[i])) { std::printf("pass %d: read %zu differs\n", pass, i); return 1; }
                if (r.BatchCounter("reads") != (int64_t)exp.size()) { std::printf("pass %d: counter reads = %lld\n", pass, (long long)r.BatchCounter("reads")); return 1; }
                if (!r.Open(argv[2])) return 1;
            }
            std::printf("BATCH OK %zu %zu\n", exp.size(), batches);
            return 0;
        }
        if (mode == "mix") {
            FastqReader r;
            UnalignedSequence s;
            UnalignedSequenceVector v;
            FastqBatch b;
            if (r.NextBatch(v)) { std::printf("a reader that is not open gave a batch\n"); return 1; }
            if (!r.Open(argv[2]) || !r.GetNextSequence(s)) return 1;
            if (!throws_logic([&]() { r.NextBatch(v); }) || !throws_logic([&]() { r.NextBatch(b); })) { std::printf("NextBatch inside a GetNextSequence pass did not throw\n"); return 1; }
            if (!r.GetNextSequence(s)) { std::printf("the per-read pass did not go on\n"); return 1; }
            if (!r.Open(argv[2]) || !r.NextBatch(v, 4096) || v.empty()) { std::printf("no batch after Open\n"); return 1; }
            if (!throws_logic([&]() { r.GetNextSequence(s); })) { std::printf("GetNextSequence inside a NextBatch pass did not throw\n"); return 1; }
            if (!r.NextBatch(v, 4096)) { std::printf("the batch pass did not go on\n"); return 1; }
            if (!r.Open(argv[2]) || !r.GetNextSequence(s) || s.Name.empty()) { std::printf("no read after Open\n"); return 1; }
            std::printf("MIX OK\n");
            return 0;
        }
        BWAIndexPtr idx = std::make_shared<BWAIndex>();
        idx->LoadIndex(argv[2]);
        BWAAligner al(idx);
        if (mode == "records" && argc >= 6) {
            const UnalignedSequenceVector reads = per_read(argv[3]);
            const bool hardclip = std::atoi(argv[5]) != 0;
            std::vector<BamRecordPtrVector> a, b;
            srand48(4242);
            al.alignSequences(reads, a, hardclip, 0.9, 10);
            FastqReader r;
            if (!r.Open(argv[3])) return 1;
            srand48(4242);
            al.alignSequences(r, b, hardclip, 0.9, 10, (size_t)std::atoll(argv[4]));
            if (a.size() != b.size() || a.size() != reads.size()) { std::printf("%zu and %zu vectors for %zu reads\n", a.size(), b.size(), reads.size()); return 1; }
            size_t n = 0;
            for (size_t i = 0; i < a.size(); ++i) {
                if (a[i].size() != b[i].size()) { std::printf("read %zu: %zu and %zu records\n", i, a[i].size(), b[i].size()); return 1; }
                for (size_t j = 0; j < a[i].size(); ++j, ++n) {
                    const BamRecord &x = *a[i][j], &y = *b[i][j];
                    if (x.Qname() != y.Qname() || x.AlignmentFlag() != y.AlignmentFlag() || x.ChrID() != y.ChrID() || x.Position() != y.Position() || x.MapQuality() != y.MapQuality() ||
                        x.CigarString() != y.CigarString() || x.Sequence() != y.Sequence()) { std::printf("read %zu record %zu differs\n", i, j); return 1; }
                }
            }
            std::printf("RECORDS OK %zu %zu\n", reads.size(), n);
            return 0;
        }
        if (mode == "tobam" && argc >= 7) {
            const UnalignedSequenceVector reads = per_read(argv[3]);
            const std::string out = argv[4];
            const bool hardclip = std::atoi(argv[6]) != 0;
            BamWriter wv, wf;
            if (!open_gpu(wv, idx, out + ".v.bam")) return 1;
            srand48(4242);
            const size_t nv = al.alignToBam(reads, wv, hardclip, 0.9, 10);
            if (!wv.Close()) return 1;
            FastqReader r;
            if (!r.Open(argv[3]) || !open_gpu(wf, idx, out + ".f.bam")) return 1;
            srand48(4242);
            const size_t nf = al.alignToBam(r, wf, hardclip, 0.9, 10, (size_t)std::atoll(argv[5]));
            if (!wf.Close()) return 1;
            std::printf("TOBAM %zu %zu %lld\n", nv, nf, (long long)r.BatchCounter("slow_reads"));
            return 0;
        }
    } catch (const std::exception &e) {
        std::fprintf(stderr, "fastq_batch_test: %s\n", e.what());
        return 1;
    }
    return 2;
}
