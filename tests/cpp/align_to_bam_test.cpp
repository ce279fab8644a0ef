// BWAAligner::alignToBam (include/SeqLib/BWAAligner.h) compiled with g++ through the headers only and driven as a SeqLib user drives it
// (tests/test_gpu_rec.py).  Every route starts from srand48(4242).  Modes:
//   vec <index prefix> <reads.tsv> <out prefix> <hardclip> <keepSecFrac> <maxSecondary> [chunk]
//       reads.tsv: name<TAB>sequence per line.  <out>.b.bam: alignSequences + WriteRecords of every read's vector through a UseGpu() writer;
//       <out>.c.bam: alignToBam through another.  chunk > 0: SEQLIB_AMD_CHUNK for the call, so that it runs in several chunks.
//       stdout: RECORDS <host records> <alignToBam's return value> <the builder's "records" counter> <its "wide_hits">
//   reader <index prefix> <in.bam> <out prefix> <batch_bytes> <original_strand> <hardclip>
//       the same two routes from a BAM file (batch_bytes 0: the reader's default); stdout: RECORDS as above, then BATCHES <n>
//   edges <index prefix> <out dir> <read.tsv: one read that aligns>
//       an empty input, the writers alignToBam refuses, UseBwaMemRecords, WriteDevice's refusals, and a 255-byte name; stdout: edges OK
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <fstream>
#include <iostream>
#include <string>
#include <vector>
#include "SeqLib/BWAAligner.h"
#include "SeqLib/BamReader.h"
#include "SeqLib/BamWriter.h"

using namespace SeqLib;

static bool open_gpu(BamWriter &w, const BWAIndexPtr &idx, const std::string &path)
{
    w.SetHeader(idx->HeaderFromIndex());
    return w.UseGpu() && w.Open(path) && w.WriteHeader();
}

template <typename F> static bool throws_invalid(F f)
{
    try { f(); } catch (const std::invalid_argument &) { return true; } catch (...) { return false; }
    return false;
}

int main(int argc, char **argv)
{
    if (argc < 2) return 2;
    const std::string mode = argv[1];
    try {
        BWAIndexPtr idx = std::make_shared<BWAIndex>();
        idx->LoadIndex(argv[2]);
        BWAAligner al(idx);
        if (mode == "vec" && argc >= 8) {
            UnalignedSequenceVector reads;
            std::ifstream in(argv[3]);
            std::string line;
            while (std::getline(in, line)) {
                const size_t tab = line.find('\t');
                if (tab == std::string::npos) return 2;
                reads.emplace_back(line.substr(0, tab), line.substr(tab + 1));
            }
            const std::string out = argv[4];
            const bool hardclip = std::atoi(argv[5]) != 0;
            const double ksf = std::atof(argv[6]);
            const int maxsec = std::atoi(argv[7]);
            if (argc > 8 && std::atol(argv[8]) > 0) setenv("SEQLIB_AMD_CHUNK", argv[8], 1);
            size_t n_b = 0;
            {
                std::vector<BamRecordPtrVector> res;
                srand48(4242);
                al.alignSequences(reads, res, hardclip, ksf, maxsec);
                BamWriter w2;
                if (!open_gpu(w2, idx, out + ".b.bam")) return 1;
                for (auto &v : res) { if (!w2.WriteRecords(v)) return 1; n_b += v.size(); }
                if (!w2.Close()) return 1;
            }
            BamWriter w;
            if (!open_gpu(w, idx, out + ".c.bam")) return 1;
            srand48(4242);
            const size_t n_c = al.alignToBam(reads, w, hardclip, ksf, maxsec);
            if (!w.Close()) return 1;
            std::printf("RECORDS %zu %zu %lld %lld\n", n_b, n_c, (long long)al.RecordBuilderCounter("records"), (long long)al.RecordBuilderCounter("wide_hits"));
            return 0;
        }
        if (mode == "reader" && argc >= 8) {
            const std::string out = argv[4];
            const long long batch_bytes = std::atoll(argv[5]);
            const bool orig = std::atoi(argv[6]) != 0, hardclip = std::atoi(argv[7]) != 0;
            size_t n_b = 0;
            {
                BamReader r;
                if (!r.Open(argv[3])) return 1;
                if (batch_bytes > 0) r.SetBatchBytes(batch_bytes);
                std::vector<BamRecordPtrVector> res;
                srand48(4242);
                al.alignSequences(r, res, hardclip, 0.9, 10, 0x900, orig);
                BamWriter w2;
                if (!open_gpu(w2, idx, out + ".b.bam")) return 1;
                for (auto &v : res) { if (!w2.WriteRecords(v)) return 1; n_b += v.size(); }
                if (!w2.Close()) return 1;
            }
            BamReader r;
            if (!r.Open(argv[3])) return 1;
            if (batch_bytes > 0) r.SetBatchBytes(batch_bytes);
            BamWriter w;
            if (!open_gpu(w, idx, out + ".c.bam")) return 1;
            srand48(4242);
            const size_t n_c = al.alignToBam(r, w, hardclip, 0.9, 10, 0x900, orig);
            if (!w.Close()) return 1;
            std::printf("RECORDS %zu %zu %lld %lld\nBATCHES %lld\n", n_b, n_c, (long long)al.RecordBuilderCounter("records"), (long long)al.RecordBuilderCounter("wide_hits"),
                        (long long)al.RecordBuilderCounter("batches"));
            return 0;
        }
        if (mode == "edges" && argc >= 5) {
            const std::string dir = argv[3];
            UnalignedSequenceVector none, one;
            one.emplace_back("r1", "ACGTACGTACGTTTGACCAGTAGGATCCAGTTAGACCAGATTTAGAC");
            {   // an empty input: header + EOF by both routes
                std::vector<BamRecordPtrVector> res;
                al.alignSequences(none, res, false, 0.9, 10);
                BamWriter w2, w;
                if (!open_gpu(w2, idx, dir + "/empty.b.bam")) return 1;
                for (auto &v : res) if (!w2.WriteRecords(v)) return 1;
                if (!w2.Close() || !open_gpu(w, idx, dir + "/empty.c.bam")) return 1;
                if (al.alignToBam(none, w, false, 0.9, 10) != 0 || !w.Close()) { std::printf("empty FAILED\n"); return 1; }
            }
            {   // a host-zlib writer, a SAM writer, a closed writer
                BamWriter host, sam(SAM), closed;
                host.SetHeader(idx->HeaderFromIndex()); sam.SetHeader(idx->HeaderFromIndex());
                if (!host.Open(dir + "/host.bam") || !host.WriteHeader() || !sam.Open(dir + "/out.sam") || !sam.WriteHeader()) return 1;
                const char dummy[4] = {0, 0, 0, 0};
                if (host.WriteDevice(dummy, 4) || sam.WriteDevice(dummy, 4) || closed.WriteDevice(dummy, 4)) { std::printf("WriteDevice FAILED\n"); return 1; }
                if (!throws_invalid([&]() { al.alignToBam(one, host, false, 0.9, 10); }) || !throws_invalid([&]() { al.alignToBam(one, sam, false, 0.9, 10); }) ||
                    !throws_invalid([&]() { al.alignToBam(one, closed, false, 0.9, 10); })) { std::printf("writer kinds FAILED\n"); return 1; }
                if (!host.Close() || !sam.Close()) return 1;
            }
            {   // bwa's own records carry host-built tags
                BWAAligner mem(idx);
                mem.UseBwaMemRecords(true);
                BamWriter w;
                if (!open_gpu(w, idx, dir + "/mem.bam")) return 1;
                if (!throws_invalid([&]() { mem.alignToBam(one, w, false, 0.9, 10); })) { std::printf("UseBwaMemRecords FAILED\n"); return 1; }
                if (!w.Close()) return 1;
            }
            {   // a name a BAM record cannot hold: the call fails, nothing of the batch is in the file, the writer closes
                UnalignedSequenceVector bad;
                FILE *f = std::fopen(argv[4], "r");          // a read that aligns (from the test): name<TAB>sequence
                char name[64], seq[4096];
                if (!f || std::fscanf(f, "%63s %4095s", name, seq) != 2) return 2;
                std::fclose(f);
                bad.emplace_back(name, seq);
                bad.emplace_back(std::string(255, 'n'), seq);
                bad.emplace_back("after", seq);
                BamWriter w;
                if (!open_gpu(w, idx, dir + "/name255.bam")) return 1;
                bool failed = false;
                std::string what;
                try { al.alignToBam(bad, w, false, 0.9, 10); } catch (const std::runtime_error &e) { failed = true; what = e.what(); }
                if (!failed || what.find("read 1 ") == std::string::npos || what.find("254") == std::string::npos) { std::printf("name255 FAILED: %s\n", what.c_str()); return 1; }
                bad[1].Name.resize(254);                      // the longest name that fits: the same writer takes the batch now
                if (al.alignToBam(bad, w, false, 0.9, 10) < 3 || !w.Close()) { std::printf("name254 FAILED\n"); return 1; }
            }
            std::printf("edges OK\n");
            return 0;
        }
    } catch (const std::exception &e) {
        std::fprintf(stderr, "align_to_bam_test: %s\n", e.what());
        return 1;
    }
    return 2;
}
