// SeqLib::BamReader over SAM text (include/SeqLib/BamReader.h, include/seqlib_amd_sam.h) compiled with g++ through the headers only and driven as a SeqLib user
// drives it (tests/test_cpp_sam.py).  Modes:
//   refuse <in.sam>                             without a GPU: Open returns false with a message, the reader stays closed
//   write <in.bam> <out.sam> <out.bam>          the records of in.bam through BamReader, written by a BamWriter(SAM) and by a BamWriter(BAM)
//   dump <in> <out.bin> <next|batch> <batch_bytes>
//       every record re-encoded from its bam1_t (block_size, the 32 fixed bytes from the core fields, the data blob) into out.bin, the header text into out.bin.hdr;
//       stdout: SAM 0|1, INDEX 0|1, REGION 0|1 (what SetRegion returned), RECORDS n
//   align <index prefix> <in> <out prefix> <batch_bytes>
//       <out>.recs.bin: the records of alignSequences(BamReader&), re-encoded; <out>.bam: the file of alignToBam(BamReader&).  srand48(4242) before each.
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

static void put32(std::string &s, uint32_t v) { s.append(reinterpret_cast<const char *>(&v), 4); }
static std::string encode(const BamRecord &r)
{
    const bam1_t *b = r.raw();
    const bam1_core_t &c = b->core;
    std::string o;
    put32(o, (uint32_t)(32 + b->l_data));
    put32(o, (uint32_t)c.tid); put32(o, (uint32_t)c.pos);
    put32(o, (uint32_t)c.bin << 16 | (uint32_t)c.qual << 8 | (uint32_t)(c.l_qname & 0xff));
    put32(o, (uint32_t)c.flag << 16 | (uint32_t)(c.n_cigar & 0xffff));
    put32(o, (uint32_t)c.l_qseq); put32(o, (uint32_t)c.mtid); put32(o, (uint32_t)c.mpos); put32(o, (uint32_t)c.isize);
    o.append(reinterpret_cast<const char *>(b->data), (size_t)b->l_data);
    return o;
}

int main(int argc, char **argv)
{
    if (argc < 3) return 2;
    const std::string mode = argv[1];
    try {
        if (mode == "refuse") {
            BamReader r;
            if (r.Open(argv[2]) || r.IsOpen() || r.Next() || r.IsSAM() || r.HasIndex()) { std::printf("refuse FAILED\n"); return 1; }
            std::printf("refuse OK\n");
            return 0;
        }
        if (mode == "write" && argc >= 5) {
            BamReader r;
            if (!r.Open(argv[2])) return 1;
            BamWriter ws(SAM), wb(BAM);
            ws.SetHeader(r.Header()); wb.SetHeader(r.Header());
            if (!ws.Open(argv[3]) || !ws.WriteHeader() || !wb.Open(argv[4]) || !wb.WriteHeader()) return 1;
            BamRecord rec;
            size_t n = 0;
            while (r.GetNextRecord(rec)) { if (!ws.WriteRecord(rec) || !wb.WriteRecord(rec)) return 1; ++n; }
            if (!ws.Close() || !wb.Close()) return 1;
            std::printf("WRITTEN %zu\n", n);
            return 0;
        }
        if (mode == "dump" && argc >= 6) {
            BamReader r;
            if (!r.Open(argv[2])) return 1;
            r.SetBatchBytes(std::atoll(argv[5]));
            const bool region = r.SetRegion(GenomicRegion(0, 0, 100000)) || r.SetRegions(GRC());
            std::ofstream out(argv[3], std::ios::binary), hdr(std::string(argv[3]) + ".hdr", std::ios::binary);
            hdr << r.Header().AsString();
            size_t n = 0;
            if (std::string(argv[4]) == "batch") {
                for (;;) {
                    BamRecordPtrVector v;
                    const size_t got = r.NextBatch(v, 1500);          // (above the slab threshold)
                    if (got != v.size()) return 1;
                    if (!got) break;
                    for (auto &p : v) { const std::string e = encode(*p); out.write(e.data(), (std::streamsize)e.size()); ++n; }
                }
            } else {
                std::string first;
                for (int i = 0; i < 10; ++i) { auto x = r.Next(); if (!x) break; first += encode(*x); }
                r.Reset();
                std::string again;
                BamRecord rec;
                while (r.GetNextRecord(rec)) { const std::string e = encode(rec); out.write(e.data(), (std::streamsize)e.size()); if (n++ < 10) again += e; }
                if (first != again) { std::printf("reset FAILED\n"); return 1; }
            }
            std::printf("SAM %d\nINDEX %d\nREGION %d\nRECORDS %zu\n", (int)r.IsSAM(), (int)r.HasIndex(), (int)region, n);
            return 0;
        }
        if (mode == "align" && argc >= 6) {
            BWAIndexPtr idx = std::make_shared<BWAIndex>();
            idx->LoadIndex(argv[2]);
            BWAAligner al(idx);
            const std::string out = argv[4];
            const long long batch_bytes = std::atoll(argv[5]);
            size_t n_a = 0;
            {
                BamReader r;
                if (!r.Open(argv[3])) return 1;
                if (batch_bytes > 0) r.SetBatchBytes(batch_bytes);
                std::vector<BamRecordPtrVector> res;
                srand48(4242);
                al.alignSequences(r, res, false, 0.9, 10, 0x900, true);
                std::ofstream o(out + ".recs.bin", std::ios::binary);
                for (auto &v : res) for (auto &p : v) { const std::string e = encode(*p); o.write(e.data(), (std::streamsize)e.size()); ++n_a; }
            }
            BamReader r;
            if (!r.Open(argv[3])) return 1;
            if (batch_bytes > 0) r.SetBatchBytes(batch_bytes);
            BamWriter w;
            w.SetHeader(idx->HeaderFromIndex());
            if (!w.UseGpu() || !w.Open(out + ".bam") || !w.WriteHeader()) return 1;
            srand48(4242);
            const size_t n_b = al.alignToBam(r, w, false, 0.9, 10, 0x900, true);
            if (!w.Close()) return 1;
            std::printf("RECORDS %zu %zu\n", n_a, n_b);
            return 0;
        }
    } catch (const std::exception &e) {
        std::fprintf(stderr, "sam_reader_test: %s\n", e.what());
        return 1;
    }
    return 2;
}
