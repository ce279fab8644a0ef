// SeqLib::BamReader (include/SeqLib/BamReader.h) and BWAAligner::alignSequences(BamReader&) compiled with g++ through the headers only and driven as a
// SeqLib user drives them (tests/test_cpp_bam.py, tests/test_gpu_bam.py).  Modes:
//   refuse <missing path>                       no GPU call: Header() before Open throws, a missing file opens false, Next() on a closed reader is empty
//   dump <in.bam> <out.bin> <batch_bytes> <next|batch|reset> <idx_fail> <chunk_bytes>
//       every record re-encoded from its bam1_t (block_size, the 32 fixed bytes from the core fields, the data blob) into out.bin, the header into
//       out.bin.hdr (text, a line "--", then name<TAB>length lines); stdout: RECORDS n, REPAIRED n.  reset: ten records, Reset(), then all of them.
//   refuse_open <in.bam>                        a second Open, SetRegion / SetRegions and SetCramReference are refused; operator<<
//   realign <index prefix> <reads.fq> <in.bam> <n> <original_strand>
//       A lines: alignSequences(UnalignedSequenceVector) of the FASTQ's reads; B lines: alignSequences(BamReader&) of the BAM; same lrand48 seed before each
//   roundtrip <index prefix> <reads.fq> <n> <tmp.bam>      align, BamWriter, BamReader: every record read equals the record written
//   readme <index prefix> <in.bam> <out.bam>               the reference README's read -> realign -> write loop, then its assembly-from-a-BAM loop
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
#include "SeqLib/FastqReader.h"
#include "SeqLib/FermiAssembler.h"

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
static std::string line_of(const BamRecord &r)
{
    int32_t nm = -1, as = -1, na = -1;
    r.GetIntTag("NM", nm); r.GetIntTag("AS", as); r.GetIntTag("NA", na);
    return r.Qname() + "\t" + std::to_string(r.ChrID()) + "\t" + std::to_string(r.Position()) + "\t" + std::to_string(r.AlignmentFlag()) + "\t" + std::to_string(r.MapQuality()) +
           "\t" + r.CigarString() + "\t" + std::to_string(nm) + "\t" + std::to_string(as) + "\t" + std::to_string(na) + "\t" + r.Sequence();
}

int main(int argc, char **argv)
{
    if (argc < 2) return 2;
    const std::string mode = argv[1];
    try {
        if (mode == "refuse") {
            BamReader r;
            bool threw = false;
            try { r.Header(); } catch (const std::runtime_error &) { threw = true; }
            if (!threw || r.IsOpen() || r.Next() || r.Open(argv[2]) || r.IsOpen()) { std::printf("refuse FAILED\n"); return 1; }
            BamRecord rec;
            if (r.GetNextRecord(rec)) return 1;
            std::printf("refuse OK\n");
            return 0;
        }
        if (mode == "refuse_open") {
            BamReader r;
            if (!r.Open(argv[2])) return 1;
            if (r.Open(argv[2]) || r.SetRegion(std::string("chr1:1-100")) || r.SetRegions(std::vector<int>{1}) || r.SetCramReference("x.fa") || !r.IsOpen()) { std::printf("refuse_open FAILED\n"); return 1; }
            std::cout << r << std::endl;
            r.Close();
            if (r.IsOpen() || r.Next()) return 1;
            std::printf("refuse_open OK\n");
            return 0;
        }
        if (mode == "dump") {
            BamReader r;
            if (!r.Open(argv[2])) return 1;
            r.SetBatchBytes(std::atoll(argv[4]));
            const std::string how = argv[5];
            if (std::atoi(argv[6]) && !r.SetKnob("idx_fail", 1)) return 1;
            if (!r.SetKnob("chunk_bytes", std::atoll(argv[7]))) return 1;
            std::ofstream out(argv[3], std::ios::binary), hdr(std::string(argv[3]) + ".hdr", std::ios::binary);
            hdr << r.Header().AsString() << "--\n";
            for (int i = 0; i < r.Header().NumSequences(); ++i) hdr << r.Header().IDtoName(i) << "\t" << r.Header().GetSequenceLength(i) << "\n";
            size_t n = 0;
            if (how == "reset") {
                std::string first;
                for (int i = 0; i < 10; ++i) { auto x = r.Next(); if (!x) break; first += encode(*x); }
                r.Reset();
                std::string again;
                for (int i = 0; i < 10; ++i) { auto x = r.Next(); if (!x) break; again += encode(*x); }
                if (first != again || first.empty()) { std::printf("reset FAILED\n"); return 1; }
                r.Reset();
            }
            if (how == "batch") {
                for (;;) {
                    BamRecordPtrVector v;
                    const size_t got = r.NextBatch(v, 1500);          // (above the slab threshold)
                    if (got != v.size()) return 1;
                    if (!got) break;
                    for (auto &p : v) { const std::string e = encode(*p); out.write(e.data(), (std::streamsize)e.size()); ++n; }
                }
            } else {
                BamRecord rec;
                while (r.GetNextRecord(rec)) { const std::string e = encode(rec); out.write(e.data(), (std::streamsize)e.size()); ++n; }
            }
            std::printf("RECORDS %zu\nREPAIRED %lld\nMEMBERS %lld\n", n, (long long)r.Counter("repaired_chunks"), (long long)r.Counter("members_done"));
            return 0;
        }
        if (mode == "realign") {
            BWAIndexPtr idx = std::make_shared<BWAIndex>();
            idx->LoadIndex(argv[2]);
            BWAAligner al(idx);
            const long n = std::atol(argv[5]);
            const bool orig = std::atoi(argv[6]) != 0;
            FastqReader fr(argv[3]);
            UnalignedSequenceVector reads;
            UnalignedSequence s;
            while ((long)reads.size() < n && fr.GetNextSequence(s)) reads.push_back(s);
            std::vector<BamRecordPtrVector> a, b;
            srand48(4242);
            al.alignSequences(reads, a, false, 0.9, 10);
            BamReader r;
            if (!r.Open(argv[4])) return 1;
            r.SetBatchBytes(300000);          // several batches, records cut at their ends
            srand48(4242);
            al.alignSequences(r, b, false, 0.9, 10, 0x900, orig);
            for (size_t i = 0; i < a.size(); ++i) for (auto &p : a[i]) std::printf("A\t%zu\t%s\n", i, line_of(*p).c_str());
            for (size_t i = 0; i < b.size(); ++i) for (auto &p : b[i]) std::printf("B\t%zu\t%s\n", i, line_of(*p).c_str());
            return 0;
        }
        if (mode == "roundtrip") {
            BWAIndexPtr idx = std::make_shared<BWAIndex>();
            idx->LoadIndex(argv[2]);
            BWAAligner al(idx);
            const long n = std::atol(argv[4]);
            FastqReader fr(argv[3]);
            UnalignedSequenceVector reads;
            UnalignedSequence s;
            while ((long)reads.size() < n && fr.GetNextSequence(s)) reads.push_back(s);
            std::vector<BamRecordPtrVector> res;
            al.alignSequences(reads, res, false, 0.9, 10);
            BamWriter w(BAM);
            w.SetHeader(idx->HeaderFromIndex());
            if (!w.Open(argv[5]) || !w.WriteHeader()) return 1;
            std::vector<std::string> written;
            for (auto &v : res) for (auto &p : v) { if (!w.WriteRecord(*p)) return 1; written.push_back(std::string(reinterpret_cast<const char *>(p->raw()->data), (size_t)p->raw()->l_data)); }
            if (!w.Close()) return 1;
            BamReader r;
            if (!r.Open(argv[5])) return 1;
            if (r.Header().AsString() != idx->HeaderFromIndex().AsString() || r.Header().NumSequences() != idx->NumSequences()) { std::printf("header differs\n"); return 1; }
            size_t k = 0, i = 0;
            for (auto &v : res)
                for (auto &p : v) {
                    auto x = r.Next();
                    if (!x) { std::printf("short: %zu of %zu\n", k, written.size()); return 1; }
                    const bam1_t *g = x->raw(), *e = p->raw();
                    const bool same = std::string(reinterpret_cast<const char *>(g->data), (size_t)g->l_data) == written[k] && g->core.tid == e->core.tid && g->core.pos == e->core.pos &&
                                      g->core.flag == e->core.flag && g->core.qual == e->core.qual && g->core.n_cigar == e->core.n_cigar && g->core.l_qseq == e->core.l_qseq &&
                                      g->core.mtid == e->core.mtid && g->core.mpos == e->core.mpos && g->core.isize == e->core.isize && g->core.l_qname == e->core.l_qname;
                    if (!same) { std::printf("record %zu differs\n", k); return 1; }
                    ++k; ++i;
                }
            if (r.Next()) { std::printf("more records than written\n"); return 1; }
            std::printf("roundtrip OK %zu\n", k);
            return 0;
        }
        if (mode == "readme") {
            // README.md:150-181 of the reference, with the class names of this drop-in (BWAIndex + BWAAligner for BWAWrapper, SetHeader for SetWriteHeader)
            BamReader bw;
            if (!bw.Open(argv[3])) return 1;
            BWAIndexPtr idx = std::make_shared<BWAIndex>();
            idx->LoadIndex(argv[2]);
            BWAAligner bwa(idx);
            BamWriter writer;
            writer.SetHeader(idx->HeaderFromIndex());
            if (!writer.Open(argv[4]) || !writer.WriteHeader()) return 1;
            BamRecord r;
            bool hardclip = false;
            float secondary_cutoff = 0.90f;
            int secondary_cap = 10;
            size_t n_in = 0, n_out = 0;
            while (bw.GetNextRecord(r)) {
                BamRecordVector results;
                bwa.AlignSequence(r.Sequence(), r.Qname(), results, hardclip, secondary_cutoff, secondary_cap);
                for (auto &i : results) { if (!writer.WriteRecord(i)) return 1; ++n_out; }
                ++n_in;
            }
            if (!writer.Close()) return 1;
            std::printf("REALIGNED %zu %zu\n", n_in, n_out);
            // README.md:184-216: assembly directly from a BAM
            FermiAssembler f;
            BamReader br;
            if (!br.Open(argv[3])) return 1;
            BamRecord rr;
            BamRecordVector brv;
            size_t count = 0;
            while (br.GetNextRecord(rr) && count++ < 20000) brv.push_back(std::move(rr));
            f.AddReads(brv);
            f.CorrectReads();
            f.PerformAssembly();
            std::vector<std::string> contigs = f.GetContigs();
            size_t total = 0;
            for (auto &c : contigs) total += c.size();
            std::printf("CONTIGS %zu %zu %zu\n", brv.size(), contigs.size(), total);
            return 0;
        }
    } catch (const std::exception &e) {
        std::fprintf(stderr, "bam_reader_test: %s\n", e.what());
        return 1;
    }
    return 2;
}
