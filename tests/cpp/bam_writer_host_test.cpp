// SeqLib::BamWriter's GPU opt-in seen from a machine without a GPU, and the unchanged host path (tests/test_bgzf_writer.py):
//   refuse <dir>    UseGpu() then Open(): false, the message of slx_last_error() on stderr, no file created; UseGpu() on a SAM or CRAM writer and after Open():
//                   refused with a message; the writer that refused goes on as a host writer
//   host <dir>      a writer without UseGpu(): <dir>/one.bam by WriteRecord, <dir>/many.bam by WriteRecords; Python rebuilds both with zlib level 6
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <sys/stat.h>
#include "SeqLib/BamWriter.h"

using namespace SeqLib;

static BamRecordPtr make_record(int i)
{
    const int len = 30 + (i * 37) % 200;
    const std::string name = "w" + std::to_string(i);
    BamRecordPtr r = std::make_shared<BamRecord>();
    bam1_t *b = r->raw();
    const bool mapped = i % 5 != 0;
    b->core.tid = mapped ? i % 3 : -1; b->core.pos = mapped ? (i * 131) % 90000 : -1;
    b->core.qual = mapped ? 60 : 0; b->core.flag = mapped ? (i % 2 ? 16 : 0) : 4;
    b->core.n_cigar = mapped ? 1 : 0;
    b->core.mtid = -1; b->core.mpos = -1; b->core.isize = 0;
    b->core.l_qname = (uint16_t)(name.size() + 1); b->core.l_qseq = len;
    b->l_data = (int)(b->core.l_qname + 4 * b->core.n_cigar + (size_t)(len + 1) / 2 + (size_t)len);
    b->data = (uint8_t *)std::calloc((size_t)b->l_data, 1);
    b->m_data = (uint32_t)b->l_data;
    std::memcpy(b->data, name.c_str(), name.size() + 1);
    if (mapped) { const uint32_t w = (uint32_t)len << 4; std::memcpy(b->data + b->core.l_qname, &w, 4); }
    uint8_t *sq = bam_get_seq(b);
    uint32_t x = (uint32_t)i * 2654435761u + 1;
    for (int k = 0; k < len; ++k) { x = x * 1664525u + 1013904223u; const uint8_t v = (uint8_t)(1u << (x >> 30)); sq[k >> 1] |= (k & 1) ? v : (uint8_t)(v << 4); }
    uint8_t *q = bam_get_qual(b);
    for (int k = 0; k < len; ++k) { x = x * 1664525u + 1013904223u; q[k] = (uint8_t)(2 + (x >> 27)); }
    return r;
}

static bool exists(const std::string &p) { struct stat sb; return stat(p.c_str(), &sb) == 0; }
#define CHECK(x) do { if (!(x)) { std::printf("FAILED line %d: %s\n", __LINE__, #x); return 1; } } while (0)

int main(int argc, char **argv)
{
    if (argc < 3) return 2;
    const std::string mode = argv[1], dir = argv[2];
    const BamHeader hdr(HeaderSequenceVector{HeaderSequence("chrA", 200000), HeaderSequence("chrB", 150000), HeaderSequence("chrC", 100001)});
    if (mode == "refuse") {
        BamWriter s(SAM), c(CRAM);
        CHECK(!s.UseGpu() && !c.UseGpu());
        {
            BamWriter w;
            w.SetHeader(hdr);
            CHECK(w.UseGpu());
            CHECK(!w.Open(dir + "/gpu.bam") && !w.IsOpen());
            CHECK(!exists(dir + "/gpu.bam"));
            CHECK(!w.WriteHeader() && !w.WriteRecord(*make_record(1)) && !w.WriteRecords(BamRecordPtrVector{make_record(1)}) && !w.Close());
        }
        BamWriter w;
        w.SetHeader(hdr);
        CHECK(w.Open(dir + "/late.bam"));
        CHECK(!w.UseGpu());                         // after Open
        CHECK(w.WriteHeader() && w.WriteRecord(*make_record(2)) && w.Close());
        std::puts("refuse OK");
        return 0;
    }
    if (mode == "host") {
        BamRecordPtrVector recs;
        for (int i = 0; i < 1500; ++i) recs.push_back(make_record(i));
        BamWriter a, b;
        a.SetHeader(hdr); b.SetHeader(hdr);
        CHECK(a.Open(dir + "/one.bam") && a.WriteHeader());
        for (auto &r : recs) CHECK(a.WriteRecord(*r));
        CHECK(a.Close());
        CHECK(b.Open(dir + "/many.bam") && b.WriteHeader());
        CHECK(b.WriteRecords(BamRecordPtrVector(recs.begin(), recs.begin() + 700)) && b.WriteRecords(BamRecordPtrVector(recs.begin() + 700, recs.end())) && b.WriteRecords(BamRecordPtrVector()));
        CHECK(b.Close());
        std::printf("host OK %zu\n", recs.size());
        return 0;
    }
    return 2;
}
