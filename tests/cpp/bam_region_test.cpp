// Region iteration through the C++ classes as a SeqLib user drives them (tests/test_cpp_region.py): BamWriter writes a coordinate-sorted BAM, BuildIndex()
// builds its BAI on the GPU, BamReader::Open finds it, and the shape of the reference's own test (/root/reference/tests/test_BamReader.cpp:76-85: a GRC of
// three regions, SetRegions, a Next loop) gives the records a brute-force pass over what was written gives.
//   bam_region_test <directory to write into>       stdout: "region OK <records of the three regions> <records of the single region>"
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <fstream>
#include <string>
#include <vector>
#include "SeqLib/BamReader.h"
#include "SeqLib/BamWriter.h"

using namespace SeqLib;

static int fails = 0;
#define CHECK(x) do { if (!(x)) { std::printf("FAILED line %d: %s\n", __LINE__, #x); ++fails; } } while (0)

struct Spec { std::string name; int tid, pos, len; };

// a mapped record of len bases, CIGAR <len>M; tid -1: unmapped and unplaced
static BamRecordPtr make_record(const Spec &s)
{
    auto r = std::make_shared<BamRecord>();
    bam1_t *b = r->raw();
    const uint32_t n_cig = s.tid >= 0 ? 1 : 0;
    b->core.tid = s.tid; b->core.pos = s.pos; b->core.qual = 30; b->core.flag = (uint16_t)(s.tid >= 0 ? 0 : 4); b->core.n_cigar = n_cig;
    b->core.mtid = -1; b->core.mpos = -1; b->core.isize = 0;
    b->core.l_qname = (uint16_t)(s.name.size() + 1); b->core.l_qseq = s.len;
    b->l_data = (int)(b->core.l_qname + 4 * n_cig + (size_t)(s.len + 1) / 2 + (size_t)s.len);
    b->data = (uint8_t *)std::calloc((size_t)b->l_data, 1);
    b->m_data = (uint32_t)b->l_data;
    std::memcpy(b->data, s.name.c_str(), s.name.size() + 1);
    if (n_cig) { const uint32_t w = (uint32_t)s.len << 4; std::memcpy(b->data + b->core.l_qname, &w, 4); }
    uint8_t *sq = bam_get_seq(b);
    for (int k = 0; k < s.len; ++k) { const uint8_t v = (uint8_t)(1u << ((k * 7 + s.pos) & 3)); sq[k >> 1] |= (k & 1) ? v : (uint8_t)(v << 4); }
    std::memset(bam_get_qual(b), 25, (size_t)s.len);
    return r;
}

static bool write_file(const std::string &path, int fmt, const BamHeader &hdr, const std::vector<Spec> &specs, BamWriter &w)
{
    (void)fmt;
    w.SetHeader(hdr);
    if (!w.Open(path) || !w.WriteHeader()) return false;
    for (const Spec &s : specs) if (!w.WriteRecord(*make_record(s))) return false;
    return w.Close();
}

// the records a region serves: pos < pos2 and end > pos1, the interval the reference hands to sam_itr_queryi
static std::vector<std::string> brute(const std::vector<Spec> &specs, const GenomicRegion &g)
{
    std::vector<std::string> out;
    for (const Spec &s : specs) if (s.tid == g.chr && s.pos < g.pos2 && s.pos + s.len > g.pos1) out.push_back(s.name);
    return out;
}

int main(int argc, char **argv)
{
    if (argc < 2) return 2;
    const std::string dir = argv[1];
    const BamHeader hdr(HeaderSequenceVector{HeaderSequence("chrA", 200000), HeaderSequence("chrB", 150000), HeaderSequence("chrC", 100001)});
    std::vector<Spec> specs;
    for (int tid = 0; tid < 3; ++tid)
        for (int i = 0; i < 1200; ++i) specs.push_back(Spec{"r" + std::to_string(tid) + "_" + std::to_string(i), tid, i * 75 + (i % 3), 40 + (i * 13) % 90});
    for (int i = 0; i < 25; ++i) specs.push_back(Spec{"u" + std::to_string(i), -1, -1, 50});

    const std::string bam = dir + "/sorted.bam";
    {
        BamWriter w(BAM);
        CHECK(!w.BuildIndex());                               // nothing named yet
        CHECK(write_file(bam, BAM, hdr, specs, w));
        CHECK(w.BuildIndex());
        CHECK(std::ifstream(bam + ".bai").good());
    }
    {
        BamWriter w(SAM);
        CHECK(write_file(dir + "/sorted.sam", SAM, hdr, specs, w));
        CHECK(!w.BuildIndex());                               // SAM output
        std::vector<Spec> rev(specs.rbegin() + 25, specs.rend());
        BamWriter u(BAM);
        CHECK(write_file(dir + "/unsorted.bam", BAM, hdr, rev, u));
        CHECK(!u.BuildIndex());                               // not coordinate-sorted
        CHECK(!std::ifstream(dir + "/unsorted.bam.bai").good());
    }

    BamReader r;
    CHECK(!r.HasIndex() && !r.SetRegion(GenomicRegion(0, 1, 100)));          // not open
    CHECK(r.Open(bam) && r.HasIndex());
    BamReader plain;
    CHECK(plain.Open(dir + "/unsorted.bam") && !plain.HasIndex() && !plain.SetRegion(GenomicRegion(0, 1, 100)));
    CHECK(!r.SetRegions(GRC()));                              // an empty collection
    CHECK(!r.SetRegion(std::string("chrA:1-100")) && !r.SetRegions(std::vector<int>{1}));          // any other type: refused as before
    CHECK(!r.SetRegion(GenomicRegion(7, 1, 100)));            // a reference outside the header

    // the reference test's shape: three regions, SetRegions, Next until it is empty
    GRC grc;
    grc.add(GenomicRegion("chrB:60,000-70,000", r.Header()));
    grc.add(GenomicRegion(0, 1000, 20000));
    grc.add(GenomicRegion(0, 19000, 19500));                  // overlaps the one before: its records come twice
    std::vector<std::string> want;
    for (const GenomicRegion &g : grc) { const auto b = brute(specs, g); want.insert(want.end(), b.begin(), b.end()); }
    CHECK(r.SetRegions(grc));
    std::vector<std::string> got;
    while (std::optional<BamRecord> rec = r.Next()) got.push_back(rec->Qname());
    CHECK(got == want && want.size() > 300);
    CHECK(r.Counter("regions_done") == 3 && r.Counter("region_kept") == (int64_t)want.size());

    // Reset drops the regions; SetRegion starts over
    r.Reset();
    const GenomicRegion one(2, 0, 301);
    const std::vector<std::string> want1 = brute(specs, one);
    CHECK(r.SetRegion(one));
    got.clear();
    BamRecord rec;
    while (r.GetNextRecord(rec)) got.push_back(rec.Qname());
    CHECK(got == want1 && !want1.empty());
    r.Reset();
    size_t whole = 0;
    while (r.GetNextRecord(rec)) ++whole;
    CHECK(whole == specs.size());

    // NextBatch serves the same records, in small batches of members too
    r.SetBatchBytes(20000);
    CHECK(r.SetRegions(grc));
    got.clear();
    for (;;) {
        BamRecordPtrVector v;
        if (!r.NextBatch(v, 1500)) break;
        for (const BamRecordPtr &p : v) got.push_back(p->Qname());
    }
    CHECK(got == want);

    if (fails) std::printf("region FAILED (%d)\n", fails);
    else std::printf("region OK %zu %zu\n", want.size(), want1.size());
    return fails ? 1 : 0;
}
