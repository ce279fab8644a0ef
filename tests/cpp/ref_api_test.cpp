// SeqLib::RefGenome through the headers only (tests/test_cpp_ref.py builds it with -Wall -Werror and links libseqlib_amd.so).
//   ref_api_test errors <fa>                  what throws, with or without a GPU; without one also that LoadIndex throws (no CPU fallback)
//   ref_api_test run <fa> <bad.fa>            GPU: LoadIndex, the accessors, QueryRegion and its exceptions, QueryRegions, FetchBatch, WriteFai; prints
//                                             "FAI" + the index text, then one "Q name p1 p2 seq" line per query, then "R name seq" per region
//   ref_api_test reader <fa> <bam> <how>      GPU: NmMd(BamReader&) batch by batch; <how> is all, regions (SetRegions over three regions) or filter (SetReadFilter,
//                                             mapq >= 30); prints "qname nm md" per record served
//   ref_api_test header <fa> <bam>            GPU: NmMd(BamReader&) must throw std::invalid_argument (a contig of another length); prints the message
//   ref_api_test mdz <fa> <fq>                GPU: the reads aligned with UseBwaMemRecords; NmMd over the records; prints "qname flag nm md MDZ NMtag" per record
//   ref_api_test builder <fa> <fq> <out>      GPU: the reads aligned and built into records in HBM as alignToBam does it; NmMd(slx_rec_batch); the records go to
//                                             <out> (u32 n, then n block_size-prefixed records); prints "nm md" per record
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <fstream>
#include <iostream>
#include <string>
#include <vector>
#include "SeqLib/BWAAligner.h"
#include "SeqLib/BWAIndex.h"
#include "SeqLib/BamReader.h"
#include "SeqLib/ReadFilter.h"
#include "SeqLib/RefGenome.h"
#include "seqlib_amd_rec.h"

using namespace SeqLib;
#define CHECK(x) do { if (!(x)) { std::printf("FAILED line %d: %s\n", __LINE__, #x); return 1; } } while (0)
#define OK(x) do { if ((x) != SLX_OK) { std::printf("FAILED line %d: %s\n", __LINE__, slx_last_error()); return 1; } } while (0)

template <class E, class F> static bool throws(F f, const char *what)
{
    try { f(); } catch (const E &e) { return std::strstr(e.what(), what) != nullptr; } catch (...) { return false; }
    return false;
}

static int errors(const char *fa)
{
    RefGenome r;
    CHECK(r.IsEmpty() && r.NumSequences() == 0 && r.Counter("contigs") == -1 && r.SequenceID("bcr") == -1);
    CHECK(throws<std::invalid_argument>([&] { (void)r.QueryRegion("bcr", 0, 10); }, "index not loaded"));
    CHECK(throws<std::invalid_argument>([&] { (void)r.QueryRegions(GRC(GenomicRegion(0, 0, 10))); }, "index not loaded"));
    CHECK(throws<std::invalid_argument>([&] { (void)r.FetchBatch(GRC(GenomicRegion(0, 0, 10))); }, "index not loaded"));
    CHECK(throws<std::invalid_argument>([&] { r.WriteFai(); }, "index not loaded"));
    CHECK(throws<std::out_of_range>([&] { (void)r.SequenceName(0); }, "no such contig"));
    std::vector<int32_t> nm;
    std::vector<std::string> md;
    slx_rec_batch none = {};
    CHECK(throws<std::invalid_argument>([&] { (void)r.NmMd(none, nm, md); }, "index not loaded"));
    CHECK(!r.LoadIndex(std::string(fa) + ".no_such_file") && r.IsEmpty());          // unreadable: false, with or without a GPU
    if (slx_device_count() == 0) {
        CHECK(throws<std::runtime_error>([&] { (void)r.LoadIndex(fa); }, "no HIP device"));
        CHECK(r.IsEmpty());
    }
    std::printf("ref api errors OK\n");
    return 0;
}

static int run(const char *fa, const char *bad)
{
    RefGenome r;
    CHECK(!r.LoadIndex(bad) && r.IsEmpty());          // malformed: false, the sentence on stderr
    CHECK(r.LoadIndex(fa) && !r.IsEmpty());
    CHECK(r.LoadIndex(fa) && !r.IsEmpty());           // again: the old one goes
    std::printf("FAI\n%s", r.FaiText().c_str());
    const int n = r.NumSequences();
    CHECK(n > 0 && r.Counter("contigs") == n);
    for (int i = 0; i < n; ++i) {
        const std::string name = r.SequenceName(i);
        const int32_t len = (int32_t)r.SequenceLength(i);
        CHECK(r.SequenceID(name) == i);
        const int32_t q[4][2] = {{0, 0}, {0, 49}, {len - 10, len + 100}, {len - 1, len - 1}};
        for (const auto &p : q) std::printf("Q %s %d %d %s\n", name.c_str(), p[0], p[1], r.QueryRegion(name, p[0], p[1]).c_str());
        CHECK(throws<std::invalid_argument>([&] { (void)r.QueryRegion(name, len, len + 5); }, "Returning empty query on " ));
    }
    const std::string first = r.SequenceName(0);
    CHECK(throws<std::invalid_argument>([&] { (void)r.QueryRegion(first, 5, 4); }, "p1 must be <= p2"));
    CHECK(throws<std::invalid_argument>([&] { (void)r.QueryRegion(first, -1, 4); }, "p1 must be >= 0"));
    CHECK(throws<std::invalid_argument>([&] { (void)r.QueryRegion("no such contig", 1, 4); }, "Could not find valid sequence"));
    CHECK(throws<std::out_of_range>([&] { (void)r.SequenceLength(n); }, "no such contig"));
    GRC grc;
    grc.add(GenomicRegion(0, 10, 19)); grc.add(GenomicRegion(n - 1, 0, 2047)); grc.add(GenomicRegion(0, (int32_t)r.SequenceLength(0) - 3, (int32_t)r.SequenceLength(0) + 3));
    grc.add(GenomicRegion(0, (int32_t)r.SequenceLength(0) + 3, (int32_t)r.SequenceLength(0) + 9));
    const UnalignedSequenceVector usv = r.QueryRegions(grc);
    CHECK(usv.size() == 4 && usv[3].Seq.empty());
    size_t total = 0;
    for (const UnalignedSequence &u : usv) { std::printf("R %s %s\n", u.Name.c_str(), u.Seq.c_str()); total += u.Seq.size(); }
    const RefBatch b = r.FetchBatch(grc);
    CHECK(b.n_regions == 4 && b.n_bytes == (int64_t)total && b.d_bases && b.d_offs);
    CHECK(throws<std::invalid_argument>([&] { (void)r.QueryRegions(GRC(GenomicRegion(n, 0, 10))); }, "which the FASTA does not have"));
    // what QueryRegions gives is what BWAIndex::ConstructIndex takes
    BWAIndex idx;
    idx.ConstructIndex(UnalignedSequenceVector(usv.begin(), usv.begin() + 2));
    CHECK(idx.NumSequences() == 2 && idx.ChrIDToName(0) == usv[0].Name);
    r.WriteFai(std::string(bad) + ".written.fai");
    std::printf("ref api run OK\n");
    return 0;
}

static int reader(const char *fa, const char *bam, const std::string &how)
{
    RefGenome r;
    CHECK(r.LoadIndex(fa));
    BamReader rd;
    CHECK(rd.Open(bam));
    rd.SetBatchBytes(6000);
    Filter::ReadFilterCollection fc;
    if (how == "regions") {
        GRC grc;
        grc.add(GenomicRegion(0, 1000, 9000)); grc.add(GenomicRegion(1, 0, 2000)); grc.add(GenomicRegion(0, 8000, 20000));
        CHECK(rd.SetRegions(grc));
    } else if (how == "filter") {
        Filter::AbstractRule q;
        q.mapq = Filter::Range(30, 255, false);
        Filter::ReadFilter f;
        f.AddRule(q);
        fc.AddReadFilter(f);
        CHECK(rd.SetReadFilter(fc));
    }
    std::vector<int32_t> nm;
    std::vector<std::string> md;
    size_t n_batches = 0, n = 0;
    while (size_t k = r.NmMd(rd, nm, md)) {
        CHECK(nm.size() == k && md.size() == k);
        for (size_t i = 0; i < k; ++i) std::printf("%d %s\n", nm[i], md[i].empty() ? "-" : md[i].c_str());
        ++n_batches; n += k;
    }
    CHECK(n_batches >= 2 && r.NmMd(rd, nm, md) == 0 && nm.empty());
    std::printf("ref api reader OK %zu\n", n);
    return 0;
}

static int header(const char *fa, const char *bam)
{
    RefGenome r;
    CHECK(r.LoadIndex(fa));
    BamReader rd;
    CHECK(rd.Open(bam));
    std::vector<int32_t> nm;
    std::vector<std::string> md;
    try { (void)r.NmMd(rd, nm, md); } catch (const std::invalid_argument &e) { std::printf("%s\n", e.what()); return 0; }
    std::printf("FAILED: no std::invalid_argument\n");
    return 1;
}

static bool read_fastq(const char *fq, size_t most, UnalignedSequenceVector &usv)
{
    std::ifstream f(fq);
    std::string l[4];
    while (usv.size() < most && std::getline(f, l[0]) && std::getline(f, l[1]) && std::getline(f, l[2]) && std::getline(f, l[3])) {
        const size_t sp = l[0].find_first_of(" \t");
        usv.push_back(UnalignedSequence(l[0].substr(1, sp == std::string::npos ? std::string::npos : sp - 1), l[1]));
    }
    return !usv.empty();
}

static int mdz(const char *fa, const char *fq)
{
    RefGenome r;
    CHECK(r.LoadIndex(fa));
    UnalignedSequenceVector usv;
    CHECK(read_fastq(fq, 3000, usv));
    BWAIndexPtr idx = std::make_shared<BWAIndex>();
    idx->LoadIndex(fa);
    BWAAligner al(idx);
    al.UseBwaMemRecords(true);
    std::vector<BamRecordPtrVector> out;
    al.alignSequences(usv, out, false, 0.9, 10);
    BamRecordPtrVector all;
    for (const BamRecordPtrVector &v : out) all.insert(all.end(), v.begin(), v.end());
    std::vector<int32_t> nm;
    std::vector<std::string> md;
    CHECK(r.NmMd(all, nm, md) == all.size());
    for (size_t i = 0; i < all.size(); ++i) {
        std::string z = "-";
        int32_t tag = -1;
        (void)all[i]->GetZTag("MD", z);
        (void)all[i]->GetIntTag("NM", tag);
        std::printf("%s %d %d %s %s %d\n", all[i]->Qname().c_str(), (int)all[i]->AlignmentFlag(), nm[i], md[i].empty() ? "-" : md[i].c_str(), z.c_str(), tag);
    }
    std::printf("ref api mdz OK %zu\n", all.size());
    return 0;
}

static int builder(const char *fa, const char *fq, const char *out)
{
    UnalignedSequenceVector usv;
    CHECK(read_fastq(fq, 500, usv));
    std::string bases, names;
    std::vector<uint64_t> offs(1, 0), noffs(1, 0);
    for (const UnalignedSequence &u : usv) { bases += u.Seq; offs.push_back(bases.size()); names += u.Name; noffs.push_back(names.size()); }
    slx_index *idx = nullptr;
    slx_aligner *al = nullptr;
    slx_rec *rb = nullptr;
    OK(slx_index_load(fa, &idx));
    const int dev = 0;
    OK(slx_aligner_create(idx, &dev, 1, &al));
    OK(slx_rec_create(al, &rb));
    slx_opt opt;
    slx_opt_init(&opt);
    void *d_bases = nullptr, *d_offs = nullptr, *d_names = nullptr, *d_noffs = nullptr;
    OK(slx_rec_upload(rb, bases.data(), offs.data(), names.data(), noffs.data(), (int64_t)usv.size(), &d_bases, &d_offs, &d_names, &d_noffs));
    slx_hits dh;
    OK(slx_align_batch_device(al, &opt, d_bases, d_offs, (int64_t)usv.size(), 0x1234abcd330eull, 0, 0, 0.9, 10, &dh));
    slx_rec_batch rbat;
    OK(slx_rec_build(rb, &dh, d_bases, d_offs, d_names, d_noffs, 0, &rbat));
    CHECK(rbat.n_records >= 500);
    RefGenome r;
    CHECK(r.LoadIndex(fa));
    std::vector<int32_t> nm;
    std::vector<std::string> md;
    CHECK(r.NmMd(rbat, nm, md) == (size_t)rbat.n_records);
    for (size_t i = 0; i < nm.size(); ++i) std::printf("%d %s\n", nm[i], md[i].empty() ? "-" : md[i].c_str());
    std::vector<uint8_t> stream((size_t)rbat.n_bytes);
    std::vector<uint64_t> off((size_t)rbat.n_records + 1);
    OK(slx_rec_to_host(rb, &rbat, stream.data(), stream.size(), off.data()));
    {
        std::ofstream o(out, std::ios::binary);
        const uint32_t n = (uint32_t)rbat.n_records;
        o.write((const char *)&n, 4);
        o.write((const char *)stream.data(), (std::streamsize)stream.size());
    }
    slx_rec_free(rb); slx_aligner_free(al); slx_index_free(idx);
    return 0;
}

int main(int argc, char **argv)
{
    try {
        if (argc == 3 && !std::strcmp(argv[1], "errors")) return errors(argv[2]);
        if (argc == 4 && !std::strcmp(argv[1], "run")) return run(argv[2], argv[3]);
        if (argc == 5 && !std::strcmp(argv[1], "reader")) return reader(argv[2], argv[3], argv[4]);
        if (argc == 4 && !std::strcmp(argv[1], "header")) return header(argv[2], argv[3]);
        if (argc == 4 && !std::strcmp(argv[1], "mdz")) return mdz(argv[2], argv[3]);
        if (argc == 5 && !std::strcmp(argv[1], "builder")) return builder(argv[2], argv[3], argv[4]);
    } catch (const std::exception &e) {
        std::printf("exception: %s\n", e.what());
        return 1;
    }
    return 2;
}
