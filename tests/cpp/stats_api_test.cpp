// SeqLib::BamStats and SeqLib::BamReadGroup as a SeqLib user drives them, through the headers only (tests/test_cpp_stats.py).
//   stats_api_test errors                     what throws, with or without a GPU; without one also that batches are refused (no CPU fallback)
//   stats_api_test host <recs.bin>            no GPU: an addRead loop over the records of the file (u32 n, then n block_size-prefixed records); prints the text
//   stats_api_test run <bam>                  GPU: an addRead loop over Next() == addReads(BamReader&) == one half each; Merge; SetMinMapq; prints the text
//   stats_api_test builder <fa> <fq> <out>    GPU: the reads of <fq> aligned and built into records in HBM as alignToBam does it (slx_rec_upload,
//                                             slx_align_batch_device, slx_rec_build), BamStats::addBatch on that batch; the records go to <out> (the format of
//                                             recs.bin) and an addRead loop over them gives the same text, which is printed
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <fstream>
#include <iostream>
#include <sstream>
#include <string>
#include <vector>
#include "SeqLib/BamReader.h"
#include "SeqLib/BamStats.h"
#include "seqlib_amd_rec.h"

using namespace SeqLib;
#define CHECK(x) do { if (!(x)) { std::printf("FAILED line %d: %s\n", __LINE__, #x); return 1; } } while (0)
#define OK(x) do { if ((x) != SLX_OK) { std::printf("FAILED line %d: %s\n", __LINE__, slx_last_error()); return 1; } } while (0)

template <class F> static bool throws_runtime(F f, const char *what)
{
    try { f(); } catch (const std::runtime_error &e) { return std::strstr(e.what(), what) != nullptr; } catch (...) { return false; }
    return false;
}

static BamRecord from_bytes(const uint8_t *p, size_t n)
{
    bam1_t *r = bam_init1();
    auto u32 = [&](size_t at) { uint32_t v; std::memcpy(&v, p + at, 4); return v; };
    auto u16 = [&](size_t at) { uint16_t v; std::memcpy(&v, p + at, 2); return v; };
    const size_t l_data = n - 36;
    r->data = static_cast<uint8_t *>(std::malloc(l_data ? l_data : 1));
    bam1_core_t &c = r->core;
    c.tid = (int32_t)u32(4); c.pos = (int32_t)u32(8); c.l_qname = p[12]; c.qual = p[13]; c.bin = u16(14); c.n_cigar = u16(16); c.flag = u16(18);
    c.l_qseq = (int32_t)u32(20); c.mtid = (int32_t)u32(24); c.mpos = (int32_t)u32(28); c.isize = (int32_t)u32(32); c.l_extranul = 0;
    std::memcpy(r->data, p + 36, l_data);
    r->l_data = (int)l_data; r->m_data = (uint32_t)l_data;
    return BamRecord(r);
}
static std::string text_of(const BamStats &s) { std::ostringstream o; o << s; return o.str(); }

// an addRead loop over a stream of records
static void add_all(BamStats &s, const std::vector<uint8_t> &stream, const std::vector<uint64_t> &off)
{
    for (size_t i = 0; i + 1 < off.size(); ++i) { BamRecord r = from_bytes(stream.data() + off[i], (size_t)(off[i + 1] - off[i])); s.addRead(r); }
}

static int errors()
{
    BamStats s;
    BamReader closed;
    // A reader cannot be opened without a GPU (inflate and the record index run there), so "addReads throws without a GPU" can only be shown through the closed
    // reader, which throws with a GPU too; addBatch's "no HIP device" below is the assertion that holds without a GPU only.
    CHECK(throws_runtime([&] { s.addReads(closed); }, "the reader is not open"));
    CHECK(s.NumGroups() == 0 && s.Counter("records_seen") == -1);
    CHECK(text_of(s) == "ReadGroup\tReadCount\tSupplementary\tUnmapped\tMateUnmapped\tQCFailed\tDuplicate\tMappingQuality\tNM\tInsertSize\tClippedBases\tMeanPhredScore\tReadLength\n");
    CHECK(throws_runtime([&] { s.SetKnob("lds_groups", 99); }, "outside") && throws_runtime([&] { s.SetKnob("no such knob", 1); }, "unknown key"));
    CHECK(s.Counter("records_seen") == 0 && s.Counter("no such counter") == -1);
    bool threw = false;
    try { s.Group("nobody"); } catch (const std::out_of_range &) { threw = true; }
    CHECK(threw);
    BamReadGroup g("mine");
    CHECK(g.Name() == "mine" && g.Counter("reads") == 0 && g.Hist(SLX_STATS_ISIZE).numBins() == 201 && g.Hist(SLX_STATS_LEN).numBins() == 251);
    threw = false;
    try { g.Counter("no such counter"); } catch (const std::invalid_argument &) { threw = true; }
    CHECK(threw);
    const slx_rec_batch none = {0, 0, nullptr, nullptr};
    if (slx_device_count() <= 0) {
        CHECK(throws_runtime([&] { s.addBatch(none); }, "no HIP device"));
        std::printf("stats api errors OK (no GPU)\n");
    } else {
        s.addBatch(none);
        CHECK(s.NumGroups() == 0);
        std::printf("stats api errors OK (GPU)\n");
    }
    return 0;
}

static bool read_recs(const char *path, std::vector<uint8_t> &stream, std::vector<uint64_t> &off)
{
    std::ifstream f(path, std::ios::binary);
    uint32_t n = 0;
    if (!f.read((char *)&n, 4)) return false;
    stream.assign(std::istreambuf_iterator<char>(f), std::istreambuf_iterator<char>());
    off.assign(1, 0);
    for (uint32_t i = 0; i < n; ++i) {
        if (off.back() + 4 > stream.size()) return false;
        uint32_t bs;
        std::memcpy(&bs, &stream[off.back()], 4);
        off.push_back(off.back() + 4 + bs);
    }
    return off.back() == stream.size();
}

static int host(const char *path)
{
    std::vector<uint8_t> stream;
    std::vector<uint64_t> off;
    CHECK(read_recs(path, stream, off));
    BamStats s;
    add_all(s, stream, off);
    // a group by its name, and one record into a group of one's own
    const std::vector<BamReadGroup> groups = s.Groups();
    CHECK(!groups.empty() && s.NumGroups() == groups.size());
    uint64_t reads = 0;
    for (const BamReadGroup &g : groups) { reads += g.Counter("reads"); CHECK(s.Group(g.Name()).Counter("reads") == g.Counter("reads")); }
    CHECK(reads == off.size() - 1);
    BamReadGroup mine("mine");
    BamRecord r0 = from_bytes(stream.data(), (size_t)off[1]);
    mine.addRead(r0);
    CHECK(mine.Counter("reads") == 1 && mine.Hist(SLX_STATS_MAPQ).totalCount() + mine.Hist(SLX_STATS_MAPQ).NumAbove() == 1);
    // two halves merged are the whole
    BamStats a, b;
    std::vector<uint64_t> o1(off.begin(), off.begin() + off.size() / 2 + 1), o2(off.begin() + off.size() / 2, off.end());
    add_all(a, stream, o1); add_all(b, stream, o2);
    a.Merge(b);
    CHECK(text_of(a) == text_of(s));
    a.clear();
    CHECK(a.NumGroups() == 0);
    std::fputs(text_of(s).c_str(), stdout);
    return 0;
}

static int run(const char *bam)
{
    BamReader rd;
    CHECK(rd.Open(bam));
    rd.SetBatchBytes(1);          // one BGZF member a batch: several batches
    BamStats a, b, h;
    size_t n = 0;
    while (std::optional<BamRecord> r = rd.Next()) { a.addRead(*r); ++n; }
    rd.Reset();
    CHECK(b.addReads(rd) == n && n > 100);
    const std::string want = text_of(a);
    CHECK(text_of(b) == want && b.Counter("records_seen") == (int64_t)n && b.NumGroups() == a.NumGroups());
    // a read taken by Next() is not handed over again by addReads: host-added and GPU-added reads land in the same object
    rd.Reset();
    for (size_t i = 0; i < n / 2; ++i) { std::optional<BamRecord> r = rd.Next(); CHECK(r); h.addRead(*r); }
    CHECK(h.addReads(rd) == n - n / 2 && text_of(h) == want);
    // Merge: the GPU's counts of one object into another that has both kinds
    BamStats m;
    rd.Reset();
    for (size_t i = 0; i < n / 2; ++i) { std::optional<BamRecord> r = rd.Next(); CHECK(r); m.addRead(*r); }
    BamStats rest;
    CHECK(rest.addReads(rd) == n - n / 2);
    m.Merge(rest);
    CHECK(text_of(m) == want);
    for (const BamReadGroup &g : a.Groups()) {
        const BamReadGroup o = b.Group(g.Name());
        for (const char *c : {"reads", "supp", "supplementary", "bases", "nm_missing", "reverse"}) CHECK(o.Counter(c) == g.Counter(c));
        for (int k = 0; k < SLX_STATS_N_HIST; ++k) CHECK(o.Hist(k).NumBelow() == g.Hist(k).NumBelow() && o.Hist(k).NumAbove() == g.Hist(k).NumAbove() && o.Hist(k).toFileString() == g.Hist(k).toFileString());
    }
    // the eligibility knobs act on batches
    BamStats q, qh;
    q.SetMinMapq(30); q.SetExcludeFlags(0x400);
    rd.Reset();
    CHECK(q.addReads(rd) == n && q.Counter("records_counted") < (int64_t)n);
    rd.Reset();
    while (std::optional<BamRecord> r = rd.Next()) if (r->MapQuality() >= 30 && !(r->raw()->core.flag & 0x400)) qh.addRead(*r);
    CHECK(text_of(q) == text_of(qh));
    b.clear();
    CHECK(b.NumGroups() == 0);
    std::fputs(want.c_str(), stdout);
    return 0;
}

static int builder(const char *fa, const char *fq, const char *out)
{
    std::vector<std::string> names, seqs;
    {
        std::ifstream f(fq);
        std::string l[4];
        while (std::getline(f, l[0]) && std::getline(f, l[1]) && std::getline(f, l[2]) && std::getline(f, l[3]) && names.size() < 500) {
            names.push_back(l[0].substr(1, l[0].find_first_of(" \t") == std::string::npos ? std::string::npos : l[0].find_first_of(" \t") - 1));
            seqs.push_back(l[1]);
        }
    }
    CHECK(names.size() == 500);
    std::string bases, nm;
    std::vector<uint64_t> offs(1, 0), noffs(1, 0);
    for (size_t i = 0; i < seqs.size(); ++i) { bases += seqs[i]; offs.push_back(bases.size()); nm += names[i]; noffs.push_back(nm.size()); }
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
    OK(slx_rec_upload(rb, bases.data(), offs.data(), nm.data(), noffs.data(), (int64_t)seqs.size(), &d_bases, &d_offs, &d_names, &d_noffs));
    slx_hits dh;
    OK(slx_align_batch_device(al, &opt, d_bases, d_offs, (int64_t)seqs.size(), 0x1234abcd330eull, 0, 0, 0.9, 10, &dh));
    slx_rec_batch rbat;
    OK(slx_rec_build(rb, &dh, d_bases, d_offs, d_names, d_noffs, 0, &rbat));
    CHECK(rbat.n_records >= 500);
    BamStats s;
    s.addBatch(rbat);
    std::vector<uint8_t> stream((size_t)rbat.n_bytes);
    std::vector<uint64_t> off((size_t)rbat.n_records + 1);
    OK(slx_rec_to_host(rb, &rbat, stream.data(), stream.size(), off.data()));
    BamStats h;
    add_all(h, stream, off);
    CHECK(text_of(h) == text_of(s) && s.Counter("records_counted") == rbat.n_records);
    {
        std::ofstream o(out, std::ios::binary);
        const uint32_t n = (uint32_t)rbat.n_records;
        o.write((const char *)&n, 4);
        o.write((const char *)stream.data(), (std::streamsize)stream.size());
    }
    slx_rec_free(rb); slx_aligner_free(al); slx_index_free(idx);
    std::fputs(text_of(s).c_str(), stdout);
    return 0;
}

int main(int argc, char **argv)
{
    try {
        if (argc == 2 && !std::strcmp(argv[1], "errors")) return errors();
        if (argc == 3 && !std::strcmp(argv[1], "host")) return host(argv[2]);
        if (argc == 3 && !std::strcmp(argv[1], "run")) return run(argv[2]);
        if (argc == 5 && !std::strcmp(argv[1], "builder")) return builder(argv[2], argv[3], argv[4]);
    } catch (const std::exception &e) {
        std::printf("exception: %s\n", e.what());
        return 1;
    }
    return 2;
}
