// read_filter_test.cpp -- SeqLib::Filter (include/SeqLib/ReadFilter.h) and the BamRecord accessors its rules call, against what tests/test_cpp_filter.py wrote
// from the Python statement of the rules (tests/filter_util.py):
//   <dir>/recs.bin    u32 n, then n block_size-prefixed records
//   <dir>/expect.txt  per record: the keep bits of the rule sets below, then full_insert_size pair_orientation interchromosomal pair_mapped num_clip num_hard_clip
//                     max_ins max_del n_bases_n, then rg=<ParseReadGroup>
//   <dir>/motifs.txt  the motif file of the "motif_links" set
// usage: read_filter_test <dir>            host only: isValid record by record, the accessors
//        read_filter_test <dir> <bam>      GPU: BamReader::SetReadFilter + NextBatch over the same records in a file, ClearReadFilter
#include <cstdio>
#include <cstring>
#include <fstream>
#include <iostream>
#include <sstream>
#include <string>
#include <vector>
#include "SeqLib/BamReader.h"
#include "SeqLib/ReadFilter.h"

using namespace SeqLib;
using namespace SeqLib::Filter;

static int fails = 0;
#define CHECK(c) do { if (!(c)) { if (++fails < 20) printf("FAIL %s:%d %s\n", __FILE__, __LINE__, #c); } } while (0)

static BamRecord from_bytes(const std::vector<uint8_t> &p)
{
    bam1_t *r = bam_init1();
    auto u32 = [&](size_t at) { uint32_t v; std::memcpy(&v, &p[at], 4); return v; };
    auto u16 = [&](size_t at) { uint16_t v; std::memcpy(&v, &p[at], 2); return v; };
    const size_t l_data = p.size() - 36;
    r->data = static_cast<uint8_t *>(std::malloc(l_data ? l_data : 1));
    bam1_core_t &c = r->core;
    c.tid = (int32_t)u32(4); c.pos = (int32_t)u32(8); c.l_qname = p[12]; c.qual = p[13]; c.bin = u16(14); c.n_cigar = u16(16); c.flag = u16(18);
    c.l_qseq = (int32_t)u32(20); c.mtid = (int32_t)u32(24); c.mpos = (int32_t)u32(28); c.isize = (int32_t)u32(32); c.l_extranul = 0;
    std::memcpy(r->data, &p[36], l_data);
    r->l_data = (int)l_data; r->m_data = (uint32_t)l_data;
    return BamRecord(r);
}

// the rule sets, in the order of the keep bits: tests/filter_util.py's "everything", "excluder", "regions_mate", "orient_rf_or_rr", "motif_links", and no filter at all
static std::vector<ReadFilterCollection> collections(const std::string &dir)
{
    std::vector<ReadFilterCollection> out(6);
    {
        AbstractRule a;
        a.mapq = Range(17, 60, false); a.isize = Range(0, 2000, false); a.nm = Range(0, 6, false); a.nbases = Range(0, 5, false); a.clip = Range(0, 60, false);
        a.len = Range(20, 400, false); a.ins = Range(0, 10, false); a.fr.setAnyOffFlag(0x200); a.SetSubsampleRate(0.8); a.SetReadGroup("grp1");
        std::ofstream(dir + "/ac_gt.txt") << "AC\nGT\n";
        a.addMotifRule(dir + "/ac_gt.txt", false);
        ReadFilter f;
        GRC g;
        g.add(GenomicRegion(0, 0, 4000)); g.add(GenomicRegion(1, 0, 4000));
        f.setRegions(g); f.AddRule(a);
        out[0].AddReadFilter(f);
    }
    {
        AbstractRule a, d, c;
        a.mapq = Range(17, 60, false); d.fr.dup.setOn(); c.clip = Range(20, 1 << 20, false);
        ReadFilter inc, exc;
        inc.AddRule(a); exc.AddRule(d); exc.AddRule(c); exc.SetExcluder(true);
        out[1].AddReadFilter(inc); out[1].AddReadFilter(exc);
    }
    {
        AbstractRule a;
        a.mapq = Range(17, 60, false);
        ReadFilter f;
        f.addRegions(GRC(GenomicRegion(0, 1000, 2000))); f.SetMateLinked(true); f.AddRule(a);
        out[2].AddReadFilter(f);
    }
    {
        AbstractRule a, b, c;
        a.fr.rf.setOn(); b.fr.rr.setOn(); c.fr.ff.setOn();
        ReadFilter f;
        f.AddRule(a); f.AddRule(b); f.AddRule(c);
        out[3].AddReadFilter(f);
    }
    {
        AbstractRule a;
        a.addMotifRule(dir + "/motifs.txt", false);
        ReadFilter f;
        f.AddRule(a);
        out[4].AddReadFilter(f);
    }
    return out;
}

int main(int argc, char **argv)
{
    if (argc < 2) return 2;
    const std::string dir = argv[1];
    std::ifstream rb(dir + "/recs.bin", std::ios::binary);
    uint32_t n = 0;
    rb.read((char *)&n, 4);
    std::vector<std::vector<uint8_t>> raw(n);
    for (auto &r : raw) {
        uint32_t bs = 0;
        rb.read((char *)&bs, 4);
        r.resize(4 + (size_t)bs);
        std::memcpy(r.data(), &bs, 4);
        rb.read((char *)r.data() + 4, bs);
    }
    CHECK(rb.good() && n > 0);
    std::ifstream ex(dir + "/expect.txt");
    std::vector<std::string> bits(n), rg(n);
    std::vector<std::vector<long>> feat(n, std::vector<long>(9));
    for (uint32_t i = 0; i < n; ++i) {
        std::string line;
        std::getline(ex, line);
        std::istringstream ss(line);
        ss >> bits[i];
        for (long &v : feat[i]) ss >> v;
        std::string tail;
        ss >> tail;
        CHECK(tail.compare(0, 3, "rg=") == 0);
        rg[i] = tail.size() >= 3 ? tail.substr(3) : "";
    }
    std::vector<ReadFilterCollection> fc = collections(dir);
    CHECK(fc[0].size() == 1 && fc[0].numRules() == 1 && fc[1].size() == 2 && fc[1].numRules() == 3 && fc[0].getAllRegions().size() == 2 && fc[5].size() == 0);

    if (argc == 2) {
        for (uint32_t i = 0; i < n; ++i) {
            BamRecord r = from_bytes(raw[i]);
            for (size_t k = 0; k < fc.size(); ++k) CHECK(fc[k].isValid(r) == (bits[i][k] == '1'));
            CHECK(r.FullInsertSize() == feat[i][0] && r.PairOrientation() == feat[i][1] && r.Interchromosomal() == (feat[i][2] != 0) && r.PairMappedFlag() == (feat[i][3] != 0));
            CHECK(r.NumClip() == feat[i][4] && r.NumHardClip() == feat[i][5] && r.MaxInsertionBases() == (uint32_t)feat[i][6] && r.MaxDeletionBases() == (uint32_t)feat[i][7]);
            CHECK(r.CountNBases() == feat[i][8] && r.ParseReadGroup() == rg[i]);
        }
        // the smaller classes answer for themselves: a rule alone, a flag rule alone, a filter's regions alone
        AbstractRule q;
        q.mapq = Range(30, 60, false);
        FlagRule dupoff;
        dupoff.dup.setOff();
        ReadFilter reg;
        reg.setRegions(GRC(GenomicRegion(0, 1000, 2000)));
        CHECK(!q.isEvery() && Range().isEvery() && Range(1, 2, true).isValid(3) && !Range(1, 2, true).isValid(2));
        size_t nq = 0, nd = 0, nr = 0;
        for (uint32_t i = 0; i < n && i < 300; ++i) {
            BamRecord r = from_bytes(raw[i]);
            const bool want_q = r.MapQuality() >= 30 && r.MapQuality() <= 60, want_d = !(r.AlignmentFlag() & 0x400);
            const bool want_r = r.ChrID() == 0 && r.Position() <= 2000 && r.PositionEnd() >= 1000;
            CHECK(q.isValid(r) == want_q && dupoff.isValid(r) == want_d && reg.isReadOverlappingRegion(r) == want_r);
            nq += want_q; nd += !want_d; nr += want_r;
        }
        CHECK(nq > 0 && nd > 0 && nr > 0);
        ReadFilterCollection only_excluders;
        ReadFilter x;
        x.SetExcluder(true); x.AddRule(q);
        only_excluders.AddReadFilter(x);
        BamRecord first = from_bytes(raw[0]);
        CHECK(!only_excluders.isValid(first));
        only_excluders.CheckHasIncluder();
        CHECK(only_excluders.size() == 2);
        bool threw = false;
        try { AbstractRule a; a.addMotifRule(dir + "/no_such_file", false); } catch (const std::runtime_error &) { threw = true; }
        CHECK(threw);
        CHECK(fc[0].Counter("seen") == (int64_t)n);
    } else {
        size_t kept_total = 0;
        for (size_t k = 0; k < fc.size(); ++k) {
            BamReader rd;
            CHECK(rd.Open(argv[2]));
            rd.SetBatchBytes(k % 2 ? 8192 : (int64_t)64 << 20);
            CHECK(rd.SetReadFilter(fc[k]));
            BamRecordPtrVector got;
            while (rd.NextBatch(got, 1000)) { }
            size_t j = 0;
            for (uint32_t i = 0; i < n; ++i) {
                if (bits[i][k] != '1') continue;
                CHECK(j < got.size() && SeqLib::detail::packed_record(got[j]->raw()) == raw[i]);
                ++j;
            }
            CHECK(j == got.size());
            kept_total += j;
            if (k == 0) {          // without the filter the reader is what it was
                rd.ClearReadFilter();
                rd.Reset();
                size_t all = 0;
                while (rd.Next()) ++all;
                CHECK(all == n);
            }
        }
        CHECK(kept_total > n);
    }
    if (fails) { printf("read_filter FAILED %d\n", fails); return 1; }
    printf("read_filter OK %u\n", n);
    return 0;
}
