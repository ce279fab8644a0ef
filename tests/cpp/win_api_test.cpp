// SeqLib::AssemblyWindows, FermiAssembler::AssembleRegions and BamRecord::QualityTrimmedSequence through the headers only (tests/test_cpp_win.py builds and runs it).
//   win_api_test host <records.bin> <out.txt>      no GPU: QualityTrimmedSequence of every record of the stream at the thresholds 0, 4, 41 and 93, a line
//                                                  "index threshold startpoint endpoint" each, for Python to compare; the refusals of a host-only collector
//   win_api_test asm <in.bam> <windows.txt> <how> <out.txt>
//                                                  GPU: BamReader -> AssemblyWindows (two records through addRead, the rest through addReads) -> Assemble, and
//                                                  AssembleRegions on a second reader, against the loop they replace on a third: Next(), an overlap test per
//                                                  window, AddRead's two tests, then AssembleWindows.  how: all | regions.  <windows.txt>: "chr pos1 pos2" a line.
//                                                  <out.txt>: per window "W index n_reads n_contigs", then its reads "R ordinal seq qual_hex", then "C contig"
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <fstream>
#include <iostream>
#include <string>
#include <vector>
#include "SeqLib/AssemblyWindows.h"
#include "SeqLib/BamReader.h"
#include "SeqLib/BamRecord.h"
#include "SeqLib/FermiAssembler.h"

using namespace SeqLib;

#define CHECK(x) do { if (!(x)) { std::printf("FAILED line %d: %s\n", __LINE__, #x); return 1; } } while (0)

static int host(const std::string &in, const std::string &out)
{
    FILE *f = std::fopen(in.c_str(), "rb");
    CHECK(f);
    std::vector<uint8_t> s;
    uint8_t buf[65536];
    size_t got;
    while ((got = std::fread(buf, 1, sizeof buf, f)) > 0) s.insert(s.end(), buf, buf + got);
    std::fclose(f);
    std::ofstream o(out);
    size_t n = 0;
    for (size_t at = 0; at + 36 <= s.size(); ++n) {
        uint32_t bs; std::memcpy(&bs, &s[at], 4);
        BamRecord r;
        bam1_t *b = r.raw();
        const uint8_t *p = &s[at];
        uint16_t u16; int32_t i32;
        std::memcpy(&i32, p + 4, 4); b->core.tid = i32; std::memcpy(&i32, p + 8, 4); b->core.pos = i32;
        b->core.l_qname = p[12]; b->core.qual = p[13];
        std::memcpy(&u16, p + 16, 2); b->core.n_cigar = u16; std::memcpy(&u16, p + 18, 2); b->core.flag = u16;
        std::memcpy(&i32, p + 20, 4); b->core.l_qseq = i32;
        b->l_data = (int)bs - 32; b->m_data = (uint32_t)b->l_data;
        b->data = (uint8_t *)std::malloc((size_t)b->l_data + 1);
        std::memcpy(b->data, p + 36, (size_t)b->l_data);
        for (int t : {0, 4, 41, 93}) {
            int32_t a = 7, e = 7;
            r.QualityTrimmedSequence(t, a, e);
            o << n << " " << t << " " << a << " " << e << "\n";
        }
        at += 4 + (size_t)bs;
    }
    BamRecord none;
    int32_t a = 7, e = 7;
    none.QualityTrimmedSequence(4, a, e);
    CHECK(a == 0 && e == -1);
    // a host-only collector: the knobs answer, the batch entries say where batches are collected
    GRC wins;
    wins.add(GenomicRegion(0, 100, 200));
    AssemblyWindows aw(wins, SLX_WIN_HOST);
    CHECK(aw.NumWindows() == 1 && aw.Counter("device") == -1);
    int refused = 0;
    auto bad = [&](auto call) { try { call(); } catch (const std::invalid_argument &) { ++refused; } };
    bad([&] { aw.SetQualityTrim(94); }); bad([&] { aw.SetKnob("wave_len", -1); }); bad([&] { aw.SetKnob("no_such_knob", 1); });
    aw.SetQualityTrim(4); aw.SetSkipFlags(0x900); aw.SetOriginalStrand(true);
    CHECK(refused == 3 && aw.Counter("qual_trim") == 4 && aw.Counter("skip_flags") == 0x900 && aw.Counter("original_strand") == 1);
    bool threw = false;
    try { std::vector<std::vector<std::string> > c; aw.Assemble(c); } catch (const std::runtime_error &x) { threw = std::strstr(x.what(), "collected on MI355X only") != nullptr; }
    CHECK(threw);
    std::printf("win api host OK %zu\n", n);
    return 0;
}

static bool restrict_reader(BamReader &rd, const std::string &how)
{
    if (how != "regions") return true;
    GRC grc;
    grc.add(GenomicRegion(0, 1000, 3500)); grc.add(GenomicRegion(0, 3300, 12000));          // they overlap: a record there is served twice
    return rd.SetRegions(grc);
}

static int assemble(const std::string &in, const std::string &wins_path, const std::string &how, const std::string &out)
{
    GRC wins;
    {
        std::ifstream wf(wins_path);
        int c, a, b;
        while (wf >> c >> a >> b) wins.add(GenomicRegion(c, a, b));
    }
    const size_t nw = wins.size();
    // the new route
    std::vector<std::vector<std::string> > contigs;
    std::vector<UnalignedSequenceVector> reads(nw);
    size_t n_gpu = 0;
    {
        BamReader rd;
        CHECK(rd.Open(in));
        rd.SetBatchBytes(20000);
        CHECK(restrict_reader(rd, how));
        AssemblyWindows aw(wins);
        for (int k = 0; k < 2; ++k) {          // two records of the first batch by hand: addReads then takes the rest of that batch
            std::optional<BamRecord> r = rd.Next();
            CHECK(r.has_value());
            aw.addRead(*r);
            ++n_gpu;
        }
        n_gpu += aw.addReads(rd);
        for (size_t w = 0; w < nw; ++w) { reads[w] = aw.Reads(w); CHECK(reads[w].size() == aw.NumReads(w)); }
        aw.Assemble(contigs);
        CHECK((size_t)aw.Counter("records") == n_gpu && aw.Counter("us_gather") >= 0);
        std::vector<std::vector<std::string> > again;          // the staged reads are left as they were: a second call gives the same
        aw.Assemble(again);
        CHECK(again == contigs);
        aw.Clear();
        CHECK(aw.NumReads(0) == 0);
    }
    // the one call
    std::vector<std::vector<std::string> > contigs_one;
    {
        BamReader rd;
        CHECK(rd.Open(in));
        rd.SetBatchBytes(20000);
        CHECK(restrict_reader(rd, how));
        FermiAssembler::AssembleRegions(rd, wins, contigs_one);
    }
    // the loop they replace
    std::vector<UnalignedSequenceVector> host_reads(nw);
    std::vector<std::vector<std::string> > contigs_host;
    size_t n_host = 0;
    {
        BamReader rd;
        CHECK(rd.Open(in));
        rd.SetBatchBytes(20000);
        CHECK(restrict_reader(rd, how));
        while (std::optional<BamRecord> r = rd.Next()) {
            const int64_t pos = r->Position(), reflen = (int64_t)r->PositionEnd() - pos, end = pos + ((r->AlignmentFlag() & 4) || reflen <= 0 ? 1 : reflen);
            const UnalignedSequence u(r->Qname(), r->Sequence(), r->Qualities());
            if (!u.Seq.empty() && !u.Name.empty())          // AddRead(const UnalignedSequence&)
                for (size_t w = 0; w < nw; ++w)
                    if (wins[w].chr == r->ChrID() && (int64_t)wins[w].pos2 >= pos && (int64_t)wins[w].pos1 <= end) host_reads[w].push_back(UnalignedSequence(std::to_string(n_host), u.Seq, u.Qual));
            ++n_host;
        }
        UnalignedSequenceVector flat;
        std::vector<int64_t> win_off(1, 0);
        for (size_t w = 0; w < nw; ++w) { flat.insert(flat.end(), host_reads[w].begin(), host_reads[w].end()); win_off.push_back((int64_t)flat.size()); }
        FermiAssembler::AssembleWindows(flat, win_off, contigs_host);
    }
    CHECK(n_gpu == n_host);
    CHECK(contigs.size() == nw && contigs == contigs_host && contigs_one == contigs_host);
    std::ofstream o(out);
    size_t total_reads = 0, total_contigs = 0;
    for (size_t w = 0; w < nw; ++w) {
        CHECK(reads[w].size() == host_reads[w].size());
        o << "W " << w << " " << reads[w].size() << " " << contigs[w].size() << "\n";
        for (size_t i = 0; i < reads[w].size(); ++i) {
            CHECK(reads[w][i].Name == host_reads[w][i].Name && reads[w][i].Seq == host_reads[w][i].Seq && reads[w][i].Qual == host_reads[w][i].Qual);
            o << "R " << reads[w][i].Name << " " << reads[w][i].Seq << " ";
            for (unsigned char q : reads[w][i].Qual) { char h[3]; std::snprintf(h, sizeof h, "%02x", q); o << h; }
            o << "\n";
        }
        for (const std::string &c : contigs[w]) o << "C " << c << "\n";
        total_reads += reads[w].size(); total_contigs += contigs[w].size();
    }
    std::printf("win api asm OK %zu %zu %zu\n", n_gpu, total_reads, total_contigs);
    return 0;
}

int main(int argc, char **argv)
{
    try {
        if (argc == 4 && !std::strcmp(argv[1], "host")) return host(argv[2], argv[3]);
        if (argc == 6 && !std::strcmp(argv[1], "asm")) return assemble(argv[2], argv[3], argv[4], argv[5]);
    } catch (const std::exception &e) {
        std::printf("FAILED with an exception: %s\n", e.what());
        return 1;
    }
    return 2;
}
