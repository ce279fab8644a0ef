// dup_api_test -- SeqLib::DuplicateMarker and BamWriter::MarkDuplicates through the headers only (tests/test_cpp_dup.py drives it).
//   dup_api_test host                               no GPU needed: the class refuses as it should without a device, or constructs with one
//   dup_api_test chain <in.bam> <out_dir>           BamReader -> DuplicateMarker (flags.txt: one verdict per ordinal), MarkFile (marked.bam), and
//                                                   Next() -> a sorting, marking GPU BamWriter -> Close() -> BuildIndex() (sorted.bam, sorted.bam.bai)
#include <cstdio>
#include <cstring>
#include <fstream>
#include <optional>
#include <string>
#include "SeqLib/BamReader.h"
#include "SeqLib/BamWriter.h"
#include "SeqLib/DuplicateMarker.h"

using namespace SeqLib;

static int host()
{
    try {
        DuplicateMarker m;
        if (m.Counter("device") < 0 || m.NumRecords() != 0) return 1;
        std::printf("dup api host OK device\n");
    } catch (const std::runtime_error &e) {
        if (!std::strstr(e.what(), "duplicates are marked on MI355X only")) { std::fprintf(stderr, "unexpected: %s\n", e.what()); return 1; }
        std::printf("dup api host OK refused\n");
    }
    BamWriter w(BAM);
    if (w.MarkDuplicates()) return 1;          // not before SortByCoordinate()
    return 0;
}

static int chain(const std::string &in, const std::string &dir)
{
    BamReader rd;
    if (!rd.Open(in)) return 1;
    DuplicateMarker m;
    m.SetHeader(rd.Header());
    const size_t n = m.addReads(rd);
    m.Finish();
    std::ofstream flags(dir + "/flags.txt");
    for (size_t i = 0; i < n; ++i) flags << (m.IsDuplicate(i) ? 1 : 0) << "\n";
    flags.close();
    bool threw = false;
    try { (void)m.IsDuplicate(n); } catch (const std::out_of_range &) { threw = true; }
    if (!threw) return 1;
    const long long dups = m.Counter("duplicates"), pairs = m.Counter("pairs");

    DuplicateMarker f;
    f.MarkFile(in, dir + "/marked.bam", 4096);          // batches small enough to part mates
    if (f.Counter("duplicates") != dups || f.NumRecords() != n) return 1;

    BamReader rd2;
    if (!rd2.Open(in)) return 1;
    BamWriter w(BAM);
    if (!w.UseGpu() || !w.SortByCoordinate() || !w.MarkDuplicates()) return 1;
    w.SetHeader(rd2.Header());
    if (!w.Open(dir + "/sorted.bam") || !w.IsMarking() || !w.WriteHeader()) return 1;
    size_t written = 0;
    while (std::optional<BamRecord> r = rd2.Next()) { if (!w.WriteRecord(*r)) return 1; ++written; }
    if (!w.Close() || written != n || w.MarkCounter("duplicates") != dups || w.MarkCounter("records") != (long long)n) return 1;
    if (!w.BuildIndex()) return 1;
    std::printf("dup api chain OK %zu %lld %lld\n", n, dups, pairs);
    return 0;
}

int main(int argc, char **argv)
{
    try {
        if (argc == 2 && !std::strcmp(argv[1], "host")) return host();
        if (argc == 4 && !std::strcmp(argv[1], "chain")) return chain(argv[2], argv[3]);
    } catch (const std::exception &e) {
        std::fprintf(stderr, "dup_api_test: %s\n", e.what());
        return 1;
    }
    std::fprintf(stderr, "usage: dup_api_test host | chain <in.bam> <out_dir>\n");
    return 2;
}
