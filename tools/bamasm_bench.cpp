// bamasm_bench -- what collecting assembly windows in HBM buys, against the host loop a user would write through BamRecords, from one process:
//     gpu        BamReader -> AssemblyWindows::addReads -> finish -> slx_fml_stage_device -> slx_fml_assemble_staged, the reads never leaving HBM
//     host_loop  Next(), an overlap test per window, AddRead's two tests into an UnalignedSequenceVector per window, then FermiAssembler::AssembleWindows
//   bamasm_bench <sorted.bam> [reps]
// <sorted.bam>: scripts/make_bench_bam.py --sorted.  The windows tile every contig of the header: 25 kb, 2 kb of overlap.  Every figure is the median of reps
// runs (at least 3) after one warm-up, with the fastest and the slowest beside it; `collect` is the wall time up to the staged reads (gpu) or up to the flat
// read vector (host_loop), `total` includes the assembly, which is the same kernels on both sides.  The stage times are the collector's counters of the LAST
// repetition.  Prints one JSON line per measurement.  Built by seqlib_amd/build.py with g++ against libseqlib_amd.so.
#include <algorithm>
#include <chrono>
#include <cstdio>
#include <cstdlib>
#include <string>
#include <vector>
#include "SeqLib/AssemblyWindows.h"
#include "SeqLib/BamReader.h"
#include "SeqLib/FermiAssembler.h"

using namespace SeqLib;

static const int WIN = 25000, OVERLAP = 2000;

static double now() { return std::chrono::duration<double>(std::chrono::steady_clock::now().time_since_epoch()).count(); }
struct Stat { double med, lo, hi; };
static Stat stat(std::vector<double> v) { std::sort(v.begin(), v.end()); return Stat{v[v.size() / 2], v.front(), v.back()}; }
struct Run {
    double collect = 0, total = 0;
    long long records = 0, reads = 0, bases = 0, contigs = 0, contig_bases = 0;
    long long us_measure = 0, us_join = 0, us_extract = 0, us_entries = 0, us_sort = 0, us_gather = 0, arena = 0;
};

static void tally_contigs(const std::vector<std::vector<std::string> > &contigs, Run &r)
{
    for (const auto &w : contigs) for (const std::string &c : w) { ++r.contigs; r.contig_bases += (long long)c.size(); }
}

static bool gpu_job(const std::string &in, const GRC &wins, Run &r)
{
    const double t0 = now();
    BamReader rd;
    if (!rd.Open(in)) return false;
    AssemblyWindows aw(wins);
    r.records = (long long)aw.addReads(rd);
    size_t reads = 0;
    for (size_t w = 0; w < wins.size(); ++w) reads += aw.NumReads(w);          // (the first call finishes)
    r.reads = (long long)reads;
    r.collect = now() - t0;
    std::vector<std::vector<std::string> > contigs;
    aw.Assemble(contigs);
    r.total = now() - t0;
    tally_contigs(contigs, r);
    r.us_measure = aw.Counter("us_measure"); r.us_join = aw.Counter("us_join"); r.us_extract = aw.Counter("us_extract"); r.us_entries = aw.Counter("us_entries");
    r.us_sort = aw.Counter("us_sort"); r.us_gather = aw.Counter("us_gather"); r.arena = aw.Counter("arena_bytes_used");
    slx_win_result v;
    if (slx_win_view(aw.raw(), &v) != SLX_OK) return false;
    r.bases = v.total;
    return true;
}

static bool host_job(const std::string &in, const GRC &wins, Run &r)
{
    const double t0 = now();
    BamReader rd;
    if (!rd.Open(in)) return false;
    std::vector<UnalignedSequenceVector> per(wins.size());
    while (std::optional<BamRecord> rec = rd.Next()) {
        const int64_t pos = rec->Position(), reflen = (int64_t)rec->PositionEnd() - pos, end = pos + ((rec->AlignmentFlag() & 4) || reflen <= 0 ? 1 : reflen);
        ++r.records;
        const UnalignedSequence u(rec->Qname(), rec->Sequence(), rec->Qualities());
        if (u.Seq.empty() || u.Name.empty()) continue;
        for (size_t w = 0; w < wins.size(); ++w)
            if (wins[w].chr == rec->ChrID() && (int64_t)wins[w].pos2 >= pos && (int64_t)wins[w].pos1 <= end) per[w].push_back(u);
    }
    UnalignedSequenceVector flat;
    std::vector<int64_t> win_off(1, 0);
    for (size_t w = 0; w < wins.size(); ++w) {
        flat.insert(flat.end(), per[w].begin(), per[w].end());
        win_off.push_back((int64_t)flat.size());
    }
    for (const UnalignedSequence &u : flat) r.bases += (long long)u.Seq.size();
    r.reads = (long long)flat.size();
    r.collect = now() - t0;
    std::vector<std::vector<std::string> > contigs;
    FermiAssembler::AssembleWindows(flat, win_off, contigs);
    r.total = now() - t0;
    tally_contigs(contigs, r);
    return true;
}

static void put(const char *what, const std::vector<Run> &runs)
{
    std::vector<double> c, t;
    for (const Run &r : runs) { c.push_back(r.collect); t.push_back(r.total); }
    const Stat sc = stat(c), st = stat(t);
    const Run &r = runs.back();
    std::printf("{\"what\": \"%s\", \"unit\": \"s\", \"collect_median\": %.4f, \"collect_min\": %.4f, \"collect_max\": %.4f, \"total_median\": %.4f, \"total_min\": %.4f, \"total_max\": %.4f, "
                "\"records\": %lld, \"reads\": %lld, \"read_bases\": %lld, \"contigs\": %lld, \"contig_bases\": %lld, \"records_per_s_collect\": %.0f, "
                "\"us_measure\": %lld, \"us_join\": %lld, \"us_extract\": %lld, \"us_entries\": %lld, \"us_sort\": %lld, \"us_gather\": %lld, \"arena_bytes\": %lld}\n",
                what, sc.med, sc.lo, sc.hi, st.med, st.lo, st.hi, r.records, r.reads, r.bases, r.contigs, r.contig_bases, (double)r.records / sc.med,
                r.us_measure, r.us_join, r.us_extract, r.us_entries, r.us_sort, r.us_gather, r.arena);
    std::fflush(stdout);
}

int main(int argc, char **argv)
{
    if (argc < 2) { std::fprintf(stderr, "usage: bamasm_bench <sorted.bam> [reps]\n"); return 2; }
    const std::string in = argv[1];
    const int reps = std::max(3, argc > 2 ? std::atoi(argv[2]) : 3);
    try {
        GRC wins;
        {
            BamReader rd;
            if (!rd.Open(in)) return 1;
            const BamHeader h = rd.Header();
            for (int c = 0; c < h.NumSequences(); ++c)
                for (int a = 0; a < h.GetSequenceLength(c); a += WIN - OVERLAP) wins.add(GenomicRegion(c, a, std::min(a + WIN, h.GetSequenceLength(c)) - 1));
        }
        const char *names[2] = {"gpu", "host_loop"};
        for (int job = 0; job < 2; ++job) {
            std::vector<Run> runs;
            for (int k = 0; k <= reps; ++k) {
                Run r;
                const bool ok = job == 0 ? gpu_job(in, wins, r) : host_job(in, wins, r);
                if (!ok) { std::fprintf(stderr, "bamasm_bench: %s failed: %s\n", names[job], slx_last_error()); return 1; }
                if (k) runs.push_back(r);          // (the first run warms up)
            }
            put(names[job], runs);
        }
    } catch (const std::exception &e) {
        std::fprintf(stderr, "bamasm_bench: %s\n", e.what());
        return 1;
    }
    return 0;
}
