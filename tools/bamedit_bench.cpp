// bamedit_bench -- what editing records in HBM buys, against the host loop a user would write through BamRecords, from one process:
//     edit      BamReader -> RecordEditor (drop XA and SA, add a constant RG:Z) -> BamWriter(UseGpu), the records never leaving HBM, against
//               Next() + RemoveTag + AddZTag + WriteRecord on the calling thread
//     calmd     BamReader -> RefGenome::WriteNmMd (NM and MD computed and written back in HBM) -> BamWriter(UseGpu), against NmMd + Next() + RemoveTag + AddIntTag +
//               AddZTag + WriteRecord
//   bamedit_bench <mapped.bam> <ref.fa> <out_dir> [reps]
// <mapped.bam>: scripts/make_bench_bam.py --sorted --ref <ref.fa>.  Every figure is the median of reps runs (at least 3) after one warm-up, with the fastest and
// the slowest beside it; the kernels' own times printed beside it are the editor's counters summed over the batches of the LAST repetition (not of the median one).  Prints one JSON line per
// measurement.  Built by seqlib_amd/build.py with g++ against libseqlib_amd.so.
#include <algorithm>
#include <chrono>
#include <cstdio>
#include <cstdlib>
#include <string>
#include <vector>
#include "SeqLib/BamReader.h"
#include "SeqLib/BamWriter.h"
#include "SeqLib/RecordEditor.h"
#include "SeqLib/RefGenome.h"

using namespace SeqLib;

static double now() { return std::chrono::duration<double>(std::chrono::steady_clock::now().time_since_epoch()).count(); }
struct Stat { double med, lo, hi; };
static Stat stat(std::vector<double> v) { std::sort(v.begin(), v.end()); return Stat{v[v.size() / 2], v.front(), v.back()}; }
struct Run { double s = 0; long long records = 0, bytes_in = 0, bytes_out = 0, us_size = 0, us_scan = 0, us_gather = 0; };
static void put(const char *what, const std::vector<Run> &runs)
{
    std::vector<double> t;
    for (const Run &r : runs) t.push_back(r.s);
    const Stat s = stat(t);
    const Run &r = runs.back();
    std::printf("{\"what\": \"%s\", \"unit\": \"s\", \"median\": %.4f, \"min\": %.4f, \"max\": %.4f, \"records\": %lld, \"records_per_s\": %.0f, \"bytes_in\": %lld, \"GB_per_s\": %.3f, "
                "\"us_size\": %lld, \"us_scan\": %lld, \"us_gather\": %lld, \"bytes_out\": %lld}\n",
                what, s.med, s.lo, s.hi, r.records, (double)r.records / s.med, r.bytes_in, (double)r.bytes_in / s.med / 1e9, r.us_size, r.us_scan, r.us_gather, r.bytes_out);
    std::fflush(stdout);
}
static void tally(Run &r, const RecordEditor &ed)
{
    r.records += ed.Counter("records"); r.bytes_in += ed.Counter("bytes_in"); r.bytes_out += ed.Counter("bytes_out");
    r.us_size += ed.Counter("us_size"); r.us_scan += ed.Counter("us_scan"); r.us_gather += ed.Counter("us_gather");
}

static bool gpu_job(const std::string &in, const std::string &out, RefGenome *ref, Run &r)
{
    const double t0 = now();
    BamReader rd;
    if (!rd.Open(in)) return false;
    BamWriter w;
    w.SetHeader(rd.Header());
    if (!w.UseGpu() || !w.Open(out) || !w.WriteHeader()) return false;
    RecordEditor ed;
    ed.DropTag("XA"); ed.DropTag("SA");
    ed.AddZTag("RG", "bench.group");
    while (ref ? ref->WriteNmMd(rd, ed) != 0 : ed.Apply(rd)) {
        const slx_edit_batch &b = ed.Batch();
        if (!w.WriteDevice(b.d_stream, b.n_bytes, b.d_rec_off, b.n_records)) return false;
        tally(r, ed);
    }
    if (!w.Close()) return false;
    r.s = now() - t0;
    return true;
}

static bool host_job(const std::string &in, const std::string &out, RefGenome *ref, Run &r)
{
    const double t0 = now();
    BamReader rd, walk;
    if (!rd.Open(in) || (ref && !walk.Open(in))) return false;
    BamWriter w;
    w.SetHeader(rd.Header());
    if (!w.Open(out) || !w.WriteHeader()) return false;
    std::vector<int32_t> nm;
    std::vector<std::string> md;
    size_t at = 0;
    while (std::optional<BamRecord> rec = rd.Next()) {
        if (ref && at == nm.size()) { at = 0; if (!ref->NmMd(walk, nm, md)) return false; }
        r.bytes_in += 36 + rec->raw()->l_data;
        rec->RemoveTag("XA"); rec->RemoveTag("SA");
        rec->AddZTag("RG", "bench.group");
        if (ref) {
            if (nm[at] >= 0) { rec->RemoveTag("NM"); rec->AddIntTag("NM", nm[at]); }
            rec->AddZTag("MD", md[at]);
            ++at;
        }
        r.bytes_out += 36 + rec->raw()->l_data;
        if (!w.WriteRecord(*rec)) return false;
        ++r.records;
    }
    if (!w.Close()) return false;
    r.s = now() - t0;
    return true;
}

int main(int argc, char **argv)
{
    if (argc < 4) { std::fprintf(stderr, "usage: bamedit_bench <mapped.bam> <ref.fa> <out_dir> [reps]\n"); return 2; }
    const std::string in = argv[1], fa = argv[2], dir = argv[3];
    const int reps = std::max(3, argc > 4 ? std::atoi(argv[4]) : 3);
    try {
        RefGenome ref;
        if (!ref.LoadIndex(fa)) return 1;
        const char *names[4] = {"edit_gpu", "edit_host_loop", "calmd_gpu", "calmd_host_loop"};
        for (int job = 0; job < 4; ++job) {
            std::vector<Run> runs;
            for (int k = 0; k <= reps; ++k) {
                Run r;
                const std::string out = dir + "/" + names[job] + ".bam";
                const bool ok = job % 2 == 0 ? gpu_job(in, out, job >= 2 ? &ref : nullptr, r) : host_job(in, out, job >= 2 ? &ref : nullptr, r);
                if (!ok) { std::fprintf(stderr, "bamedit_bench: %s failed: %s\n", names[job], slx_last_error()); return 1; }
                if (k) runs.push_back(r);          // (the first run warms up)
            }
            put(names[job], runs);
        }
    } catch (const std::exception &e) {
        std::fprintf(stderr, "bamedit_bench: %s\n", e.what());
        return 1;
    }
    return 0;
}
